"""Inputs aimed at the rare paths of the device code under every sort engine: the vote table of
correct.hip, the string sort of irregular.hip, cc_labels of dist_cluster.hip and the windowed
edge search of directional.hip. Shared by tests/test_backend_cases.py (the preconditions, on
the CPU) and the GPU tests of those four pieces (not a test module itself).

Every builder is cached: a column is built once per session and must not be changed by a caller.
"""
from __future__ import annotations

import functools
import zlib
from collections import Counter, defaultdict

import numpy as np

# the vote table of correct.hip: a workgroup covers VOTE_TILE consecutive sorted rows and hashes
# each vote's cluster id into VOTE_SLOTS LDS slots, VOTE_PROBES probes from its home slot
VOTE_TILE = 4096
VOTE_SLOTS = 1024
VOTE_PROBES = 8

# cc_labels: every kernel is grid-stride over at most this many items per trip
CC_LAUNCH_CAP = 16384 * 256


def ascii_of(c: int, L: int) -> bytes:
    """The 2-bit code c as L bases, first base in the highest digit."""
    return bytes(b"ACGT"[(c >> (2 * (L - 1 - p))) & 3] for p in range(L))


def vote_home(cluster_id: int) -> int:
    """The home slot of a cluster id: the hash that vote() in correct.hip computes."""
    return ((cluster_id * 2654435761) & 0xFFFFFFFF) >> 22


# ------------------------------------------------------------------ vote table
class VoteCase:
    """Packed rows (codes, regular bits, caller ids, n_clusters, umi_len) of one vote-table case."""

    def __init__(self, name, codes, reg, ids, k, L):
        self.name, self.k, self.L = name, int(k), int(L)
        self.codes = np.asarray(codes, dtype=np.uint32)
        self.reg = np.asarray(reg, dtype=bool)
        self.ids = np.asarray(ids, dtype=np.uint32)
        for a in (self.codes, self.reg, self.ids):
            a.setflags(write=False)

    @property
    def n(self):
        return len(self.codes)

    def items(self, all_regular: bool):
        """The rows as the restatement takes them: a row whose regular bit is off is None."""
        return [ascii_of(int(c), self.L) if (all_regular or r) else None for c, r in zip(self.codes, self.reg)]

    def spec_ids(self, all_regular: bool):
        return [int(i) if (all_regular or r) else None for i, r in zip(self.ids, self.reg)]


def _own_id():
    """All 4096 codes of 4^6 and one more row of code 0; every distinct code is its own cluster."""
    rng = np.random.default_rng(61)
    codes = np.concatenate([np.arange(4096, dtype=np.uint32), np.zeros(1, np.uint32)])
    rng.shuffle(codes)
    reg = rng.random(len(codes)) > 0.06
    return VoteCase("own_id", codes, reg, codes.copy(), 4096, 6)


def _interleaved():
    """About 3 tiles of rows at L = 7. In code order: three singleton clusters, then one member of
    one of 40 large clusters, round robin. Inside a large cluster the largest count (5) is held by
    its second and its last but one code, which lie in the first and in the last tile; every other
    member has 1 to 3 rows. Cluster ids are a random permutation, so the ids of a tile do not
    follow the code order."""
    rng = np.random.default_rng(71)
    L, n_large, D = 7, 40, 9000
    dist = np.sort(rng.choice(4 ** L, size=D, replace=False)).astype(np.uint32)
    n_single = D - D // 4
    label = rng.permutation(n_large + n_single)  # [0, 40): the large clusters; then the singletons
    ids = np.empty(D, np.uint32)
    counts = np.ones(D, np.int64)
    members = defaultdict(list)
    single = 0
    for j in range(D):
        if j % 4 == 3:
            c = (j // 4) % n_large
            ids[j] = label[c]
            members[c].append(j)
            counts[j] = int(rng.integers(1, 4))
        else:
            ids[j] = label[n_large + single]
            single += 1
    assert single == n_single
    for m in members.values():
        counts[m[1]] = counts[m[-2]] = 5
    codes = np.repeat(dist, counts)
    row_ids = np.repeat(ids, counts)
    order = rng.permutation(len(codes))
    codes, row_ids = codes[order], row_ids[order]
    reg = rng.random(len(codes)) > 0.06
    return VoteCase("interleaved", codes, reg, row_ids, n_large + n_single, L)


def same_home_ids(count: int = 12, home: int = 613):
    """The `count` smallest cluster ids whose home slot is `home`."""
    out, i = [], 0
    while len(out) < count:
        if vote_home(i) == home:
            out.append(i)
        i += 1
    return out


def _same_home():
    """60 rows at L = 8 in 12 clusters whose ids share one home slot, so they compete for one
    window of 8 slots. Each cluster has three codes with 2, 2 and 1 rows: the smaller code of the
    tie must win wherever its vote was combined. n_clusters covers the ids; most have no row."""
    rng = np.random.default_rng(81)
    ids = same_home_ids()
    L = 8
    # all codes inside one 4096-code block of the code space: one tile for the count-table method too
    dist = (5 * VOTE_TILE + rng.choice(VOTE_TILE, size=3 * len(ids), replace=False)).astype(np.uint32)
    codes, row_ids = [], []
    for j, cid in enumerate(ids):
        for c, cnt in zip(dist[3 * j:3 * j + 3], (2, 2, 1)):
            codes += [int(c)] * cnt
            row_ids += [cid] * cnt
    order = rng.permutation(len(codes))
    codes, row_ids = np.array(codes, np.uint32)[order], np.array(row_ids, np.uint32)[order]
    return VoteCase("same_home", codes, np.ones(len(codes), bool), row_ids, max(ids) + 1, L)


@functools.lru_cache(maxsize=None)
def vote_case(name: str) -> VoteCase:
    return {"own_id": _own_id, "interleaved": _interleaved, "same_home": _same_home}[name]()


def packed_votes(case: VoteCase, all_regular: bool):
    """The votes of the packed sort method in the kernel's order: (sorted row of the run's head,
    code, cluster id, count) per distinct code of the regular rows, codes ascending."""
    keep = np.ones(case.n, bool) if all_regular else case.reg
    codes, ids = case.codes[keep], case.ids[keep]
    order = np.argsort(codes, kind="stable")
    codes, ids = codes[order], ids[order]
    heads = np.flatnonzero(np.concatenate([[True], codes[1:] != codes[:-1]])) if len(codes) else np.zeros(0, int)
    ends = np.concatenate([heads[1:], [len(codes)]])
    return [(int(h), int(codes[h]), int(ids[h]), int(e - h)) for h, e in zip(heads, ends)]


def tiles_of_votes(votes, position=lambda v: v[0]):
    """{tile: [vote, ...]}: the workgroup that casts each vote."""
    tiles = defaultdict(list)
    for v in votes:
        tiles[position(v) // VOTE_TILE].append(v)
    return dict(tiles)


def tile_profile(tiles, n_positions: int):
    """[(positions of the tile, distinct cluster ids voted for in it)] in tile order."""
    out = []
    for t in range((n_positions + VOTE_TILE - 1) // VOTE_TILE):
        rows = min(VOTE_TILE, n_positions - t * VOTE_TILE)
        out.append((rows, len({v[2] for v in tiles.get(t, [])})))
    return out


def clusters_over_tiles(tiles, at_least: int):
    """Cluster ids that get votes from at least `at_least` tiles."""
    seen = defaultdict(set)
    for t, votes in tiles.items():
        for v in votes:
            seen[v[2]].add(t)
    return sorted(c for c, ts in seen.items() if len(ts) >= at_least)


def cross_tile_ties(tiles):
    """Cluster ids whose largest count is held by two or more votes cast in different tiles."""
    top = {}
    for t, votes in tiles.items():
        for v in votes:
            best = top.setdefault(v[2], [0, set()])
            if v[3] > best[0]:
                best[0], best[1] = v[3], {t}
            elif v[3] == best[0]:
                best[1].add(t)
    return sorted(c for c, (_, ts) in top.items() if len(ts) >= 2)


# the same cases as string columns for the general path (rows sorted by (id, string rank))
@functools.lru_cache(maxsize=None)
def vote_strings(name: str):
    """(rows, ids, n_clusters, umi_len): the packed case as strings, with irregular strings (an N,
    a short row) put into clusters of regular codes by the caller's ids, and nulls whose id is
    0xFFFFFFFF. An irregular string with more rows than every regular member is the
    representative; at equal counts a regular string is."""
    case = vote_case(name)
    rng = np.random.default_rng(91)
    L = case.L
    rows = case.items(True)
    ids = [int(i) for i in case.ids]
    count = Counter(zip(rows, ids))
    top = defaultdict(int)
    for (_, i), c in count.items():
        top[i] = max(top[i], c)
    picks = rng.choice(len(rows), size=min(120, len(rows) // 2), replace=False)
    for j, r in enumerate(picks):
        s, i = bytearray(rows[r]), ids[r]
        if j % 2:
            s[int(rng.integers(0, L))] = ord("N")
        else:
            s = s[:-1]
        copies = top[i] + (j % 3) - 1  # one row fewer than the cluster's largest count, as many, one more
        rows += [bytes(s)] * copies
        ids += [i] * copies
    rows += [None] * 50
    ids += [0xFFFFFFFF] * 50
    order = rng.permutation(len(rows))
    return tuple(rows[j] for j in order), tuple(ids[j] for j in order), case.k, L


def general_votes(rows, ids):
    """The votes of the general path in the kernel's order: the non-null rows sorted by (cluster
    id, byte-lexicographic rank of the string); (sorted row of the run's head, string, id, count)."""
    live = sorted((i, x) for x, i in zip(rows, ids) if x is not None)
    votes, k = [], 0
    while k < len(live):
        e = k
        while e < len(live) and live[e] == live[k]:
            e += 1
        votes.append((k, live[k][1], live[k][0], e - k))
        k = e
    return votes, len(live)


# ------------------------------------------------------------------ string sort
HOSTILE_LEN = 8


def _replace(s: bytes, p: int, b: int) -> bytes:
    return s[:p] + bytes([b]) + s[p + 1:]


@functools.lru_cache(maxsize=None)
def hostile_distinct():
    """The distinct strings of the hostile column, in the order they were made."""
    rng = np.random.default_rng(101)
    out = []
    # prefix chains: strings that differ only in their trailing NUL bytes
    for stem in (b"", b"A", b"ACGTACG", b"ACGTACGT", b"\xff" * 7):
        out += [stem + b"\0" * z for z in range(12)]
    # chunk edges: one byte changed at the first byte, around byte 7 / 8 and at the last byte
    for n in (7, 8, 9, 15, 16, 17, 23, 24, 25, 63, 64, 65, 130, 257):
        stem = bytes(rng.integers(0, 256, n, dtype=np.uint8))
        out.append(stem)
        for p in (0, 6, 7, 8, n - 1):
            if p < n:
                out += [_replace(stem, p, b) for b in (0x00, 0x7F, 0x80, 0xFF, ord("N"))]
    # regular rows with every one-byte variant over ACGTNn\0\xff: edges at every position
    alphabet = b"ACGTNn\x00\xff"
    for _ in range(10):
        parent = bytes(b"ACGT"[d] for d in rng.integers(0, 4, HOSTILE_LEN))
        out.append(parent)
        for p in range(HOSTILE_LEN):
            out += [_replace(parent, p, b) for b in alphabet]
        for _ in range(5):  # two bytes outside ACGT: no edge to a code
            p, q = rng.choice(HOSTILE_LEN, size=2, replace=False)
            out.append(_replace(_replace(parent, int(p), alphabet[int(rng.integers(4, 8))]), int(q),
                                alphabet[int(rng.integers(4, 8))]))
    return tuple(dict.fromkeys(out))


@functools.lru_cache(maxsize=None)
def hostile_rows():
    """About 6 000 rows over the hostile strings, 1 to 11 copies each (count ties are common),
    shuffled, so equal strings are not neighbours; about 100 nulls."""
    rng = np.random.default_rng(102)
    rows = []
    for s in hostile_distinct():
        rows += [s] * int(rng.integers(1, 12))
    rows += [None] * 100
    order = rng.permutation(len(rows))
    return tuple(rows[j] for j in order)


@functools.lru_cache(maxsize=None)
def hostile_restated(umi_len: int, max_distance: int, first: int = 0):
    """correct_spec.restate of hostile_rows()[first:]."""
    from correct_spec import restate

    return restate(list(hostile_rows()[first:]), umi_len, max_distance)


@functools.lru_cache(maxsize=None)
def one_long_row():
    """One row of 257 bytes among rows of at most 3 bytes over {NUL, A, N, 0x80, 0xFF}: 33 chunk
    passes over padding. The long row extends the short row A NUL NUL by NUL bytes only."""
    rng = np.random.default_rng(103)
    sym = np.frombuffer(b"\x00AN\x80\xff", np.uint8)
    rows = [bytes(sym[rng.integers(0, 5, int(rng.integers(0, 4)))]) for _ in range(700)]
    rows += [b"A\0\0", b"A\0\0", b"A" + b"\0" * 256, None, None]
    order = rng.permutation(len(rows))
    return tuple(rows[j] for j in order)


@functools.lru_cache(maxsize=None)
def caller_id_rows():
    """(rows, ids, n_clusters) for the summary with caller ids at umi_len 8. Clusters 0 to 4 are
    hand made, every member with two rows: strings that differ only in trailing NULs, a regular
    string against smaller irregular ones, bytes on both sides of 0x80, strings that differ first
    at byte 7, 8 or 64. Then the hostile rows in 37 clusters by a checksum of their bytes, and one
    cluster without rows."""
    base = bytes(range(1, 71))
    made = [
        [b"A\0\0", b"A\0", b"A"],
        [b"ACGTACGT", b"ACGTACG", b"ACGTACG\0", b"ACGTACGN"],
        [b"\x80", b"\x7f", b"\xff", b"\x7f\x00"],
        [_replace(base, 64, 0x90), _replace(base, 64, 0x10), _replace(base, 8, 0xF0), _replace(base, 7, 0xF1)],
        [b"\0", b"", b"\0\0"],
    ]
    rows, ids = [], []
    for c, members in enumerate(made):
        for s in members:
            rows += [s, s]
            ids += [c, c]
    for s in hostile_rows():
        rows.append(s)
        ids.append(0xFFFFFFFF if s is None else len(made) + zlib.crc32(s) % 37)
    order = np.random.default_rng(104).permutation(len(rows))
    return tuple(rows[j] for j in order), tuple(ids[j] for j in order), len(made) + 37 + 1


# ------------------------------------------------------------------ cc_labels
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def cc_path(nv: int = 100_000):
    """A path through all nv vertices, vertex numbers shuffled: (nv, edges in path order)."""
    v = np.random.default_rng(111).permutation(nv).astype(np.int32)
    return (nv,) + _frozen(np.stack([v[:-1], v[1:]], axis=1))


@functools.lru_cache(maxsize=None)
def cc_star(nv: int = 10_001):
    """Every vertex joined to the largest index, edges shuffled and in both orientations."""
    rng = np.random.default_rng(112)
    leaves = rng.permutation(nv - 1).astype(np.int32)
    E = np.stack([np.full(nv - 1, nv - 1, np.int32), leaves], axis=1)
    flip = rng.random(nv - 1) < 0.5
    E[flip] = E[flip][:, ::-1]
    return (nv,) + _frozen(E)


def planted_partition(rng, nv: int, sizes):
    """Components of the given sizes over shuffled vertices: (order, comp, start, pos), where
    order[i] is the vertex at slot i, comp[i] its component, start[c] the component's first slot
    and pos[i] = i - start[comp[i]]."""
    sizes = np.asarray(sizes, dtype=np.int64)
    assert sizes.sum() == nv and (sizes > 0).all()
    order = rng.permutation(nv).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    comp = np.repeat(np.arange(len(sizes)), sizes)
    pos = np.arange(nv) - start[comp]
    return order, comp, start, pos


def partition_labels(nv, order, comp, start):
    """Labels of the planted components, numbered by their smallest vertex; and their number."""
    mins = np.minimum.reduceat(order, start)
    rank = np.empty(len(start), np.int64)
    rank[np.argsort(mins)] = np.arange(len(start))
    labels = np.empty(nv, np.int32)
    labels[order] = rank[comp]
    return labels, len(start)


def _sizes(rng, nv, low, high):
    """Random sizes in [low, high] that add up to nv (the last one cut to fit)."""
    s = rng.integers(low, high + 1, size=nv // low + 1)
    c = np.cumsum(s)
    last = int(np.searchsorted(c, nv))
    sizes = s[:last + 1].copy()
    sizes[last] -= c[last] - nv
    return sizes.tolist()


def _tree_edges(rng, order, start, comp, pos):
    """A random spanning tree of every component: slot i > its component's first joins an earlier slot."""
    kids = np.flatnonzero(pos > 0)
    parents = start[comp[kids]] + (rng.random(len(kids)) * pos[kids]).astype(np.int64)
    return np.stack([order[kids], order[parents]], axis=1)


@functools.lru_cache(maxsize=None)
def cc_small_components(nv: int = 70_001):
    """Components of 1 to 5 vertices (isolated vertices included), every tree edge given twice,
    once reversed, and 1 501 self loops, shuffled: (nv, edges, labels, n_components)."""
    rng = np.random.default_rng(113)
    order, comp, start, pos = planted_partition(rng, nv, _sizes(rng, nv, 1, 5))
    T = _tree_edges(rng, order, start, comp, pos)
    loops = rng.integers(0, nv, 1501)
    E = np.concatenate([T, T[:, ::-1], np.stack([loops, loops], axis=1)])
    E = E[rng.permutation(len(E))].astype(np.int32)
    labels, k = partition_labels(nv, order, comp, start)
    return (nv,) + _frozen(E, labels) + (k,)


@functools.lru_cache(maxsize=None)
def cc_grid_stride(nv: int = CC_LAUNCH_CAP + 3):
    """More vertices and more edges than one trip of a grid-stride kernel covers: components of 1
    to 8 vertices and three of 50 000, a shuffled spanning tree of each and extra edges inside
    components; numpy only: (nv, edges, labels, n_components)."""
    rng = np.random.default_rng(114)
    big = [50_000] * 3
    sizes = big + _sizes(rng, nv - sum(big), 1, 8)
    order, comp, start, pos = planted_partition(rng, nv, sizes)
    T = _tree_edges(rng, order, start, comp, pos)
    a = rng.integers(0, nv, nv // 3)
    size_of = np.asarray(sizes, dtype=np.int64)[comp[a]]
    b = start[comp[a]] + (rng.random(len(a)) * size_of).astype(np.int64)
    E = np.concatenate([T, np.stack([order[a], order[b]], axis=1)])
    E = E[rng.permutation(len(E))].astype(np.int32)
    labels, k = partition_labels(nv, order, comp, start)
    return (nv,) + _frozen(E, labels) + (k,)


# ------------------------------------------------------------------ directional edge search
GRID_COUNTS = (1, 1, 1, 2, 3, 5, 8, 100)


@functools.lru_cache(maxsize=None)
def grid_counts(L: int, percent: int = 100):
    """{string: count} over `percent` % of the 4^L codes (all of them at 100), counts drawn from
    GRID_COUNTS. A frozen view: callers get a fresh dict from dict(...)."""
    rng = np.random.default_rng(1000 * L + percent)
    space = 4 ** L
    codes = np.arange(space) if percent == 100 else np.sort(rng.choice(space, space * percent // 100, replace=False))
    counts = rng.choice(np.array(GRID_COUNTS), size=len(codes))
    return tuple((ascii_of(int(c), L), int(k)) for c, k in zip(codes, counts))


LARGE_COUNT_PAIRS = {
    # name: ((count of ACGA, count of ACGT), ACGA -> ACGT is an edge)
    "edge_at_2_pow_31": ((2 ** 32 - 1, 2 ** 31), True),  # 2 * 2^31 - 1 = 2^32 - 1
    "no_edge_above": ((2 ** 32 - 1, 2 ** 31 + 1), False),
    "equal_maxima": ((2 ** 32 - 1, 2 ** 32 - 1), False),
}
