"""The directional UMI-clustering spec restated twice in pure Python, shared
by tests/test_directional_spec.py and tests/test_gpu_directional.py (not a test module).

Vertices: the distinct regular strings (length L, only ACGT) with count = their rows. Edge
a -> b: one substitution apart and count(a) >= 2 * count(b) - 1. key(v) = (count, -code):
more rows first, then the smaller code. root(v) = the ancestor of v (v included) of largest
key. Irregular non-null strings are their own clusters, after the regular ones.

  roots_bfs         (a) the UMI-tools procedure: vertices in key order, a breadth-first search
                    over the out-edges from every vertex not yet claimed, first claim wins.
  roots_fixed_point (b) best[v] = max over in-neighbours u of best[u], to the fixed point.
"""
from collections import Counter, defaultdict, deque

import numpy as np

from correct_spec import is_regular, resolve_len, summarize

# The known answer: umi_len 4. The five groups of DESIGN.md §4c in one column, a null and two
# irregular strings. Each group alone behaves as its name says (KNOWN_GROUPS below); in the
# one column two edges cross groups, AAAA x10 -> GAAA x1 and TCGG x60 -> TTGG x8, so the
# count-1 plateau hangs below AAAA and the contested vertex (with TTGG) below TCGG. Both
# restatements derive KNOWN_TABLE (tests/test_directional_spec.py).
KNOWN_ROWS = ([b"AAAA"] * 10 + [b"AAAT"] * 5 + [b"AATT"] * 2 + [b"ATTT"]          # chain of depth 3
              + [b"CCCC"] * 6 + [b"CCCG"] * 6                                      # blocked pair
              + [b"GGGA", b"GGAA", b"GAAA"]                                        # count-1 plateau
              + [b"TTTT"] * 8 + [b"TTGG"] * 8 + [b"TTTG"]                          # contested vertex
              + [b"ACAC"] * 100 + [b"ACAG"] * 40 + [b"ACGG"] * 15 + [b"TCGG"] * 60  # reach through a claimed vertex
              + [None] + [b"ACGN"] * 2 + [b"ACGTA"])
KNOWN_TABLE = [(b"AAAA", 21, 7), (b"ACAC", 155, 3), (b"CCCC", 6, 1), (b"CCCG", 6, 1), (b"TCGG", 69, 3),
               (b"TTTT", 8, 1), (b"ACGN", 2, 1), (b"ACGTA", 1, 1)]
# each group on its own: rows -> {member: root}
KNOWN_GROUPS = {
    "chain": ([b"AAAA"] * 10 + [b"AAAT"] * 5 + [b"AATT"] * 2 + [b"ATTT"],
              {b"AAAA": b"AAAA", b"AAAT": b"AAAA", b"AATT": b"AAAA", b"ATTT": b"AAAA"}),
    "blocked": ([b"CCCC"] * 6 + [b"CCCG"] * 6, {b"CCCC": b"CCCC", b"CCCG": b"CCCG"}),
    "plateau": ([b"GGGA", b"GGAA", b"GAAA"], {b"GGGA": b"GAAA", b"GGAA": b"GAAA", b"GAAA": b"GAAA"}),
    "contested": ([b"TTTT"] * 8 + [b"TTGG"] * 8 + [b"TTTG"], {b"TTTT": b"TTTT", b"TTGG": b"TTGG", b"TTTG": b"TTGG"}),
    "through": ([b"ACAC"] * 100 + [b"ACAG"] * 40 + [b"ACGG"] * 15 + [b"TCGG"] * 60,
                {b"ACAC": b"ACAC", b"ACAG": b"ACAC", b"ACGG": b"ACAC", b"TCGG": b"TCGG"}),
}

_DIGIT = {65: 0, 67: 1, 71: 2, 84: 3}


def code(s: bytes) -> int:
    c = 0
    for b in s:
        c = c * 4 + _DIGIT[b]
    return c


def key(counts, v):
    return (counts[v], -code(v))


def passes(count_a: int, count_b: int) -> bool:
    """The count test of the edge a -> b."""
    return count_a >= 2 * count_b - 1


def regular_counts(items, L: int) -> Counter:
    return Counter(bytes(x) for x in items if x is not None and is_regular(bytes(x), L))


def roots_bfs(counts) -> dict:
    """(a): {vertex: root}. The search walks through vertices that are already claimed, so the
    first search to reach v starts at v's best ancestor."""
    claimed = {}
    for s in sorted(counts, key=lambda v: key(counts, v), reverse=True):
        if s in claimed:
            continue
        seen, queue = {s}, deque([s])
        while queue:
            u = queue.popleft()
            claimed.setdefault(u, s)
            for p in range(len(u)):
                for b in b"ACGT":
                    if b == u[p]:
                        continue
                    w = u[:p] + bytes([b]) + u[p + 1:]
                    if w in counts and w not in seen and passes(counts[u], counts[w]):
                        seen.add(w)
                        queue.append(w)
    return claimed


def roots_fixed_point(counts) -> dict:
    """(b): {vertex: root}. In-edges from buckets of strings equal but for one position; then
    best[v] = max(best[v], best[u] for u -> v) until nothing changes."""
    buckets = defaultdict(list)
    for v in counts:
        for p in range(len(v)):
            buckets[(p, v[:p], v[p + 1:])].append(v)
    into = defaultdict(list)
    for members in buckets.values():
        for u in members:
            for v in members:
                if u != v and passes(counts[u], counts[v]):
                    into[v].append(u)
    best = {v: (key(counts, v), v) for v in counts}
    changed = True
    while changed:
        changed = False
        for v, us in into.items():
            b = max([best[v]] + [best[u] for u in us])
            if b != best[v]:
                best[v] = b
                changed = True
    return {v: b[1] for v, b in best.items()}


def ids_of(items, L: int, roots: dict):
    """(ids with None for nulls, n_clusters): regular clusters in ascending order of their
    root's code, then the distinct irregular strings in byte-lexicographic order."""
    label = {r: k for k, r in enumerate(sorted(set(roots.values()), key=code))}
    irregular = sorted({bytes(x) for x in items if x is not None and not is_regular(bytes(x), L)})
    for s in irregular:
        label[s] = len(label)
    ids = [None if x is None else label[roots.get(bytes(x), bytes(x))] for x in items]
    return ids, len(label)


def restate(items, umi_len: int, roots_fn=roots_fixed_point):
    """(ids with None for nulls, n_clusters, table, corrected), as correct_spec.restate."""
    L = resolve_len(items, umi_len)
    ids, k = ids_of(items, L, roots_fn(regular_counts(items, L)))
    table, corrected = summarize(items, ids, k, L)
    return ids, k, table, corrected


def random_families(seed: int = 20, L: int = 8, parents: int = 2000, mean: float = 10.0, p_sub: float = 0.05):
    """Seeded UMI families: `parents` random codes, geometric family sizes of the given mean,
    every base of every read substituted with probability p_sub. About 20 k rows at the
    defaults in a crowded code space (4^8), so plateaus and contested vertices occur."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    par = rng.integers(0, 4, size=(parents, L))
    sizes = rng.geometric(1.0 / mean, size=parents)
    reads = np.repeat(par, sizes, axis=0)
    hit = rng.random(reads.shape) < p_sub
    reads = np.where(hit, (reads + rng.integers(1, 4, size=reads.shape)) % 4, reads)
    rows = [bytes(r) for r in acgt[reads]]
    order = rng.permutation(len(rows))
    return [rows[i] for i in order]
