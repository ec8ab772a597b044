"""A plain model of the k-mer minimizer filter's per-group decision (DESIGN.md §3b,
kmer_kernels.hip k_minimizer_filter) and seeded builders of the groups that reach its rare
paths. Plain Python and numpy; the GPU library is not imported here.

The rule. A candidate group (class 3, every row with observations certified, min_coverage
rows with observations or more) is emptied iff all three hold:
  * no row has more than LIST_CAP = 28 minimizer runs,
  * the group has at most CLAIM_CAP = 384 distinct minimizers,
  * no minimizer is counted min_coverage times,
a row adding a window's minimizer (the smallest of the window's K - 15 16-mers, 2-bit codes
compared as integers) once per run of consecutive windows that share it. The decision is a
function of the group's rows, K and min_coverage alone: not of how the kernel batches groups.

`decision` is written naively on purpose (every 16-mer as an integer, every window by min()
over its 16-mers, runs by comparing with the previous window): no block decomposition, no
prefix or suffix minima, nothing the kernel's own derivation could share a mistake with.
"""
from __future__ import annotations

import random
from collections import Counter, namedtuple
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np

LIST_CAP = 28    # kMzList: a row's minimizer runs the kernel lists
CLAIM_CAP = 384  # kMzClaim: distinct minimizers of one group before the kernel gives up
BATCH_GROUPS = 8  # kMzG
BATCH_ROWS = 64
C3_ROWS, C3_WORDS = 192, 576  # class 3: rows, and rows * stride (64-bit words per staged row)
CODE = {65: 0, 67: 1, 71: 2, 84: 3}

Verdict = namedtuple("Verdict", "verdict max_runs distinct max_count")


def mers16(row: bytes) -> List[int]:
    out = []
    for q in range(len(row) - 15):
        v = 0
        for c in row[q:q + 16]:
            v = (v << 2) | CODE[c]
        out.append(v)
    return out


def row_runs(row: bytes, K: int = 32) -> List[int]:
    """The row's window minimizers, one per run of consecutive windows that share it."""
    h = mers16(row)
    w = K - 15
    runs, prev = [], None
    for p in range(len(row) - K + 1):
        m = min(h[p:p + w])
        if m != prev:
            runs.append(m)
        prev = m
    return runs


def decision(rows, mc: int, K: int = 32) -> Verdict:
    """("emptied" | "kept", the largest run count of a row, the distinct minimizers, the
    largest count). Rows shorter than K have no window."""
    counts: Counter = Counter()
    max_runs = 0
    for r in rows:
        runs = row_runs(r, K)
        max_runs = max(max_runs, len(runs))
        counts.update(runs)
    distinct = len(counts)
    max_count = max(counts.values(), default=0)
    emptied = max_runs <= LIST_CAP and distinct <= CLAIM_CAP and max_count < mc
    return Verdict("emptied" if emptied else "kept", max_runs, distinct, max_count)


def capped_max_count(rows, K: int = 32) -> int:
    """The largest count if every row's list stopped silently at LIST_CAP runs."""
    c: Counter = Counter()
    for r in rows:
        c.update(row_runs(r, K)[:LIST_CAP])
    return max(c.values(), default=0)


def has_valid_kmer(rows, mc: int, K: int = 32) -> bool:
    c: Counter = Counter()
    for r in rows:
        for p in range(len(r) - K + 1):
            c[r[p:p + K]] += 1
    return max(c.values(), default=0) >= mc


def certified(row: bytes) -> bool:
    """True => the pack kernels set the repeat certificate for this row, whatever rows share
    its wave. Stricter than tests/test_kmer_cert.py norep: the kernels compare an aligned
    16-mer with later positions up to the longest row of the wave, which for a shorter row
    run into its zero (A) padding, and an aligned position past the row's end reads as a
    repeat when a later 16-mer is its bitwise complement (kmer_kernels.hip may_repeat16)."""
    if len(row) > 224 or any(c not in CODE for c in row):
        return False
    h = mers16(row + b"A" * (240 - len(row)))
    for a in range(0, 209, 16):
        want = h[a] if a + 16 <= len(row) else h[a] ^ 0xFFFFFFFF
        if want in h[a + 1:]:
            return False
    return True


def plan_batches(sizes: List[int]) -> List[List[int]]:
    """How one wave batches consecutive candidates of these row counts (indices into
    sizes): up to 8 groups and 64 rows, a group of more than 64 rows alone."""
    out, cur, rows = [], [], 0
    for i, n in enumerate(sizes):
        if cur and (len(cur) == BATCH_GROUPS or rows + n > BATCH_ROWS):
            out.append(cur)
            cur, rows = [], 0
        cur.append(i)
        rows += n
        if rows > BATCH_ROWS:
            out.append(cur)
            cur, rows = [], 0
    if cur:
        out.append(cur)
    return out


@dataclass
class Group:
    role: str                      # what the group is built for
    candidate: bool                # the filter must decide it (dbg != 0); else dbg == 0
    expect: Optional[str] = None   # candidates: "emptied" | "kept", as built
    valid: Optional[bool] = None   # built to have (True) / not to have (False) a valid K-mer
    gave_up: bool = False          # runs alone and passes the claim cap: dbg == 3 exactly


@dataclass
class Family:
    name: str
    mc: int
    offsets: np.ndarray            # int64, rows + 1
    values: np.ndarray             # uint8
    go: np.ndarray                 # int64, groups + 1
    groups: Dict[int, Group] = field(default_factory=dict)  # groups absent here: fillers, no candidates

    @property
    def n_groups(self) -> int:
        return len(self.go) - 1

    @property
    def max_len(self) -> int:
        return int(np.diff(self.offsets).max())

    @property
    def stride(self) -> int:
        """64-bit words per staged row: both staging paths take ceil(longest row / 32) of
        the column (PackedReads.max_len; kmer_spectrum_fused max_len = -1)."""
        return max(1, (self.max_len + 31) // 32)

    def rows_of(self, g: int) -> List[bytes]:
        o = self.offsets
        return [self.values[o[r]:o[r + 1]].tobytes() for r in range(int(self.go[g]), int(self.go[g + 1]))]

    def candidates(self) -> List[int]:
        return [g for g, i in sorted(self.groups.items()) if i.candidate]

    def capacity(self) -> int:
        return int(np.clip(np.diff(self.offsets) - 3, 0, None).sum())


def _family(name, mc, groups) -> Family:
    """groups: [(Group, [rows])] in order."""
    rows = [r for _, rs in groups for r in rs]
    lens = np.array([len(r) for r in rows], np.int64)
    go = np.concatenate([[0], np.cumsum([len(rs) for _, rs in groups])]).astype(np.int64)
    fam = Family(name, mc, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
                 np.frombuffer(b"".join(rows), np.uint8).copy(), go, {g: info for g, (info, _) in enumerate(groups)})
    _check_classes(fam)
    return fam


def _check_classes(fam: Family) -> None:
    """A candidate is a class-3 group: within the row and word limits at the column's stride,
    min_coverage rows with observations, every row certified."""
    for g, info in fam.groups.items():
        if not info.candidate:
            continue
        rows = fam.rows_of(g)
        assert len(rows) <= C3_ROWS and len(rows) * fam.stride <= C3_WORDS, (fam.name, g, len(rows), fam.stride)
        assert sum(len(r) >= 32 for r in rows) >= fam.mc, (fam.name, g)
        assert all(certified(r) for r in rows), (fam.name, g)


def _rand(rnd: random.Random, L: int, alphabet: bytes = b"ACGT") -> bytes:
    """A certified random row."""
    while True:
        r = bytes(rnd.choices(alphabet, k=L))
        if certified(r):
            return r


def _read(rnd, tpl: bytes, L: int, errs: int) -> bytes:
    while True:
        o = rnd.randint(0, len(tpl) - L)
        x = bytearray(tpl[o:o + L])
        for _ in range(errs):
            q = rnd.randrange(L)
            x[q] = rnd.choice([c for c in b"ACGT" if c != x[q]])
        if certified(bytes(x)):
            return bytes(x)


def _until(make, ok):
    for _ in range(100000):
        x = make()
        if ok(x):
            return x
    raise AssertionError("builder: no sample met its condition")


EMPTIED = dict(candidate=True, expect="emptied", valid=False)
KEPT_VALID = dict(candidate=True, expect="kept", valid=True)
LENGTHS = (31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 207, 208, 209, 223, 224)


def lengths(seed: int = 11) -> Family:
    """mc 2, two rows of one length at the half-word and word edges up to the 224-base
    limit; per length: identical rows, unrelated rows, rows that share only their first 32
    bases, rows that share only their last 32 (a T-rich tail: its 16-mers sort high, so the
    shared count hangs on the last windows next to the padding, which sorts below them).
    Rows of 31 bases have no window: those groups are no candidates."""
    rnd = random.Random(seed)
    groups = []
    for L in LENGTHS:
        cand = L >= 32
        kept = dict(candidate=True, expect="kept", valid=True) if cand else dict(candidate=False, valid=False)
        empt = EMPTIED if cand else dict(candidate=False, valid=False)
        a = _rand(rnd, L)
        groups.append((Group(f"len{L}:identical", **kept), [a, a]))
        groups.append((Group(f"len{L}:unrelated", **empt), [_rand(rnd, L), _rand(rnd, L)]))
        if cand:
            head = _rand(rnd, 32)
            rows = _until(lambda: [head + bytes(rnd.choices(b"ACGT", k=L - 32)) for _ in range(2)],
                          lambda rs: all(certified(r) for r in rs) and (L == 32 or rs[0][32] != rs[1][32]))
            groups.append((Group(f"len{L}:head32", **kept), rows))
            tail = _rand(rnd, 32, b"TTTTTTTCGA")
            rows = _until(lambda: [bytes(rnd.choices(b"ACGT", k=L - 32)) + tail for _ in range(2)],
                          lambda rs: all(certified(r) for r in rs) and (L == 32 or rs[0][-33] != rs[1][-33]))
            groups.append((Group(f"len{L}:tail32", **kept), rows))
        else:
            groups.append((Group(f"len{L}:head", candidate=False, valid=False), [_rand(rnd, L), _rand(rnd, L)]))
            groups.append((Group(f"len{L}:tail", candidate=False, valid=False), [_rand(rnd, L), _rand(rnd, L)]))
    return _family("lengths", 2, groups)


def list_cap(seed: int = 12) -> Family:
    """224-base rows around the 28-entry list. Group 0: two rows of more than 28 runs with
    unique prefixes and a shared 40-base tail whose windows lie past the 28th run: kept only
    by the kernel's keep bit (a list capped silently would count nothing twice). Group 1:
    the same shape, at most 28 runs, nothing shared: emptied. Group 2: nothing shared, the
    longest list exactly 28. Group 3: 29 runs in one row, nothing shared and nothing valid:
    kept by the row alone."""
    rnd = random.Random(seed)
    tail = _rand(rnd, 40)

    def over():  # > 28 runs, every shared window past the 28th run
        r = bytes(rnd.choices(b"ACGT", k=184)) + tail
        return r

    def over_ok(r):
        if not certified(r):
            return False
        return len(row_runs(r[:-9])) > LIST_CAP  # 29 runs or more in the windows before the shared 9

    a, b = _until(over, over_ok), _until(over, over_ok)
    plain = lambda: _until(lambda: _rand(rnd, 224), lambda r: len(row_runs(r)) <= LIST_CAP)
    exact = _until(lambda: _rand(rnd, 224), lambda r: len(row_runs(r)) == LIST_CAP)
    one_over = _until(lambda: _rand(rnd, 224), lambda r: len(row_runs(r)) == LIST_CAP + 1)
    return _family("list_cap", 2, [
        (Group("over the list cap, valid past it", **KEPT_VALID), [a, b]),
        (Group("control: within the cap, nothing shared", **EMPTIED), [plain(), plain()]),
        (Group("exactly 28 runs", **EMPTIED), [exact, plain()]),
        (Group("29 runs, nothing valid", candidate=True, expect="kept", valid=False), [one_over, plain()]),
    ])


def claim_cap(seed: int = 13) -> Family:
    """150-base rows (stride 5) around the 384-claim cap, mc 2.
    0: 70 unrelated rows (more than 64: a batch alone, two passes), > 384 distinct: gave up.
    1-3: a small kept group, 40 unrelated rows (> 384 distinct) and a small emptied group in
    one batch: the batch passes the cap and is redone group by group.
    4-5: about 27 unrelated rows with close to but at most 384 distinct minimizers (emptied) and
    32 copies of one row (kept) in one batch: more than 384 list entries, at most 384
    distinct keys, so the capped insert of the whole batch succeeds."""
    rnd = random.Random(seed)
    big70 = [_rand(rnd, 150) for _ in range(70)]
    tpl = _rand(rnd, 150)
    small_kept = [tpl, _rand(rnd, 150), tpl]
    big40 = [_rand(rnd, 150) for _ in range(40)]
    small_empt = [_rand(rnd, 150) for _ in range(3)]
    near = []  # rows added until the distinct minimizers are within 10 % below the cap, 20 left for the copies
    while decision(near, 2).distinct < CLAIM_CAP * 0.9:
        near.append(_rand(rnd, 150))
    assert decision(near, 2).distinct <= CLAIM_CAP - 20 and len(near) <= 32, len(near)
    one = _rand(rnd, 150)
    return _family("claim_cap", 2, [
        (Group("70 unrelated rows alone", candidate=True, expect="kept", valid=False, gave_up=True), big70),
        (Group("split: small kept", **KEPT_VALID), small_kept),
        (Group("split: 40 unrelated rows", candidate=True, expect="kept", valid=False), big40),
        (Group("split: small emptied", **EMPTIED), small_empt),
        (Group("near the claim cap", **EMPTIED), near),
        (Group("32 copies beside it", **KEPT_VALID), [one] * 32),
    ])


PASS_SIZES = (64, 65, 128, 129, 192)


def passes(seed: int = 14) -> Family:
    """Rows of 40-44 bases with at most 2 minimizer runs each, in a column of their own (stride
    2, so 192 rows are a class-3 group and stay within 384 distinct minimizers), mc 2.
    Per size 64, 65, 128, 129, 192: unrelated rows (emptied), and the same with one template
    in row 1 and in the last row, so the count reaches mc only across passes (kept, valid).
    Last: 192 rows of 3 runs each, which pass the claim cap in a later pass (gave up)."""
    rnd = random.Random(seed)
    short = lambda: _until(lambda: _rand(rnd, rnd.randint(40, 44)), lambda r: len(row_runs(r)) <= 2)
    groups = []
    for n in PASS_SIZES:
        groups.append((Group(f"{n} unrelated rows", **EMPTIED), [short() for _ in range(n)]))
        rows = [short() for _ in range(n)]
        rows[-1] = rows[1]
        groups.append((Group(f"{n} rows, a template in row 1 and the last", **KEPT_VALID), rows))
    three = lambda: _until(lambda: _rand(rnd, 44), lambda r: len(row_runs(r)) == 3)
    groups.append((Group("192 rows past the claim cap in a later pass", candidate=True, expect="kept", valid=False,
                         gave_up=True), [three() for _ in range(192)]))
    return _family("passes", 2, groups)


def batches(seed: int = 15) -> Family:
    """100-base rows and one of 224 (stride 7), mc 2, all in one 64-group chunk (one wave).
    0-8: nine two-row candidates: the 9th starts a new batch; one template read once in
    group 0 and once in group 7 (both emptied: the key carries the group); group 3 kept by
    its count, the 9th by a row past the list cap. Then candidates between groups that are none (a poly-A row: uncertified; a
    single row; 200 rows: too large for class 3), a 60-row group that fills a batch alone
    (and passes the claim cap there), and batches of exactly 64 rows (30 + 34) and of 30 alone because 30 + 35 = 65."""
    rnd = random.Random(seed)
    R = lambda: _rand(rnd, 100)
    tpl = R()
    groups = []
    for g in range(9):
        if g in (0, 7):
            info, rows = Group(f"template once (group {g})", **EMPTIED), [tpl, R()]
        elif g == 3:
            a = R()
            info, rows = Group("identical rows", **KEPT_VALID), [a, a]
        elif g == 8:  # kept by its 29-run row alone: were it a 9th group of the batch, no keep bit would hold it
            over = _until(lambda: _rand(rnd, 224), lambda r: len(row_runs(r)) == LIST_CAP + 1)
            info = Group("9th: a new batch; a 224-base row of 29 runs, nothing valid", candidate=True, expect="kept",
                         valid=False)
            rows = [over, R()]
        else:
            info, rows = Group("unrelated rows", **EMPTIED), [R(), R()]
        groups.append((info, rows))
    polya = b"A" * 60 + bytes(rnd.choices(b"CGT", k=40))
    groups.append((Group("poly-A row: uncertified", candidate=False, valid=True), [polya, R()]))
    groups.append((Group("unrelated rows", **EMPTIED), [R(), R()]))
    groups.append((Group("single row", candidate=False, valid=False), [R()]))
    a = R()
    groups.append((Group("identical rows", **KEPT_VALID), [a, a]))
    groups.append((Group("200 rows: past class 3", candidate=False, valid=False), [R() for _ in range(200)]))
    groups.append((Group("unrelated rows", **EMPTIED), [R(), R()]))
    groups.append((Group("60 unrelated rows: a batch alone, past the claim cap", candidate=True, expect="kept",
                         valid=False, gave_up=True), [R() for _ in range(60)]))
    groups.append((Group("30 rows (30 + 34 = 64)", **EMPTIED), [R() for _ in range(30)]))
    rows = [R() for _ in range(34)]
    rows[33] = rows[0]
    groups.append((Group("34 rows (30 + 34 = 64), a template twice", **KEPT_VALID), rows))
    groups.append((Group("30 rows (30 + 35 = 65: alone)", **EMPTIED), [R() for _ in range(30)]))
    groups.append((Group("35 rows (30 + 35 = 65: the next batch)", **EMPTIED), [R() for _ in range(35)]))
    return _family("batches", 2, groups)


CHUNK_WAVES = 2 * 4096           # waves of the filter's largest grid: a wave's chunks are this far apart
CHUNK_A = 3                      # the chunk (64 groups) whose last three groups are candidates
CHUNKS_G = 64 * CHUNK_WAVES + 64 * (CHUNK_A + 1) + 37


def chunks(seed: int = 16) -> Family:
    """One batch across two chunks of one wave. A wave takes a second 64-group chunk only
    past 64 * 2 * 4096 groups, so this family needs G = 524,581 groups: about half a million
    rows (21 MB); nothing smaller reaches the second chunk of a wave. Nearly every group is a
    single 40-base row: no candidate at mc 2, cheap for the oracle, never looked at by the
    model. The last three groups of chunk 3 and the first three of chunk 3 + 8192 (the same
    wave's next chunk) are two-row candidates of 64 bases, batched together: one has a valid
    K-mer (in the second chunk), and one template is read once in a group of each chunk."""
    rnd = random.Random(seed)
    rng = np.random.default_rng(seed)
    G = CHUNKS_G
    first = [64 * CHUNK_A + 61 + i for i in range(3)]
    second = [64 * (CHUNK_A + CHUNK_WAVES) + i for i in range(3)]
    R = lambda: _rand(rnd, 64)
    tpl, a = R(), R()
    special = {
        first[0]: (Group("chunk 3: template once", **EMPTIED), [tpl, R()]),
        first[1]: (Group("chunk 3: unrelated", **EMPTIED), [R(), R()]),
        first[2]: (Group("chunk 3: unrelated", **EMPTIED), [R(), R()]),
        second[0]: (Group("chunk 3 + 8192: template once", **EMPTIED), [R(), tpl]),
        second[1]: (Group("chunk 3 + 8192: identical rows", **KEPT_VALID), [a, a]),
        second[2]: (Group("chunk 3 + 8192: unrelated", **EMPTIED), [R(), R()]),
    }
    nrows = np.ones(G, np.int64)
    nrows[list(special)] = 2
    go = np.concatenate([[0], np.cumsum(nrows)]).astype(np.int64)
    n = int(go[-1])
    lens = np.full(n, 40, np.int64)
    for g in special:
        lens[go[g]:go[g + 1]] = 64
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    values = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=int(offsets[-1]))]
    for g, (_, rows) in special.items():
        for i, r in enumerate(rows):
            o = int(offsets[go[g] + i])
            values[o:o + 64] = np.frombuffer(r, np.uint8)
    fam = Family("chunks", 2, offsets, values, go, {g: info for g, (info, _) in special.items()})
    _check_classes(fam)
    return fam


def coverage(mc: int, seed: int = 17) -> Family:
    """150-base rows at min_coverage mc (3 and 20): mc copies of one read (kept); mc - 1
    copies (emptied by the row count before the filter: no candidate); mc - 1 copies plus an
    unrelated row (candidate, emptied); one template read mc times at shifted offsets with
    one error each (kept)."""
    rnd = random.Random(seed + mc)
    a, b, c = (_rand(rnd, 150) for _ in range(3))
    tpl = _rand(rnd, 200)
    shifted = _until(lambda: [_read(rnd, tpl, 150, 1) for _ in range(mc)],
                     lambda rs: decision(rs, mc).verdict == "kept" and has_valid_kmer(rs, mc))
    return _family(f"coverage{mc}", mc, [
        (Group("mc copies", **KEPT_VALID), [a] * mc),
        (Group("mc - 1 copies: the row count empties it", candidate=False, valid=False), [b] * (mc - 1)),
        (Group("mc - 1 copies and an unrelated row", **EMPTIED), [c] * (mc - 1) + [_rand(rnd, 150)]),
        (Group("a template mc times, shifted, one error each", **KEPT_VALID), shifted),
    ])


BUILDERS = {
    "lengths": lengths, "list_cap": list_cap, "claim_cap": claim_cap, "passes": passes, "batches": batches,
    "chunks": chunks, "coverage3": lambda: coverage(3), "coverage20": lambda: coverage(20),
}
_cache: Dict[str, Family] = {}
_refs: Dict[str, dict] = {}


def family(name: str) -> Family:
    """Built once per process; tests must not change it."""
    if name not in _cache:
        _cache[name] = BUILDERS[name]()
    return _cache[name]


def oracle_ref(name: str, k: int = 17) -> dict:
    """The CPU oracle's spectra of every group of a family (oracle/kmer_oracle.cpp), once
    per process. Through oracle.pyoracle.kmer_spectrum; for the half-million groups of
    `chunks` through the same C entry with buffers allocated once (kmer_spectrum's per-group
    arrays cost 17 s there; tests/test_mz_spec.py holds the two drivers together)."""
    key = f"{name}:{k}"
    if key not in _refs:
        fam = family(name)
        _refs[key] = (oracle_lean if fam.n_groups > 100_000 else oracle_full)(fam, k)
    return _refs[key]


def _col(fam: Family):
    from oracle import pyoracle as P

    return P.StrCol(fam.offsets, fam.values, None, len(fam.offsets) - 1)


def oracle_full(fam: Family, k: int = 17, g0: int = 0, g1: Optional[int] = None) -> dict:
    from oracle import pyoracle as P

    go = fam.go[g0:(fam.n_groups if g1 is None else g1) + 1]
    return P.kmer_spectrum(_col(fam), k, fam.mc, False, go, threads=1)


def oracle_lean(fam: Family, k: int = 17, g0: int = 0, g1: Optional[int] = None) -> dict:
    import ctypes

    from oracle import pyoracle as P

    L = P.lib()
    col = _col(fam)
    offs, vals, valid = col._ptrs()
    g1 = fam.n_groups if g1 is None else g1
    G = g1 - g0
    go = fam.go.tolist()
    cap = int(np.diff(fam.go).max()) * fam.max_len + 1
    km, ex, cn = np.zeros(2 * cap, np.uint64), np.zeros(cap, np.uint8), np.zeros(cap, np.uint16)
    stats = np.zeros((G, 5), np.int64)
    vp = ctypes.c_void_p
    pk, pe, pc, ps = vp(km.ctypes.data), vp(ex.ctypes.data), vp(cn.ctypes.data), stats.ctypes.data
    counts = np.zeros(G, np.int64)
    his, los, exs, cns = [], [], [], []
    fn, mc = L.oracle_kmer_spectrum, int(fam.mc)
    for i in range(G):
        m = fn(offs, 8, vals, valid, 0, go[g0 + i], go[g0 + i + 1], k, 0, mc, pk, pe, pc, cap, vp(ps + 40 * i))
        assert m >= 0
        if m:
            counts[i] = m
            his.append(km[0:2 * m:2].copy())
            los.append(km[1:2 * m:2].copy())
            exs.append(ex[:m].copy())
            cns.append(cn[:m].copy())
    out_off = np.zeros(G + 1, np.int64)
    out_off[1:] = np.cumsum(counts)
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    return {"kmer_hi": cat(his, np.uint64), "kmer_lo": cat(los, np.uint64), "exts": cat(exs, np.uint8),
            "counts": cat(cns, np.uint16), "group_offsets": out_off, "stats": stats}
