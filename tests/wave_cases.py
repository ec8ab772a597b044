"""Read groups that pin the wave-per-group k-mer kernel (k_kmer_wave, kmer_kernels.hip) at
its table, sort and row limits, built and checked without a GPU.

A case is one named group: byte rows (None = a null row) with k, min_coverage, what it is
meant to hit, the figures it must show and the size class it must start and end in. The
figures come from oracle.pyoracle.py_kmer_spectrum and the rows alone (figures); the classes
from a restatement of k_group_classify's choice (initial_class) and of the caps at which
each kernel hands a group on (final_class). A layout is a list of cases of one (k,
min_coverage) in the group order of one spectrum call.

tests/test_wave_cases.py asserts every case's figures and classes on the CPU;
tests/test_gpu_wave_classes.py compares the kernels' outputs with the oracle and the classes
rogtk_kmer_debug_classes reports with the predictions made here. Only numpy and the oracle
are needed.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

# ------------------------------------------------------------------------------- the caps
# Each constant restates one line of rogtk_amd/csrc/kmer_kernels.hip (quoted beside it).
WAVE_MAX_K = 16                  # "if (wave && K <= 16 && nrows <= kWaveRows && words <= kWaveWords) cls = 2;"
WAVE_ROWS = 64                   # "constexpr int kWaveRows = 64;       // one row per lane"
WAVE_WORDS = {2: 192, 6: 320}    # "static constexpr int kWords = SLOTS == 1024 ? 192 : 320;"
WAVE_CLAIM = {2: 832, 6: 1664}   # "static constexpr int kClaim = SLOTS * 13 / 16;"  (claims > kWaveClaim leaves;
#                                   the all-T 16-mer claims nothing: "(v == kWEmpty) & (allt == 0u)")
WAVE_VALID = {2: 512, 6: 1024}   # "static constexpr int kValid = SLOTS / 2;"  ("if (nv > (uint32_t)kWaveValid) over = true;")
WAVE_DEEP = 257                  # "deep |= li > 255u;": the 257th entry of one rank-sort bucket
WAVE_BUCKETS = 256               # "TK[i] >> bsh & 255u", "bsh = 2 * K - 8 >= 2 ? 2 * K - 8 : 2"
LDS_ORDER = (3, 1, 4)            # "gsmall[g] = CLS == 3 ? 1 : CLS == 1 ? 4 : 0;"
LDS_ROWS = {3: 192, 1: 256, 4: 512}      # "kRows = CLS == 3 ? 192 : CLS == 1 ? 256 : 512;"
LDS_WORDS = {3: 576, 1: 768, 4: 4096}    # "kWords = CLS == 3 ? 576 : CLS == 1 ? 768 : 4096;"
LDS_CLAIM = {3: 1472, 1: 2048, 4: 6144}  # "kClaim = CLS == 4 ? 6144 : CLS == 3 ? 1472 : kObs;"
LDS_OBS = {3: 1024, 1: 2048, 4: 2048}    # "kObs = CLS == 3 ? 1024 : 2048;"  ("if (nv > (uint32_t)kLdsObs)")
CHUNK = 64                       # "const int64_t n_chunks = (G + 63) >> 6;": groups a wave takes together

_ACGT = np.frombuffer(b"ACGT", np.uint8)


def effective_k(k: int) -> int:
    return 4 if k <= 4 else 8 if k <= 8 else 16 if k <= 16 else 32 if k <= 32 else 64


# ------------------------------------------------------------------------------- classes
def _usable(row, K: int) -> bool:
    """A row that yields observations: not null, ACGT in either case, at least K bases."""
    return row is not None and len(row) >= K and all(c in b"ACGTacgt" for c in row)


def group_shape(rows: Sequence[Optional[bytes]], K: int, stride: int = 0):
    """(rows, packed words, observations) as k_group_classify sees them. Ragged staging
    (stride 0): words = sum of ceil(len / 32) over the non-null rows (k_row_meta: "row_words[r]
    = valid ? (len + 31) >> 5 : 0"); fixed stride: "if (stride) words = nrows * stride"."""
    nrows = len(rows)
    words = nrows * stride if stride else sum((len(r) + 31) // 32 for r in rows if r is not None)
    obs = sum(len(r) - K + 1 for r in rows if _usable(r, K))
    return nrows, words, obs


def initial_class(nrows: int, words: int, obs: int, K: int, wave: bool = True) -> int:
    """k_group_classify's choice for a group of effective k K (the repeat certificate, K >=
    31 only, left aside). wave False: rogtk_kmer_set_path(2)."""
    if K > 32 or obs <= 0:
        return 0
    if wave and K <= WAVE_MAX_K and nrows <= WAVE_ROWS:
        for cls in (2, 6):
            if words <= WAVE_WORDS[cls]:
                return cls
    for cls in LDS_ORDER:
        if nrows <= LDS_ROWS[cls] and words <= LDS_WORDS[cls]:
            return cls
    return 0


def final_class(cls: int, words: int, distinct: int, distinct_not_allt: int, valid: int, top_bucket: int) -> int:
    """The class a group ends in: each kernel's caps in launch order (2, 6, 3, 1, 4)."""
    if cls == 2 and (distinct_not_allt > WAVE_CLAIM[2] or valid > WAVE_VALID[2] or top_bucket >= WAVE_DEEP):
        # "gsmall[g] = SLOTS == 1024 && nwords <= kWaveBigWords ? kClsWaveBig : 3;"
        cls = 6 if words <= WAVE_WORDS[6] else 3
    if cls == 6 and (distinct_not_allt > WAVE_CLAIM[6] or valid > WAVE_VALID[6] or top_bucket >= WAVE_DEEP):
        cls = 3
    for c, nxt in ((3, 1), (1, 4), (4, 0)):
        if cls == c and (distinct > LDS_CLAIM[c] or valid > LDS_OBS[c]):
            cls = nxt
    return cls


# ------------------------------------------------------------------------------- figures
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def kmer_key(s: str) -> int:
    v = 0
    for ch in s:
        v = v * 4 + _CODE[ch]
    return v


def bucket_of(key: int, K: int) -> int:
    return (key >> max(2 * K - 8, 2)) & (WAVE_BUCKETS - 1)


@functools.lru_cache(maxsize=None)
def _spectrum(rows: tuple, k: int, min_cov: int):
    from oracle.pyoracle import py_kmer_spectrum

    return py_kmer_spectrum(list(rows), k, min_cov)


def figures(rows: Sequence[Optional[bytes]], k: int, min_cov: int) -> dict:
    """distinct (k-mers at min_coverage 1), distinct_not_allt (without T x K at K = 16, the key
    that equals the table's empty mark), valid, top_bucket (the most valid k-mers in one
    bucket of the rank sort)."""
    K = effective_k(k)
    rows = tuple(rows)
    all_, _ = _spectrum(rows, k, 1)
    val, _ = _spectrum(rows, k, min_cov)
    allt = "T" * 16
    n_allt = sum(1 for km, _, _ in all_ if K == 16 and km == allt)
    buckets = np.bincount([bucket_of(kmer_key(km), K) for km, _, _ in val], minlength=256)
    return {"distinct": len(all_), "distinct_not_allt": len(all_) - n_allt, "valid": len(val),
            "top_bucket": int(buckets.max()), "allt_count": next((c for km, _, c in all_ if K == 16 and km == allt), 0)}


def segments(rows: Sequence[Optional[bytes]], K: int) -> dict:
    """k_kmer_wave's lane tasks for a group of at most 64 rows: spr segments per row of Ls
    positions, nst[lane] positions of each lane's segment, L0 trips of the uniform loop."""
    nobs = [len(r) - K + 1 if _usable(r, K) else 0 for r in rows]
    nrows = len(rows)
    assert 1 <= nrows <= WAVE_ROWS
    spr = max(1, 64 // nrows)
    Ls = (max(nobs) + spr - 1) // spr
    nst = [min(max(nobs[lane // spr] - (lane % spr) * Ls, 0), Ls) for lane in range(64) if lane // spr < nrows]
    L0 = min(min(nst), Ls) & ~1
    return {"spr": spr, "Ls": Ls, "L0": L0, "nst": nst, "nobs": nobs}


def claim_trip(rows: Sequence[Optional[bytes]], K: int, cap: int):
    """The trip t after which the wave kernel sees more than `cap` claimed keys (None: never),
    replaying its insert order: lane (row r, segment) starts at rotation (7 r) % nst of its
    segment and wraps; the count is tested after every second trip and after the last one."""
    sg = segments(rows, K)
    spr, Ls = sg["spr"], sg["Ls"]
    up = [r.upper().decode() if _usable(r, K) else "" for r in rows]
    seen, allt = set(), "T" * 16
    for t in range(Ls):
        for lane, nst in enumerate(sg["nst"]):
            if t < nst:
                r = lane // spr
                p = (lane % spr) * Ls + ((7 * r) % nst + t) % nst
                km = up[r][p:p + K]
                if not (K == 16 and km == allt):
                    seen.add(km)
        if (t % 2 == 1 or t == Ls - 1) and len(seen) > cap:
            return t
    return None


# --------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    name: str
    rows: tuple            # bytes or None per row
    k: int
    min_cov: int
    hits: str              # what the group is meant to reach
    expect: dict           # figure -> exact value or (lo, hi) inclusive
    init: int              # the class it must start in (ragged staging)
    final: int             # the class it must end in (0 = the global path)
    extra: dict = field(default_factory=dict, compare=False, hash=False)

    @property
    def K(self) -> int:
        return effective_k(self.k)

    def figures(self) -> dict:
        return figures(self.rows, self.k, self.min_cov)

    def predict(self, stride: int = 0, wave: bool = True):
        """(initial, final) class for ragged (stride 0) or fixed-stride staging."""
        nrows, words, obs = group_shape(self.rows, self.K, stride)
        f = self.figures()
        init = initial_class(nrows, words, obs, self.K, wave)
        return init, final_class(init, words, f["distinct"], f["distinct_not_allt"], f["valid"], f["top_bucket"])


def rand_rows(seed, n: int, L: int) -> list:
    rng = np.random.default_rng(seed)
    return [_ACGT[rng.integers(0, 4, L)].tobytes() for _ in range(n)]


def fragments(seed, n: int, lens, tpl_len: int = 200) -> list:
    """n overlapping fragments of one random template (few distinct k-mers, real coverage);
    lens: one length for all rows, or a sequence cycled over the rows."""
    rng = np.random.default_rng(seed)
    tpl = _ACGT[rng.integers(0, 4, tpl_len)].tobytes()
    lens = [lens] * n if isinstance(lens, int) else [lens[i % len(lens)] for i in range(n)]
    return [tpl[a:a + L] for L, a in ((L, int(rng.integers(0, tpl_len - L + 1))) for L in lens)]


def _deep_rows(seed, n: int, L: int, a_run: int = 13) -> list:
    """Rows of blocks A x a_run + 4 random bases of CGT: most 16-mers start with AAAA."""
    rng = np.random.default_rng(seed)
    cgt = np.frombuffer(b"CGT", np.uint8)
    out = []
    for _ in range(n):
        s = b""
        while len(s) < L:
            s += b"A" * a_run + cgt[rng.integers(0, 3, 4)].tobytes()
        out.append(s[:L])
    return out


def de_bruijn4(n: int) -> bytes:
    """The de Bruijn sequence B(4, n) over ACGT, its first n - 1 bases appended (every n-mer
    occurs exactly once as a window)."""
    a = [0] * (4 * n)
    seq = []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, 4):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    s = _ACGT[np.array(seq, np.int64)].tobytes()
    return s + s[:n - 1]


_T16 = b"T" * 16
PLAIN = tuple(fragments(101, 6, 100))  # the "plain group" of the state-carrying layout


def _claim_cases():
    base = rand_rows(7, 8, 119)
    c = [Case("claim_832_stays", tuple(base + [base[0]] * 3), 16, 2,
              "832 claimed keys, the most class 2 takes (checked in the tail loop)",
              {"distinct": 832, "valid": 104}, 2, 2),
         Case("claim_833_leaves", tuple(base[:7] + rand_rows(8, 1, 120) + [base[0]] * 3), 16, 2,
              "833 claimed keys: the 833rd in the checked tail loop", {"distinct": 833, "valid": 104}, 2, 6,
              {"claim_loop": "tail"})]
    big = rand_rows(9, 16, 119)
    c += [Case("claim_1664_stays_in_6", tuple(big + [big[0]] * 3), 16, 2,
               "1664 claimed keys, the most class 6 takes", {"distinct": 1664, "valid": 104}, 2, 6),
          # 1665 distinct k-mers are also past class 3's 1472 claims: class 1 keeps the group
          Case("claim_1665_leaves_6", tuple(big[:15] + rand_rows(10, 1, 120) + [big[0]] * 3), 16, 2,
               "1665 claimed keys: past class 6 (and class 3's 1472)", {"distinct": 1665, "valid": 104}, 2, 1)]
    # 52 / 53 rows of 31 bases: one segment per row of Ls = 16 = L0 trips, all in the uniform loop
    short = rand_rows(11, 53, 31)
    c += [Case("claim_832_uniform_stays", tuple(short[:52] + [short[0]]), 16, 2,
               "832 claimed keys with every trip in the uniform loop (L0 == Ls)",
               {"distinct": 832, "valid": 16}, 2, 2, {"L0_eq_Ls": True}),
          # the 53rd row: the first row moved on by one base, 15 known 16-mers and a new one
          Case("claim_833_uniform_leaves", tuple(short[:52] + [short[0][1:] + short[52][:1]]), 16, 2,
               "833 claimed keys: the 833rd in the uniform loop", {"distinct": 833, "valid": 15}, 2, 6,
               {"claim_loop": "uniform", "L0_eq_Ls": True}),
          Case("claim_mid_uniform", tuple(rand_rows(12, 16, 150)), 16, 2,
               "2160 distinct k-mers in rows of one length: class 2 bails in the middle of its uniform loop",
               {"distinct": 2160, "valid": 0}, 2, 4, {"claim_loop": "uniform", "mid": True}),
          Case("claim_mid_tail", tuple(rand_rows(13, 1, 160) + rand_rows(14, 30, 40)), 16, 1,
               "one long row and 30 short ones (L0 = 0 << Ls): class 2 bails in the checked tail loop",
               {"distinct": 895, "valid": 895}, 2, 6, {"claim_loop": "tail", "mid": True, "L0": 0})]
    return c


def _valid_cases():
    r4, r8 = rand_rows(21, 4, 143), rand_rows(22, 8, 143)
    t_row = [b"T" * 16]
    return [
        Case("valid_512_stays", tuple(r4), 16, 1, "512 valid k-mers, the most class 2 takes",
             {"distinct": 512, "valid": 512}, 2, 2),
        Case("valid_513_leaves", tuple(r4[:3] + rand_rows(23, 1, 144)), 16, 1, "513 valid k-mers",
             {"distinct": 513, "valid": 513}, 2, 6),
        Case("valid_1024_stays_in_6", tuple(r8), 16, 1, "1024 valid k-mers, the most class 6 takes",
             {"distinct": 1024, "valid": 1024}, 2, 6),
        # 1025 valid k-mers are also past class 3's sort buffer (1024): class 1 keeps the group
        Case("valid_1025_leaves_6", tuple(r8[:7] + rand_rows(24, 1, 144)), 16, 1, "1025 valid k-mers",
             {"distinct": 1025, "valid": 1025}, 2, 1),
        Case("valid_511_plus_allt_stays", tuple(r4[:3] + [r4[3][:142]] + t_row), 16, 1,
             "the all-T 16-mer is the 512th valid entry (written at nv = 511)",
             {"distinct": 512, "distinct_not_allt": 511, "valid": 512}, 2, 2),
        Case("valid_512_plus_allt_leaves", tuple(r4 + t_row), 16, 1,
             "the all-T 16-mer is the 513th valid entry (not written; nv counts it)",
             {"distinct": 513, "distinct_not_allt": 512, "valid": 513}, 2, 6),
        Case("valid_mc2_leaves", tuple(rand_rows(25, 4, 145) * 2), 16, 2,
             "520 valid k-mers at min_coverage 2 (every row twice)", {"distinct": 520, "valid": 520}, 2, 6)]


# (seed, rows, bases, A-run, bases cut from the last row): found by search, pinned by the CPU test
_DEEP = {"deep_257_leaves": (1, 4, 150, 12, 0), "deep_256_stays": (1, 4, 150, 12, 1),
         "deep_289_leaves": (0, 4, 160, 13, 0), "deep_mid_stays": (0, 2, 160, 13, 0)}


def _deep_group(name):
    seed, n, L, a_run, cut = _DEEP[name]
    rows = _deep_rows(seed, n, L, a_run)
    rows[-1] = rows[-1][:L - cut]
    return rows


def _deep_cases():
    return [
        # class 2 -> 6 -> 3 by `deep` alone: both wave instances bail, class 3 (a bitonic sort) keeps it
        Case("deep_257_leaves", tuple(_deep_group("deep_257_leaves")), 16, 1,
             "a rank-sort bucket past 256 entries (`deep`), within the claim and valid caps",
             {"distinct": 447, "valid": 447, "top_bucket": 257}, 2, 3),
        Case("deep_256_stays", tuple(_deep_group("deep_256_stays")), 16, 1,
             "a rank-sort bucket of exactly 256 entries, the most it takes (the same rows, one base shorter)",
             {"distinct": 446, "valid": 446, "top_bucket": 256}, 2, 2),
        Case("deep_289_leaves", tuple(_deep_group("deep_289_leaves")), 16, 1,
             "a bucket well past 256 entries (the entries past 255 all record place 255)",
             {"distinct": 459, "valid": 459, "top_bucket": 289}, 2, 3),
        Case("deep_mid_stays", tuple(_deep_group("deep_mid_stays")), 16, 1,
             "a bucket of 5..255 entries: the rank and neighbour loops past the 4-entry fast path",
             {"distinct": 254, "valid": 254, "top_bucket": 156}, 2, 2),
        Case("deep_mc2_leaves", tuple(_deep_group("deep_289_leaves") * 2), 16, 2,
             "the deep bucket at min_coverage 2 (every row twice)",
             {"distinct": 459, "valid": 459, "top_bucket": 289}, 2, 3)]


def _k8_k4_cases():
    sfx = [_ACGT[[(i >> 6) & 3, (i >> 4) & 3, (i >> 2) & 3, i & 3]].tobytes() for i in range(256)]
    rng = np.random.default_rng(31)
    arr = []
    # two arrangements of the 256 targets ACGT????, 17 to a row of 153 bases, each followed by a
    # spacer base (C in one arrangement, G in the other): a target is seen twice, and every
    # other 8-mer holds a spacer, so it is seen once unless two of them collide
    for spacer in (b"C", b"G"):
        order = rng.permutation(256)
        arr += [b"".join(b"ACGT" + sfx[j] + spacer for j in order[17 * r:17 * r + 17]) for r in range(16)]
    # the largest one-bucket load a group can finish with in a wave instance at effective k 8
    # (see full_bucket_k8 below): 40 rows of 4 targets and 24 rows of one
    order = rng.permutation(256)
    fit = [b"".join(b"ACGT" + sfx[j] for j in order[4 * r:4 * r + 4]) for r in range(40)]
    fit += [b"ACGT" + sfx[j] for j in order[160:184]]
    db = de_bruijn4(4)
    four = [_ACGT[[(i >> 6) & 3, (i >> 4) & 3, (i >> 2) & 3, i & 3]].tobytes() for i in range(0, 256, 5)]
    return [
        # All 256 8-mers ACGT???? valid at min_coverage 2. Every target brings the 8 k-mers of its
        # junction, so the group has 2,706 distinct k-mers and fails the claim caps of classes 2,
        # 6, 3 and 1; class 4 finishes it. No group of <= 64 rows holds all 256 within a wave
        # instance's caps: a target costs >= 4.5 distinct k-mers in rows of two or more targets
        # (64 rows of one target give 64), and the junction k-mers ?ACGT???, ??ACGT??, ???ACGT?
        # are shared by 4 targets each, so about as many of them are valid as targets are (757
        # valid here, not <= 512). big_bucket_k8_in_6 is the fullest bucket a wave instance
        # finishes at effective k 8
        Case("full_bucket_k8", tuple(arr), 8, 2, "256 valid 8-mers in one bucket, the most effective k 8 allows",
             {"valid": 757, "top_bucket": 256, "distinct": 2706}, 2, 4),
        Case("big_bucket_k8_in_6", tuple(fit), 8, 1, "184 valid 8-mers in one bucket, finished by class 6",
             {"valid": 950, "top_bucket": 184, "distinct": 950}, 2, 6),
        Case("all_4mers", (db[:160], db[157:]), 4, 1, "all 256 4-mers valid: 64 buckets of 4 (bsh clamped to 2)",
             {"distinct": 256, "valid": 256, "top_bucket": 4}, 2, 2),
        Case("rows_of_4_bases", tuple(four + [b"TTTT"] * 3 + [b"ACG", b"", None]), 4, 1,
             "rows of exactly 4 bases: one observation per row",
             {"distinct": 52, "valid": 52, "top_bucket": (1, 4)}, 2, 2),
        Case("t8_at_k8", (b"T" * 8, b"GT" + b"T" * 8 + b"A", b"ACGTTTTTTTT"), 8, 1,
             "T x 8 at effective k 8: its key is not the empty mark", {"valid": (5, 12), "allt_count": 0}, 2, 2)]


def _allt_cases():
    fl = rand_rows(41, 4, 40)
    mid = fl[0] + b"A" + _T16 + b"A" + fl[1]
    dup = fl[2]
    return [
        Case("allt_only", (_T16,), 16, 1, "the only k-mer is T x 16 (nv = 1, table untouched)",
             {"distinct": 1, "distinct_not_allt": 0, "valid": 1, "allt_count": 1}, 2, 2),
        Case("allt_run", (b"T" * 40, b"t" * 17), 16, 1, "T x 16 counted 27 times, its own left and right neighbour",
             {"distinct": 1, "distinct_not_allt": 0, "valid": 1, "allt_count": 27}, 2, 2),
        Case("allt_neighbours_valid", (mid, dup), 16, 1, "T x 16 valid between AT...T and T...TA, both valid",
             {"distinct_not_allt": 107, "valid": 108, "allt_count": 1}, 2, 2),
        Case("allt_neighbours_invalid", (mid, b"C" + _T16 + b"G", dup, dup), 16, 2,
             "T x 16 valid (seen twice), its neighbours seen once", {"valid": 26, "allt_count": 2}, 2, 2),
        Case("allt_below_min_cov", (mid, dup, dup), 16, 2, "T x 16 seen once at min_coverage 2",
             {"valid": 25, "allt_count": 1}, 2, 2)]


def _state_cases():
    fl = rand_rows(51, 3, 60)
    t3 = [fl[0] + b"G" + _T16 + b"C", b"A" + _T16, _T16 + b"G" + fl[1][:20], fl[0]]
    t1 = [fl[2] + b"C" + _T16 + b"A" + fl[1], fl[2], fl[1]]
    return [
        Case("state_allt_3", tuple(t3), 16, 2, "T x 16 seen 3 times", {"allt_count": 3, "valid": (46, 60)}, 2, 2),
        Case("state_allt_1", tuple(t1), 16, 2, "T x 16 seen once at min_coverage 2: not valid unless a count leaks in",
             {"allt_count": 1, "valid": 90}, 2, 2),
        Case("plain", PLAIN, 16, 2, "a plain group: its outputs must not depend on what its wave ran before",
             {"distinct": (86, 400), "valid": (40, 400)}, 2, 2)]


def _limit_cases():
    f = fragments
    return [
        Case("rows_64_stays_wave", tuple(f(61, 64, 60)), 16, 2, "64 rows, one per lane", {}, 2, 2),
        Case("rows_65_class_3", tuple(f(62, 65, 60)), 16, 2, "65 rows: no wave class", {}, 3, 3),
        Case("words_192_class_2", tuple(f(63, 48, 128)), 16, 2, "48 rows of 4 words: 192 packed words", {}, 2, 2,
             {"words": 192}),
        Case("words_193_class_6", tuple(f(64, 47, 128) + f(65, 1, 129)), 16, 2, "193 packed words", {}, 6, 6,
             {"words": 193}),
        Case("words_320_class_6", tuple(f(66, 64, 160)), 16, 2, "64 rows of 5 words: 320 packed words", {}, 6, 6,
             {"words": 320}),
        Case("words_321_class_3", tuple(f(67, 63, 160) + f(68, 1, 161)), 16, 2, "321 packed words in 64 rows", {}, 3, 3,
             {"words": 321}),
        Case("chain_from_6", tuple(rand_rows(69, 64, 160)), 16, 1,
             "9,280 distinct k-mers in 320 words: fails classes 6, 3, 1 and 4", {"distinct": 9280, "valid": 9280}, 6, 0,
             {"words": 320}),
        Case("chain_from_2", tuple(rand_rows(70, 64, 96)), 16, 1,
             "5,184 distinct and valid k-mers in 192 words: fails classes 2, 6, 3, 1 and 4 (its valid cap)",
             {"distinct": 5184, "valid": 5184}, 2, 0, {"words": 192})]


SHAPE_ROWS = (1, 2, 3, 21, 22, 32, 33, 63, 64)


def _shape_cases():
    out = []
    for R in SHAPE_ROWS:
        rng = np.random.default_rng(200 + R)
        tpl = _ACGT[rng.integers(0, 4, 220)].tobytes()

        def frag(L, rng=rng, tpl=tpl):
            a = int(rng.integers(0, 40))
            return tpl[a:a + L]

        # (a) very unequal rows: 16 and 160 bases, so late segments are empty (nst 0 or 1)
        a = [frag(160 if i % 5 == 0 else 16) for i in range(R)]
        # (b) lengths 32..160 in turn, the word-multiple lengths as last row too; odd rows out
        lens = (32, 64, 96, 128, 160, 47, 100, 131)
        b = [frag(lens[(i + R) % len(lens)]) for i in range(R)]
        b[-1] = frag((32, 64, 96, 128, 160)[SHAPE_ROWS.index(R) % 5])
        # (c) rows that yield nothing among rows that do
        odd = [frag(15), frag(16), b"", None, frag(50)[:20] + b"N" + frag(50)[:20], frag(90).lower(), frag(7)]
        c = [odd[i % len(odd)] if i % 3 == 1 else frag(70 + (i % 4)) for i in range(R)]
        for tag, rows in (("unequal", a), ("lengths", b), ("odd_rows", c)):
            out.append(Case(f"shape_{R}_{tag}", tuple(rows), 16, 2, f"{R} rows, {tag}", {}, 0, 0, {"shape": True}))
    return out


@functools.lru_cache(maxsize=None)
def all_cases() -> dict:
    cases = (_claim_cases() + _valid_cases() + _deep_cases() + _k8_k4_cases() + _allt_cases() + _state_cases()
             + _limit_cases())
    for c in _shape_cases():  # their classes follow from the shapes: taken from the restatement, wave expected
        init, final = c.predict()
        cases.append(Case(c.name, c.rows, c.k, c.min_cov, c.hits, c.expect, init, final, c.extra))
    by = {c.name: c for c in cases}
    assert len(by) == len(cases)
    return by


# ------------------------------------------------------------------------------- layouts
EMPTY = Case("empty", (), 16, 1, "a group without rows", {}, 0, 0)


def _with(c: Case, k: int, min_cov: int) -> Case:
    """The same rows under another call's k and min_coverage (classes predicted again)."""
    d = Case(c.name, c.rows, k, min_cov, c.hits, {}, 0, 0, c.extra)
    init, final = d.predict()
    return Case(c.name, c.rows, k, min_cov, c.hits, {}, init, final, c.extra)


def layout_state() -> list:
    """Consecutive groups of one 64-group chunk (one wave runs them in this order), all class
    2 at the start, min_coverage 2; then empty groups to the chunk's end and the plain group
    alone in a chunk of its own."""
    by = all_cases()
    order = ["state_allt_3", "state_allt_1", "claim_mid_uniform", "plain", "valid_mc2_leaves", "plain",
             "deep_mc2_leaves", "plain"]
    groups = [by[n] for n in order]
    return groups + [_with(EMPTY, 16, 2)] * (CHUNK - len(groups)) + [by["plain"]]


def layout_pipeline() -> list:
    """Chunks that hold exactly 1, 2 and 3 class-2 groups among groups of classes 6, 3, 0 and
    empty ones, a chunk of 64 class-2 groups, and a last chunk of 5 groups (min_coverage 2)."""
    by = all_cases()
    c6, c3 = by["words_193_class_6"], by["rows_65_class_3"]
    c0 = Case("rows_513_global", tuple(fragments(71, 513, 20, 60)), 16, 2, "513 rows: no LDS class", {}, 0, 0)
    e = _with(EMPTY, 16, 2)
    small = [by["plain"], by["allt_below_min_cov"], by["state_allt_3"], by["shape_3_lengths"], by["shape_2_unequal"]]
    out = []
    for n2 in (1, 2, 3):
        chunk = [e] * CHUNK
        chunk[0], chunk[1], chunk[5], chunk[62] = c6, c3, c0 if n2 == 1 else c3, c6
        for j, at in enumerate((63, 2, 31)[:n2]):  # the chunk's last group, an early one, a middle one
            chunk[at] = small[j]
        out += chunk
    out += [small[i % len(small)] for i in range(CHUNK)]
    out += [small[0], c6, small[1], e, small[2]]
    return out


def general_layouts() -> dict:
    """Every case outside the two ordered layouts, one call per (k, min_coverage)."""
    calls = {}
    for c in all_cases().values():
        calls.setdefault((c.k, c.min_cov), []).append(c)
    return calls


# the cases that also run through fixed-stride staging (effective k 16): the limits of claim,
# valid and deep, the all-T cases; the row and word limits are built for the stride (below)
STRIDE_CASES = ("claim_832_stays", "claim_833_leaves", "claim_1664_stays_in_6", "claim_1665_leaves_6",
                "claim_832_uniform_stays", "claim_833_uniform_leaves", "valid_512_stays", "valid_513_leaves",
                "valid_1024_stays_in_6", "valid_1025_leaves_6", "valid_511_plus_allt_stays",
                "valid_512_plus_allt_leaves", "deep_257_leaves", "deep_256_stays", "deep_289_leaves", "deep_mid_stays", "allt_only",
                "allt_run", "allt_neighbours_valid", "allt_neighbours_invalid", "allt_below_min_cov")


def stride_limit_cases() -> list:
    """Row and word limits at stride 5 (rows of 150 bases): 38 rows = 190 words stay in class
    2, 39 = 195 take class 6, 64 = 320 stay there, 65 rows take class 3. init / final here are
    the fixed-stride classes (Case.predict(5))."""
    out = []
    for R, init in ((38, 2), (39, 6), (64, 6), (65, 3)):
        out.append(Case(f"stride_rows_{R}", tuple(fragments(80 + R, R, 150)), 16, 2, f"{R} rows of 5 words", {},
                        init, init))
    return out


def layouts_fixed_stride() -> dict:
    """Calls for the fixed-stride entry points, per (k, min_coverage): every row has at most
    160 bases and each call holds one of more than 128, so staging uses stride 5."""
    by = all_cases()
    calls = {}
    for n in STRIDE_CASES:
        calls.setdefault((by[n].k, by[n].min_cov), []).append(by[n])
    calls[(16, 2)] = calls[(16, 2)] + stride_limit_cases() + layout_state()
    return calls


def flatten(groups: Sequence[Case]):
    """(items, group_offsets) of one call."""
    items, go = [], [0]
    for c in groups:
        items += list(c.rows)
        go.append(len(items))
    return items, go
