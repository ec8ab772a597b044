"""Cell-barcode correction against a whitelist on the GPU (rogtk_amd/csrc/barcode.hip, DESIGN.md
§4e) against restatement (a) of tests/barcode_spec.py: exact equality of index, status,
corrected, both count arrays and the totals.

Shapes are small and sit where the kernels can break: barcode lengths at both ends and at the
32-bit code boundary, prefix tables with P = L and P < L and with empty buckets, row counts
around the wave and the pack tile, miss lists that are empty or hold every row, and both probe
kernels on a crowded whitelist."""
from __future__ import annotations

import numpy as np
import pyarrow as pa
import pytest

import barcode_spec as B

pytestmark = pytest.mark.gpu

BASES = b"ACGT"


@pytest.fixture(scope="module")
def rg():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import rogtk_amd

    assert rogtk_amd.device_count() >= 1
    return rogtk_amd


def _bin(items):
    return pa.array(items, type=pa.large_binary())


def _same(got, want):
    assert got.keys.tolist() == want.index
    assert got.status.tolist() == want.status
    assert got.index.type == pa.uint32()
    assert got.index.to_pylist() == [w if s <= 1 else None for w, s in zip(want.index, want.status)]
    assert [None if x is None else bytes(x, "ascii") if isinstance(x, str) else x
            for x in got.corrected.to_pylist()] == want.corrected
    assert got.exact_counts.dtype == np.uint32 and got.exact_counts.tolist() == want.exact_counts
    assert got.counts.dtype == np.uint32 and got.counts.tolist() == want.counts
    assert list(got.totals) == ["exact", "corrected", "ambiguous", "no_match", "null"]
    assert list(got.totals.values()) == want.totals


def _check(wl, rows, whitelist, ambiguous="counts", counts=None):
    """One eager call on the handle `wl` of `whitelist` against restatement (a)."""
    want = B.correct_dict(rows, whitelist, ambiguous, counts)
    _same(wl.correct(_bin(rows), ambiguous, None if counts is None else np.asarray(counts, dtype=np.uint32)), want)
    return want


def _random_whitelist(rng, L, W):
    seen = {}
    while len(seen) < W:
        seen[bytes(BASES[int(x)] for x in rng.integers(0, 4, size=L))] = None
    return list(seen)


def _mutate(rng, s, j=None):
    j = int(rng.integers(0, len(s))) if j is None else j
    return s[:j] + bytes([BASES[(BASES.index(s[j]) + int(rng.integers(1, 4))) & 3]]) + s[j + 1:]


def _rows(rng, whitelist, n, p_exact=0.6):
    """n rows: exact entries, one substitution, one or two N / lower case, other lengths, random, nulls."""
    L = len(whitelist[0])
    out = []
    for _ in range(n):
        s = whitelist[int(rng.integers(0, len(whitelist)))]
        r = rng.random()
        if r < p_exact:
            pass
        elif r < p_exact + 0.2:
            s = _mutate(rng, s)
        elif r < p_exact + 0.28:
            for _ in range(int(rng.integers(1, 3))):
                j = int(rng.integers(0, L))
                s = s[:j] + (b"N" if rng.integers(0, 2) else s[j:j + 1].lower()) + s[j + 1:]
        elif r < p_exact + 0.32:
            s = s[:-1] if rng.integers(0, 2) else s + b"A"
        elif r < p_exact + 0.37:
            s = bytes(BASES[int(x)] for x in rng.integers(0, 4, size=L))
        elif r < p_exact + 0.39:
            s = None
        out.append(s)
    return out


# ------------------------------------------------------------ the known answer
@pytest.mark.parametrize("mode", list(B.KNOWN))
def test_known_answer_eager(rg, mode):
    ambiguous, caller = mode
    counts = B.KNOWN_CALLER_COUNTS if caller else None
    want = B.correct_dict(B.KNOWN_ROWS, B.KNOWN_WHITELIST, ambiguous, counts)
    assert (want.index, want.status, want.totals, want.counts) == B.KNOWN[mode]
    res = rg.barcode_correct(_bin(B.KNOWN_ROWS), _bin(B.KNOWN_WHITELIST), ambiguous,
                             None if counts is None else np.asarray(counts, dtype=np.uint32))
    _same(res, want)
    corrected = rg.col(_bin(B.KNOWN_ROWS)).barcode.correct(B.KNOWN_WHITELIST, ambiguous, counts)
    assert corrected.to_pylist() == want.corrected


@pytest.mark.parametrize("typ", [pa.string(), pa.large_string(), pa.binary()])
@pytest.mark.parametrize("n_chunks", [1, 3])
def test_known_answer_host_chunks_and_offset_widths(rg, n_chunks, typ):
    text = pa.types.is_string(typ) or pa.types.is_large_string(typ)
    # (acgt, lower case, is valid UTF-8; every known row is)
    items = [x.decode() if text and x is not None else x for x in B.KNOWN_ROWS]
    cuts = np.linspace(0, len(items), n_chunks + 1).astype(int)
    col = pa.chunked_array([pa.array(items[a:b], type=typ) for a, b in zip(cuts[:-1], cuts[1:])])
    wl = rg.BarcodeWhitelist(pa.array([w.decode() for w in B.KNOWN_WHITELIST], type=typ) if text
                             else pa.array(B.KNOWN_WHITELIST, type=typ))
    assert wl.info()["W"] == 7 and wl.info()["L"] == 4 and len(wl) == 7
    for ambiguous in ("counts", "reject"):
        _same(wl.correct(col, ambiguous), B.correct_dict(B.KNOWN_ROWS, B.KNOWN_WHITELIST, ambiguous))


def _device_column(items):
    import torch

    dense = [u if u is not None else b"" for u in items]
    off = torch.tensor(np.concatenate([[0], np.cumsum([len(u) for u in dense])]), dtype=torch.int64).cuda()
    val = torch.tensor(np.frombuffer(b"".join(dense) or b"\0", np.uint8).copy()).cuda()
    vbits = torch.from_numpy(np.packbits(np.array([u is not None for u in items] + [False] * 7),
                                         bitorder="little")).cuda()
    return off, val, vbits


@pytest.mark.parametrize("mode", list(B.KNOWN))
def test_known_answer_device_entry(rg, mode):
    import torch

    ambiguous, caller = mode
    counts = B.KNOWN_CALLER_COUNTS if caller else None
    want = B.correct_dict(B.KNOWN_ROWS, B.KNOWN_WHITELIST, ambiguous, counts)
    wl = rg.BarcodeWhitelist(B.KNOWN_WHITELIST)
    off, val, vbits = _device_column(B.KNOWN_ROWS)
    prior = None if counts is None else torch.tensor(counts, dtype=torch.int32).cuda()
    index, status, exact, final, totals = wl.correct_device(off, val, vbits, ambiguous, prior)
    assert index.cpu().numpy().view(np.uint32).tolist() == want.index
    assert status.cpu().numpy().tolist() == want.status
    assert exact.cpu().numpy().view(np.uint32).tolist() == want.exact_counts
    assert final.cpu().numpy().view(np.uint32).tolist() == want.counts
    assert list(totals.values()) == want.totals


@pytest.mark.parametrize("n_chunks", [1, 3])
def test_known_answer_plugin(rg, n_chunks):
    from rogtk_amd import plugin

    strs = [None if x is None else x.decode() for x in B.KNOWN_ROWS]
    cuts = np.linspace(0, len(strs), n_chunks + 1).astype(int)
    col = pa.chunked_array([pa.array(strs[a:b], type=pa.string()) for a, b in zip(cuts[:-1], cuts[1:])])
    wl = pa.chunked_array([pa.array([w.decode() for w in B.KNOWN_WHITELIST[:3]]),
                           pa.array([w.decode() for w in B.KNOWN_WHITELIST[3:]])])
    for ambiguous, kwargs in (("counts", None), ("counts", {"ambiguous": "counts"}), ("reject", {"ambiguous": "reject"})):
        want = B.correct_dict(B.KNOWN_ROWS, B.KNOWN_WHITELIST, ambiguous)
        out, name = plugin.call_plugin_named("barcode_correct_expr", [col, wl], kwargs, ["cbc", "whitelist"])
        assert name == "cbc" and out.type == pa.uint32()
        assert out.combine_chunks().to_pylist() == [w if s <= 1 else None for w, s in zip(want.index, want.status)]


# ------------------------------------------------------------ barcode lengths
@pytest.mark.parametrize("L,W", [(1, 1), (1, 4), (2, 9), (12, 300), (16, 300), (17, 300), (32, 300)])
def test_lengths(rg, L, W):
    rng = np.random.default_rng(100 + L + W)
    whitelist = _random_whitelist(rng, L, W)
    if L == 32:  # a legal code of all ones, and the smallest code
        whitelist[5], whitelist[9] = b"T" * 32, b"A" * 32
    wl = rg.BarcodeWhitelist(whitelist)
    assert wl.info()["L"] == L and wl.info()["W"] == W
    rows = _rows(rng, whitelist, 600)
    if L == 32:
        rows += [b"T" * 32, b"T" * 31 + b"G", b"N" + b"T" * 31, b"A" * 32, b"C" + b"A" * 31, b"T" * 31 + b"N"]
    for ambiguous in ("counts", "reject"):
        want = _check(wl, rows, whitelist, ambiguous)
    if L == 32:
        assert want.index[-6:] == [5, 5, 5, 9, 9, 5] and want.status[-6:] == [0, 1, 1, 0, 1, 1]


# ------------------------------------------------------------ the prefix table
def test_whitelist_of_one(rg):
    wl = rg.BarcodeWhitelist([b"ACGTAC"])
    assert wl.info()["prefix_digits"] == 1
    rows = [b"ACGTAC", b"ACGTAA", b"CCGTAC", b"NCGTAC", b"ACGTAN", b"AAGTAA", b"TTTTTT", b"AAAAAA", None, b""]
    want = _check(wl, rows, [b"ACGTAC"])
    assert want.status == [0, 1, 1, 1, 1, 3, 3, 3, 4, 3]


def test_complete_whitelist(rg):
    """All 4^3 codes (P = L): every regular row is exact, every one-N row has four candidates."""
    whitelist = [bytes([a, b, c]) for a in BASES for b in BASES for c in BASES]
    rng = np.random.default_rng(5)
    whitelist = [whitelist[i] for i in rng.permutation(64)]
    wl = rg.BarcodeWhitelist(whitelist)
    assert wl.info()["prefix_digits"] == 3
    rows = list(whitelist) + [b"NAA", b"ANA", b"AAN", b"TTN", b"NTT", b"NNA", b"AA", b"AAAA"] + [b"ACG"] * 3
    want = _check(wl, rows, whitelist)
    assert want.status[:64] == [0] * 64 and want.status[64:69] == [2, 2, 2, 2, 2]
    assert want.index[-3:] == [whitelist.index(b"ACG")] * 3
    prior = [0] * 64
    prior[whitelist.index(b"GAA")] = 0xFFFFFFFF  # counts near 2^32 - 1
    prior[whitelist.index(b"TAA")] = 0xFFFFFFFE
    prior[whitelist.index(b"ACA")] = prior[whitelist.index(b"AGA")] = 0xFFFFFFFF  # a tie at the top
    want = _check(wl, rows, whitelist, "counts", prior)
    assert want.index[64] == whitelist.index(b"GAA") and want.status[64:66] == [1, 2]
    _check(wl, rows, whitelist, "reject")


def test_prefix_shorter_than_barcode_and_bucket_shapes(rg):
    rng = np.random.default_rng(11)
    L = 12
    # P < L
    whitelist = _random_whitelist(rng, L, 300)
    wl = rg.BarcodeWhitelist(whitelist)
    assert 1 <= wl.info()["prefix_digits"] < L
    _check(wl, _rows(rng, whitelist, 500), whitelist)
    # every entry shares one prefix: one bucket holds the whole whitelist
    shared = [b"ACGTAC" + s for s in _random_whitelist(rng, 6, 200)]
    wl = rg.BarcodeWhitelist(shared)
    assert wl.info()["prefix_digits"] <= 6
    _check(wl, _rows(rng, shared, 500) + [b"CCGTAC" + shared[0][6:]], shared)
    # every bucket but two empty; the smallest and the largest code are entries
    two = [b"A" * 12, b"T" * 12] + [b"AAAAAA" + s for s in _random_whitelist(rng, 6, 60) if s != b"AAAAAA"] + \
          [b"TTTTTT" + s for s in _random_whitelist(rng, 6, 60) if s != b"TTTTTT"]
    wl = rg.BarcodeWhitelist(two)
    rows = _rows(rng, two, 500) + [b"A" * 12, b"T" * 12, b"A" * 11 + b"N", b"N" + b"T" * 11, b"C" + b"A" * 11,
                                   b"T" * 11 + b"G", b"G" * 12]
    want = _check(wl, rows, two)
    assert want.status[-7:-5] == [0, 0] and want.status[-1] == 3


def test_candidates_in_another_bucket_and_in_the_same(rg):
    s = b"GATTACAGATTA"
    whitelist = [b"A" + s, b"C" + s, s + b"A", s + b"C", b"T" * 13]
    wl = rg.BarcodeWhitelist(whitelist)
    rows = [b"G" + s, b"N" + s, s + b"G", s + b"N", b"A" + s, s + b"C", s + b"C"]
    want = _check(wl, rows, whitelist)
    # the highest digit: A+s has 1 exact row, C+s none; the lowest digit: s+C has 2, s+A none
    assert want.index == [0, 0, 3, 3, 0, 3, 3] and want.status == [1, 1, 1, 1, 0, 0, 0]
    want = _check(wl, rows, whitelist, "reject")
    assert want.status == [2, 2, 2, 2, 0, 0, 0]
    want = _check(wl, rows, whitelist, "counts", [0, 7, 9, 0, 0])  # the caller's counts reverse both
    assert want.index[:4] == [1, 1, 2, 2]


# ------------------------------------------------------------ rows
@pytest.fixture(scope="module")
def crowd(rg):
    """L = 6, 700 of 4096 codes: most misses have candidates, many have several."""
    rng = np.random.default_rng(77)
    whitelist = _random_whitelist(rng, 6, 700)
    return whitelist, rg.BarcodeWhitelist(whitelist)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1025, 5003])
def test_row_counts(rg, crowd, n):
    whitelist, wl = crowd
    rows = _rows(np.random.default_rng(n), whitelist, n)
    for ambiguous in ("counts", "reject"):
        _check(wl, rows, whitelist, ambiguous)


def test_miss_fractions(rg, crowd):
    whitelist, wl = crowd
    rng = np.random.default_rng(3)
    inside = set(whitelist)
    exact = [whitelist[int(i)] for i in rng.integers(0, len(whitelist), 600)]
    want = _check(wl, exact, whitelist)  # an empty miss list
    assert want.totals == [600, 0, 0, 0, 0]
    misses = [m for m in (_mutate(rng, s) for s in exact) if m not in inside]
    misses += [s[:2] + b"N" + s[3:] for s in exact[:100]]
    want = _check(wl, misses, whitelist)  # no exact row: every multi-candidate row ties at 0
    assert want.totals[0] == 0 and want.totals[1] > 0 and want.totals[2] > 0
    assert all(s != 1 or len(c) == 1 for s, c in zip(want.status, _candidate_sets(misses, whitelist)))
    assert B.correct_dict(misses, whitelist, "reject").status == want.status
    _check(wl, misses, whitelist, "reject")


def _candidate_sets(rows, whitelist):
    out = []
    for r in rows:
        out.append([k for k, w in enumerate(whitelist)
                    if len(r) == len(w) and sum(a != b for a, b in zip(r, w)) == 1])
    return out


def test_row_kinds(rg, crowd):
    whitelist, wl = crowd
    w = whitelist[0]
    rows = [b"N" + w[1:], w[:-1] + b"N", b"N" + w[1:-1] + b"N", b"NN" + w[2:], w[:-1], w + b"A", b"", w.lower(),
            w[:3] + w[3:4].lower() + w[4:], b"n" + w[1:], None, w]
    want = _check(wl, rows, whitelist)
    assert want.status[2:8] == [3, 3, 3, 3, 3, 3] and want.status[-2:] == [4, 0]
    _check(wl, rows, whitelist, "reject")
    # a null-only and an empty column
    _check(wl, [None] * 70, whitelist)
    _check(wl, [], whitelist)
    for typ in (pa.string(), pa.large_binary()):
        res = wl.correct(pa.array([], type=typ))
        assert len(res.index) == 0 and len(res.corrected) == 0 and res.counts.tolist() == [0] * len(whitelist)


def test_validity_with_a_bit_offset(rg, crowd):
    whitelist, wl = crowd
    rows = _rows(np.random.default_rng(9), whitelist, 300)
    rows[10], rows[11], rows[75] = None, None, None
    arr = _bin(rows)
    for a, b in ((3, 300), (9, 130), (64, 65), (10, 12)):
        part = arr.slice(a, b - a)
        assert part.offset == a
        _same(wl.correct(part), B.correct_dict(rows[a:b], whitelist))


# ------------------------------------------------------------ counts
def test_counts_decide(rg):
    whitelist = [b"AAAAAAAA", b"AAAAAAAC", b"AAAAAAAG", b"CCCCCCCC", b"CCCCCCCG"]
    wl = rg.BarcodeWhitelist(whitelist)
    # a strict winner among three candidates
    rows = [whitelist[0]] * 3 + [whitelist[1]] * 5 + [whitelist[2]] * 4 + [b"AAAAAAAT", b"AAAAAAAN"]
    want = _check(wl, rows, whitelist)
    assert want.index[-2:] == [1, 1]
    # a two-way tie at the top beside a smaller third candidate
    rows = [whitelist[0]] * 5 + [whitelist[1]] * 5 + [whitelist[2]] * 4 + [b"AAAAAAAT", b"AAAAAAAN"]
    want = _check(wl, rows, whitelist)
    assert want.status[-2:] == [2, 2]
    # the caller's counts reverse this call's winner
    rows = [whitelist[0]] * 3 + [whitelist[1]] * 5 + [whitelist[2]] * 4 + [b"AAAAAAAT", b"CCCCCCCA"]
    want = _check(wl, rows, whitelist, "counts", [9, 1, 1, 0, 1])
    assert want.index[-2:] == [0, 4]
    # counts near 2^32 - 1
    want = _check(wl, rows, whitelist, "counts", [0xFFFFFFFE, 0xFFFFFFFF, 0xFFFFFFFD, 0, 0])
    assert want.index[-2] == 1 and want.status[-1] == 2
    want = _check(wl, rows, whitelist, "counts", [0xFFFFFFFF, 0xFFFFFFFF, 0, 0x80000000, 0x7FFFFFFF])
    assert want.status[-2] == 2 and want.index[-1] == 3


def test_count_over_batches(rg, crowd):
    whitelist, wl = crowd
    rows = _rows(np.random.default_rng(21), whitelist, 3000)
    one = B.correct_dict(rows, whitelist)
    total = None
    for a, b in ((0, 1000), (1000, 1001), (1001, 3000)):
        total = wl.count(_bin(rows[a:b]), into=total)
    assert total.dtype == np.uint32 and total.tolist() == one.exact_counts
    assert wl.count(_bin(rows)).tolist() == one.exact_counts
    assert wl.count(_bin([])).tolist() == [0] * len(whitelist)
    # count first, correct second: every batch with the whole file's counts
    parts = [wl.correct(_bin(rows[a:b]), counts=total) for a, b in ((0, 1000), (1000, 3000))]
    assert np.concatenate([p.keys for p in parts]).tolist() == one.index


def test_skew(rg, crowd):
    """20 k rows of which 15 k are one barcode: the pre-combined atomics' case."""
    whitelist, wl = crowd
    rng = np.random.default_rng(31)
    big = whitelist[123]
    rows = [big] * 15_000 + [_mutate(rng, big) for _ in range(500)] + _rows(rng, whitelist, 4_500)
    rows = [rows[i] for i in rng.permutation(len(rows))]
    want = _check(wl, rows, whitelist)
    assert len(rows) == 20_000 and want.exact_counts[123] >= 15_000
    _check(wl, rows, whitelist, "reject")


# ------------------------------------------------------------ the probe knob
def test_both_probe_kernels_and_the_plain_search(rg):
    from rogtk_amd import _lib

    rng = np.random.default_rng(8)
    codes = rng.choice(65_536, size=20_000, replace=False)
    whitelist = [bytes(BASES[(int(c) >> (2 * (7 - j))) & 3] for j in range(8)) for c in codes]
    rows = _rows(rng, whitelist, 20_000, p_exact=0.35)
    want = {a: B.correct_dict(rows, whitelist, a) for a in ("counts", "reject")}
    for a in want:  # no branch goes untested for this seed
        assert all(t > 100 for t in want[a].totals[:4]) and want[a].totals[4] > 0, want[a].totals
    wl = rg.BarcodeWhitelist(whitelist)
    assert wl.info()["prefix_digits"] == 8
    try:
        for probe in (0, 1, 2, 3):
            _lib.call("rogtk_barcode_set_probe", probe)
            for a in want:
                _same(wl.correct(_bin(rows), a), want[a])
    finally:
        _lib.call("rogtk_barcode_set_probe", 1)  # the default
    with pytest.raises(_lib.RogtkError):
        _lib.call("rogtk_barcode_set_probe", 4)


# ------------------------------------------------------------ invariance, composition
def test_row_order_and_chunking_change_nothing(rg, crowd):
    whitelist, wl = crowd
    rng = np.random.default_rng(41)
    rows = _rows(rng, whitelist, 2000)
    base = _check(wl, rows, whitelist)
    p = rng.permutation(len(rows))
    shuffled = [rows[i] for i in p]
    cuts = [0, 1, 700, 701, 2000]
    col = pa.chunked_array([_bin(shuffled[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
    res = wl.correct(col)
    assert res.keys.tolist() == [base.index[i] for i in p] and res.status.tolist() == [base.status[i] for i in p]
    assert res.counts.tolist() == base.counts and res.exact_counts.tolist() == base.exact_counts
    assert list(res.totals.values()) == base.totals


def test_composition_with_grouped_umi_correction(rg, crowd):
    """FASTQ batch -> BarcodeWhitelist.correct -> umi_correct(groups=res.keys)."""
    whitelist, wl = crowd
    rng = np.random.default_rng(51)
    cells = [whitelist[int(i)] for i in rng.integers(0, 40, 3000)]
    cbcs = [c if rng.random() < 0.9 else _mutate(rng, c) for c in cells]
    cbcs[7], cbcs[8] = None, b"NN" + cbcs[8][2:]
    parents = _random_whitelist(rng, 12, 60)
    umis = [parents[int(i)] if rng.random() < 0.85 else _mutate(rng, parents[int(i)])
            for i in rng.integers(0, 60, 3000)]
    want = B.correct_dict(cbcs, whitelist)
    res = wl.correct(_bin(cbcs))
    _same(res, want)
    got = rg.umi_correct(_bin(umis), 12, method="directional", groups=res.keys)
    ref = rg.umi_correct(_bin(umis), 12, method="directional", groups=np.asarray(want.index, dtype=np.uint32))
    keep = np.asarray(want.status) <= 1
    assert 0 < keep.sum() < len(cbcs)
    assert np.array_equal(np.asarray(got.cluster_id.to_numpy(zero_copy_only=False))[keep],
                          np.asarray(ref.cluster_id.to_numpy(zero_copy_only=False))[keep])
    assert got.corrected.to_pylist() == ref.corrected.to_pylist()
    # two rows share a cluster only inside one corrected cell
    cid = np.asarray(got.cluster_id.to_numpy(zero_copy_only=False))
    cell_of = {}
    for c, k in zip(cid[keep], np.asarray(want.index)[keep]):
        assert cell_of.setdefault(int(c), int(k)) == int(k)
