"""The string, fuzzy and barcode host entries on the shared level-2 layer: one
per-thread context with three input-column slots, one upload (sliced columns rebased on the
host), one writer of a rogtk_str_result, staged and pinned transfers.

Expected values come from oracle/pystrings.py (through tests/strings_cases.py), the regex
restatement of tests/test_fuzzy.py, tests/barcode_spec.py and tests/correct_spec.py, or, at
the one size the per-row oracle cannot hold, a vectorised numpy reverse complement; never from
a second run of the code under test.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pyarrow as pa
import pytest

import barcode_spec as B
import strings_cases as C
from correct_spec import as_bytes, restate
from test_fuzzy import gen_pattern, re_replace
from test_gpu_barcode import _random_whitelist, _rows

pytestmark = pytest.mark.gpu

TARGET, REPL = "ACGT", "<R>"


@pytest.fixture(scope="module")
def S():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from rogtk_amd import strings

    return strings


@pytest.fixture(scope="module")
def crowd():
    """tests/test_gpu_barcode.py's crowded whitelist: L = 6, 700 of 4096 codes."""
    import rogtk_amd as rg

    whitelist = _random_whitelist(np.random.default_rng(77), 6, 700)
    return whitelist, rg.BarcodeWhitelist(whitelist)


def _enc(rows):
    return [None if r is None else r.encode() if isinstance(r, str) else bytes(r) for r in rows]


def _same_column(got: pa.Array, want):
    """null_count, offsets, values and validity of an output column against its expected rows
    (bytes or None; a null row has no bytes)."""
    n = len(want)
    assert len(got) == n and got.offset == 0
    assert got.null_count == sum(w is None for w in want)
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([0 if w is None else len(w) for w in want], out=offs[1:])
    validity, offsets, values = got.buffers()
    wide = pa.types.is_large_string(got.type) or pa.types.is_large_binary(got.type)
    assert np.frombuffer(offsets, dtype=np.int64 if wide else np.int32, count=n + 1).tolist() == offs.tolist()
    have = b"" if values is None else values.to_pybytes()[:int(offs[-1])]
    assert have == b"".join(w for w in want if w is not None)
    if got.null_count:
        bits = np.unpackbits(np.frombuffer(validity, dtype=np.uint8), bitorder="little")[:n]
        assert bits.tolist() == [int(w is not None) for w in want]
    else:
        assert validity is None


def _transform(S, op, arrays, n, param=0):
    """rogtk_str_transform_host on pyarrow arrays as they are (slices included), n output rows."""
    from rogtk_amd import _lib
    from rogtk_amd.columns import one_chunk

    keep = [one_chunk(a, rebase=False) for a in arrays]
    descs = (_lib.StrCol * len(arrays))(*[ch.desc() for ch in keep])
    res = _lib.StrResult()
    _lib.check(_lib.hip().rogtk_str_transform_host(C.OPS[op], descs, len(arrays), n, param, ctypes.byref(res)))
    return _lib.take_str(res)


def _dna(rng, n, lo, hi):
    return C._rand_dna(rng, n, lo, hi, "ACGTN")


def _fuzzy_rows(rng, n):
    rows = []
    for s in _dna(rng, n, 0, 90):
        if rng.random() < 0.6:  # the target, or a one-edit neighbour of it, somewhere inside
            hit = TARGET if rng.random() < 0.5 else TARGET[:2] + "N" + TARGET[3:]
            k = int(rng.integers(0, len(s) + 1))
            s = s[:k] + hit + s[k:]
        rows.append(s)
    rows[n // 3] = None
    return rows


def _replace_target(S, rows_or_array):
    return S.FuzzyNamespace(rows_or_array).replace_target(TARGET, REPL)


def _want_replace(rows):
    return _enc(re_replace(gen_pattern(TARGET), REPL, rows, False))


# ------------------------------------------------------------------ 1. sliced inputs per slot
@pytest.mark.parametrize("typ", [pa.string(), pa.large_string()], ids=["string", "large_string"])
@pytest.mark.parametrize("broadcast", [False, True], ids=["rows", "broadcast0"])
@pytest.mark.parametrize("name,op", [("aligned_ref", "aligned_ref"), ("enrich", "enrich")])
def test_sliced_inputs_per_slot(S, name, op, broadcast, typ):
    n = 65
    case = C.random_case(name, n)
    cols = [list(c) for c in case["cols"]]
    if broadcast:
        cols[0] = [next(x for x in cols[0] if x)]
    arrays = []
    for k, (col, lead) in enumerate(zip(cols, (3, 8, 13))):
        junk = [None if j % 3 == 1 else "TTGCA"[: 1 + j % 5] * (k + 1) for j in range(lead)]
        a = pa.array(junk + col + ["tail"], type=typ).slice(lead, len(col))
        offs = np.frombuffer(a.buffers()[1], dtype=np.int64 if typ == pa.large_string() else np.int32)
        assert a.offset == lead and offs[lead] > 0  # another bit offset and another first offset per slot
        arrays.append(a)
    want = C.expected({"op": op, "param": 0, "cols": cols})
    assert len(want) == n and any(w for w in want)
    # enrich hands the allele through where seq or cigar is null: its nulls are the allele's alone
    assert any(w is None for w in want) or (op == "enrich" and broadcast)
    _same_column(_transform(S, op, arrays, n), want)


# ------------------------------------------------------------------ 2. one thread, many entries
def test_slot_reuse_and_regrowth_on_one_thread(S, crowd):
    import rogtk_amd as rg

    whitelist, wl = crowd
    rng = np.random.default_rng(11)
    first = C.random_case("revcomp", 1000)
    want_first = C.expected(first)

    def revcomp_first():
        return S.reverse_complement(pa.array(first["cols"][0], type=pa.large_string()))

    got_first = revcomp_first()
    _same_column(got_first, want_first)

    frows = _fuzzy_rows(rng, 257)
    _same_column(_replace_target(S, pa.array(frows, type=pa.string())), _want_replace(frows))

    brows = _rows(np.random.default_rng(5003), whitelist, 5003)
    res = wl.correct(pa.array(brows, type=pa.large_binary()))
    want = B.correct_dict(brows, whitelist)
    assert res.status.tolist() == want.status
    _same_column(res.corrected, want.corrected)

    seeds = [bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, 8)) for _ in range(12)]
    urows = []
    for _ in range(300):
        s = seeds[int(rng.integers(0, len(seeds)))]
        if rng.random() < 0.3:
            j = int(rng.integers(0, 8))
            s = s[:j] + b"ACGTN"[int(rng.integers(0, 5)):][:1] + s[j + 1:]
        urows.append(s)
    urows[17] = None
    ures = rg.umi_correct(pa.array(urows, type=pa.large_binary()), 8, 1)
    ids, k, _, corrected = restate(urows, 8, 1)
    assert ures.n_clusters == k and ures.cluster_id.to_pylist() == ids
    _same_column(ures.corrected, corrected)

    long_rows = _dna(rng, 63, 20000, 30000)  # 63 rows that outgrow what the 1,000 left behind
    long_rows[5] = None
    _same_column(S.reverse_complement(pa.array(long_rows, type=pa.large_string())),
                 C.expected({"op": "revcomp", "param": 0, "cols": [long_rows]}))

    again = revcomp_first()
    _same_column(again, want_first)
    assert again.equals(got_first)


# ------------------------------------------------------------------ 3. edge sizes
_EDGE = {
    "n=0": lambda rows: [],
    "all-null-64": lambda rows: [None] * 64,
    "no-bytes-64": lambda rows: [""] * 64,
    "65-partial-word": lambda rows: [None if i in (0, 31, 63, 64) else r for i, r in enumerate(rows[:65])],
}


@pytest.mark.parametrize("edge", list(_EDGE))
@pytest.mark.parametrize("entry", ["revcomp", "fuzzy_replace", "barcode_corrected"])
def test_edge_sizes_through_the_shared_writer(S, crowd, entry, edge):
    rng = np.random.default_rng(3)
    if entry == "barcode_corrected":
        whitelist, wl = crowd
        base = [None if r is None else r.decode() for r in _rows(rng, whitelist, 70)]
    else:
        base = _fuzzy_rows(rng, 70)
    rows = _EDGE[edge](base)
    arr = pa.array(rows, type=pa.large_string())
    if entry == "revcomp":
        got, want = S.reverse_complement(arr), C.expected({"op": "revcomp", "param": 0, "cols": [rows]}) if rows else []
    elif entry == "fuzzy_replace":
        got, want = _replace_target(S, arr), _want_replace(rows)
    else:  # an empty string matches no barcode: valid rows in, an all-null column without bytes out
        got, want = wl.correct(arr).corrected, B.correct_dict(_enc(rows), whitelist).corrected
        assert edge != "no-bytes-64" or want == [None] * 64
    _same_column(got, want)


# ------------------------------------------------------------------ 4. staged and pinned transfers
_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCAtgca"):
    _COMP[_a] = _b


def test_staged_transfer_of_more_than_two_chunks(S):
    """70 MiB of values: three 32 MiB chunks up and three down, the third through the first
    staging buffer again."""
    n, w = 70 * (1 << 20) // 64, 64
    rng = np.random.default_rng(4)
    vals = np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.integers(0, 5, size=(n, w), dtype=np.uint8)]
    assert vals.nbytes > 2 * (32 << 20)
    offsets = np.arange(n + 1, dtype=np.int64) * w
    col = pa.Array.from_buffers(pa.large_string(), n, [None, pa.py_buffer(offsets), pa.py_buffer(vals)])
    got = S.reverse_complement(col)
    assert len(got) == n and got.null_count == 0
    _, goff, gval = got.buffers()
    assert np.array_equal(np.frombuffer(goff, dtype=np.int64, count=n + 1), offsets)
    assert np.array_equal(np.frombuffer(gval, dtype=np.uint8, count=n * w).reshape(n, w), _COMP[vals][:, ::-1])


def test_pinned_input_goes_by_direct_dma(S):
    from rogtk_amd import _lib

    lib = _lib.hip()
    n, w = 4096, 64  # 256 KiB of values straight from the pinned block; the 32 KiB of offsets are a small copy
    rng = np.random.default_rng(5)
    vals = np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.integers(0, 5, size=(n, w), dtype=np.uint8)]
    blocks = [ctypes.c_void_p(), ctypes.c_void_p()]
    try:
        _lib.check(lib.rogtk_host_alloc((n + 1) * 8, ctypes.byref(blocks[0])))
        _lib.check(lib.rogtk_host_alloc(n * w + 1, ctypes.byref(blocks[1])))
        offs = np.ctypeslib.as_array(ctypes.cast(blocks[0], ctypes.POINTER(ctypes.c_int64)), (n + 1,))
        pinned = np.ctypeslib.as_array(ctypes.cast(blocks[1], ctypes.POINTER(ctypes.c_uint8)), (n * w + 1,))
        offs[:] = np.arange(n + 1, dtype=np.int64) * w
        pinned[: n * w] = vals.reshape(-1)
        desc = (_lib.StrCol * 1)(_lib.StrCol(blocks[0], 8, blocks[1], n * w + 1, None, 0, n))
        res = _lib.StrResult()
        _lib.check(lib.rogtk_str_transform_host(C.OPS["revcomp"], desc, 1, n, 0, ctypes.byref(res)))
        _, goff, gval, _, nulls = _lib.take_str_buffers(res)
    finally:
        for b in blocks:
            lib.rogtk_host_free(b)
    assert nulls == 0 and np.array_equal(goff, np.arange(n + 1, dtype=np.int64) * w)
    assert np.array_equal(gval.reshape(n, w), _COMP[vals][:, ::-1])


# ------------------------------------------------------------------ 5. failure frees
@pytest.mark.parametrize("case", C.OVER_CAP, ids=lambda c: c["name"])
def test_over_cap_leaves_the_result_zeroed(S, case):
    from rogtk_amd import _lib
    from rogtk_amd.columns import one_chunk

    lib = _lib.hip()
    arrays = [pa.array(c, type=pa.large_string()) for c in case["cols"]]
    n = max(len(a) for a in arrays)
    keep = [one_chunk(a, rebase=False) for a in arrays]
    descs = (_lib.StrCol * len(arrays))(*[ch.desc() for ch in keep])
    res = _lib.StrResult()
    res.n = 77
    rc = lib.rogtk_str_transform_host(C.OPS[case["op"]], descs, len(arrays), n, case["param"], ctypes.byref(res))
    try:
        assert rc == _lib.ROGTK_E_UNSUPPORTED, lib.rogtk_last_error()
        assert f"row {case['over'][0]}:" in lib.rogtk_last_error().decode()
        assert not res.offsets and not res.values and not res.validity and res.n == 0
    finally:
        lib.rogtk_str_result_free(ctypes.byref(res))
