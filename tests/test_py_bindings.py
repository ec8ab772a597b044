"""The one layer between the Python wrappers and the C ABI: a host column as a
rogtk_str_col (rogtk_amd/columns.py), a per-row integer argument as uint32 (columns.as_u32), and
the library-allocated results as Arrow (rogtk_amd/_lib.py). Needs the built library (the takers
free through it), no device."""
from __future__ import annotations

import ctypes
import gc
import glob
import os
import re

import numpy as np
import pyarrow as pa
import pytest

import py_binding_cases as C
from rogtk_amd import _lib, columns

PKG = os.path.dirname(os.path.abspath(_lib.__file__))
ROWS = ["".join("ACGT"[(i * 7 + j * j) % 4] for j in range(i % 9 + 3)) for i in range(C.N_ROWS)]
for _i in (0, 5, 6, 40, 69):
    ROWS[_i] = None
ROWS[9] = ""


# ------------------------------------------------------------------ the column
def _read_back(d):
    """The rows (bytes or None) that the addresses of a rogtk_str_col describe."""
    n = d.n
    offs = _lib.copy_out(d.offsets, np.int64 if d.offset_width == 8 else np.int32, n + 1)
    vals = _lib.copy_out(d.values, np.uint8, d.values_len).tobytes()
    valid = np.ones(n, dtype=bool)
    if d.validity:
        nbytes = (d.validity_offset + n + 7) // 8
        bits = np.unpackbits(_lib.copy_out(d.validity, np.uint8, nbytes), bitorder="little")
        valid = bits[d.validity_offset:d.validity_offset + n].astype(bool)
    else:
        assert d.validity_offset == 0
    assert len(offs) == n + 1 and (n == 0 or int(offs[-1]) <= len(vals))
    return [vals[offs[i]:offs[i + 1]] if valid[i] else None for i in range(n)]


def _as_bytes(rows):
    return [r.encode() if isinstance(r, str) else r for r in rows]


FORMS = [(kind, name, col) for kind in C.TYPES for name, col, _ in C.forms(ROWS, kind)]


@pytest.mark.parametrize("rebase", [True, False])
@pytest.mark.parametrize("kind,name,col", FORMS, ids=[f"{k}-{n}" for k, n, _ in FORMS])
def test_descriptor_reads_back_the_rows(kind, name, col, rebase):
    ch = columns.one_chunk(col, rebase=rebase)
    d = ch.desc()
    assert d.n == ch.n == len(col) and d.offset_width == ch.offset_width
    assert _read_back(d) == _as_bytes(col.to_pylist())
    loose = ch.loose()
    assert [getattr(a, "value", a) for a in loose] == [d.offsets, d.offset_width, d.values, d.values_len, d.validity,
                                                       d.validity_offset, d.n]
    offsets_buf = ch.arrow.buffers()[1]
    if rebase:
        assert ch.n == 0 or int(ch.offsets[0]) == 0
    elif offsets_buf is not None and offsets_buf.size:
        assert np.shares_memory(ch.offsets, np.frombuffer(offsets_buf, dtype=np.uint8))
        assert d.values_len == max(ch.arrow.buffers()[2].size if ch.arrow.buffers()[2] is not None else 0, 1)


def test_chunks_yields_every_chunk_rebased():
    col = C.forms(ROWS, "string")[-1][1]
    got = [r for ch in columns.chunks(col) for r in _read_back(ch.desc())]
    assert got == _as_bytes(col.to_pylist()) and len(list(columns.chunks(col))) == 3


@pytest.mark.parametrize("rebase", [True, False])
def test_descriptor_keeps_a_temporary_alive(rebase):
    rows = [None if i % 11 == 0 else f"ROW{i:06d}" * 3 for i in range(5000)]

    def make():
        return columns.one_chunk(pa.array(rows, type=pa.string()).slice(3), rebase=rebase).desc()

    d = make()
    gc.collect()
    junk = [np.full(1 << 16, 0xAB, dtype=np.uint8) for _ in range(64)]  # what freed memory would be handed to
    assert _read_back(d) == _as_bytes(rows[3:])
    del junk


def test_text_type_follows_the_input():
    for kind, want in (("string", pa.large_string()), ("large_string", pa.large_string()),
                       ("string_view", pa.large_string()), ("binary", pa.large_binary())):
        assert columns.text_type(columns.one_chunk(pa.array(["A"], type=C.TYPES[kind]))) == want
    assert columns.text_type(columns.one_chunk(pa.array([b"A"], type=pa.large_binary()))) == pa.large_binary()


# ------------------------------------------------------------------ as_u32
NAMES = ["groups", "counts", "score"]


@pytest.mark.parametrize("name", NAMES)
def test_as_u32_accepts(name):
    want = np.array([3, 0, 4294967295, 7], dtype=np.uint32)
    same = columns.as_u32(want, name, rows=4)
    assert same is want or (np.shares_memory(same, want) and same.dtype == np.uint32)
    inputs = [want.astype(np.int64), want.astype(np.uint64), [3, 0, 4294967295, 7], pa.array(want),
              pa.array(want.astype(np.int64)), pa.chunked_array([pa.array(want[:1]), pa.array(want[1:])]),
              want.astype(np.int64)[::-1][::-1], np.stack([want, want], axis=1)[:, 0]]
    for x in inputs:
        got = columns.as_u32(x, name, rows=4)
        assert got.dtype == np.uint32 and got.flags.c_contiguous and got.tolist() == want.tolist()
    small = pa.array([1, 2, 3], type=pa.uint8())
    assert columns.as_u32(small, name).tolist() == [1, 2, 3]
    for empty in (pa.chunked_array([], type=pa.uint32()), np.zeros(0, np.int16), pa.array([], type=pa.int8()), []):
        got = columns.as_u32(empty, name, rows=0)
        assert got.dtype == np.uint32 and got.shape == (0,)


@pytest.mark.parametrize("name", NAMES)
def test_as_u32_fills_nulls_only_when_asked(name):
    for typ in (pa.uint32(), pa.int8(), pa.int64(), pa.uint64()):
        x = pa.array([1, None, 2], type=typ)
        with pytest.raises(ValueError, match=rf"{name}.*nulls"):
            columns.as_u32(x, name)
        assert columns.as_u32(x, name, nulls_to=0xFFFFFFFF).tolist() == [1, 0xFFFFFFFF, 2]
        assert columns.as_u32(pa.chunked_array([x, x]), name, rows=6, nulls_to=9).tolist() == [1, 9, 2, 1, 9, 2]
    big = pa.array([1, None, 2**63], type=pa.uint64())  # not through int64: the refusal is the range's
    with pytest.raises(ValueError, match=rf"{name}.*0\.\.2\^32-1"):
        columns.as_u32(big, name, nulls_to=0)


REFUSED = [
    ("arrow float", pa.array([1.0, 2.0, 3.0]), "integer"),
    ("arrow bool", pa.array([True, False, True]), "integer"),
    ("arrow string", pa.array(["1", "2", "3"]), "integer"),
    ("chunked float", pa.chunked_array([pa.array([1.0, 2.0, 3.0])]), "integer"),
    ("numpy float", np.zeros(3, np.float64), "integer"),
    ("numpy bool", np.zeros(3, bool), "integer"),
    ("empty numpy float", np.zeros(0, np.float32), "integer"),
    ("nulls", pa.array([1, None, 0], type=pa.uint32()), "nulls"),
    ("chunked nulls", pa.chunked_array([pa.array([1, 2], type=pa.int64()), pa.array([None], type=pa.int64())]), "nulls"),
    ("2-D", np.zeros((3, 1), np.uint32), None),
    ("0-D", np.zeros((), np.uint32), None),
    ("short", np.zeros(2, np.uint32), "shape.*3"),
    ("long", pa.array([1, 2, 3, 4], type=pa.uint8()), "shape.*3"),
    ("negative", np.array([1, -1, 0]), r"0\.\.2\^32-1"),
    ("negative arrow", pa.array([1, -1, 0], type=pa.int8()), r"0\.\.2\^32-1"),
    ("past u32", np.array([1, 2**32, 0], dtype=np.int64), r"0\.\.2\^32-1"),
    ("past u32 arrow", pa.array([1, 2**32, 0], type=pa.uint64()), r"0\.\.2\^32-1"),
]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("what,x,needs", REFUSED, ids=[r[0] for r in REFUSED])
def test_as_u32_refuses(name, what, x, needs, monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "call", no_library)
    monkeypatch.setattr(_lib, "hip", no_library)
    with pytest.raises(ValueError, match=name if needs is None else rf"{name}.*{needs}"):
        columns.as_u32(x, name, rows=3)


def test_as_u32_answers_in_one_order():
    """type before nulls before shape before range, whoever asks."""
    with pytest.raises(ValueError, match="integer"):
        columns.as_u32(pa.array([1.5, None]), "groups", rows=3)
    with pytest.raises(ValueError, match="nulls"):
        columns.as_u32(pa.array([-1, None]), "groups", rows=3)
    with pytest.raises(ValueError, match="1-D"):
        columns.as_u32(np.full((2, 2), -1), "groups", rows=3)
    with pytest.raises(ValueError, match="shape"):
        columns.as_u32(np.array([-1, 2**40]), "groups", rows=3)


# ------------------------------------------------------------------ the takers
_libc = ctypes.CDLL(None)
_libc.malloc.restype = ctypes.c_void_p
_libc.malloc.argtypes = [ctypes.c_size_t]


def _malloced(a: np.ndarray) -> int:
    """a's bytes in a block of libc malloc (at least one byte), which the library's free() takes."""
    p = _libc.malloc(max(a.nbytes, 1))
    assert p
    ctypes.memmove(p, a.ctypes.data, a.nbytes)
    return p


def _str_result(rows) -> _lib.StrResult:
    n = len(rows)
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([0 if r is None else len(r) for r in rows], out=offs[1:])
    vals = np.frombuffer(b"".join(r for r in rows if r is not None), dtype=np.uint8)
    bits = np.zeros(max((n + 63) // 64, 1) * 64, dtype=np.uint8)
    bits[:n] = [r is not None for r in rows]
    return _lib.StrResult(n, _malloced(offs), _malloced(vals), vals.size, _malloced(np.packbits(bits, bitorder="little")),
                          sum(r is None for r in rows))


def _u32_result(values) -> _lib.U32Result:
    return _lib.U32Result(len(values), _malloced(np.asarray(values, dtype=np.uint32)))


def _zeroed(res) -> bool:
    if isinstance(res, _lib.U32Result):
        return not res.data and res.n == 0
    return not res.offsets and not res.values and not res.validity and res.n == 0 and res.values_len == 0


STR_ROWS = {
    "no rows": [],
    "no bytes": [b"", b"", b""],
    "no nulls": [b"ACGT", b"", b"TT"],
    "nulls": [None, b"ACGT", None, b"G"],
    "all null": [None] * 3,
    "65 rows": [None if i in (0, 63, 64) else b"AC" * (i % 3) for i in range(65)],
}


@pytest.mark.parametrize("rows", STR_ROWS.values(), ids=list(STR_ROWS))
def test_take_str(rows):
    for typ, want in ((None, [None if r is None else r.decode() for r in rows]), (pa.large_binary(), rows)):
        res = _str_result(rows)
        got = _lib.take_str(res) if typ is None else _lib.take_str(res, typ)
        assert _zeroed(res)
        assert got.type == (typ or pa.large_string()) and got.to_pylist() == want
        assert got.null_count == sum(r is None for r in rows)
        assert (got.buffers()[0] is None) == (got.null_count == 0)
        got.validate(full=True)
    res = _str_result(rows)
    n, offs, vals, bits, nulls = _lib.take_str_buffers(res)
    assert _zeroed(res)
    assert n == len(rows) and nulls == sum(r is None for r in rows) and offs.dtype == np.int64 and len(offs) == n + 1
    assert vals.tobytes() == b"".join(r for r in rows if r is not None)
    assert bits.dtype == np.uint8 and len(bits) == max((n + 63) // 64, 1) * 8
    assert np.unpackbits(bits, bitorder="little")[:n].tolist() == [int(r is not None) for r in rows]


@pytest.mark.parametrize("values", [[], [7], [0, 4294967295, 5]])
def test_take_u32(values):
    res = _u32_result(values)
    got = _lib.take_u32(res)
    assert _zeroed(res)
    assert got.type == pa.uint32() and got.null_count == 0 and got.to_pylist() == values


@pytest.mark.parametrize("rows", STR_ROWS.values(), ids=list(STR_ROWS))
def test_a_refused_conversion_still_frees(rows):
    res = _str_result(rows)
    with pytest.raises((pa.ArrowException, ValueError, TypeError)):
        _lib.take_str(res, pa.int32())  # three buffers for a type of two
    assert _zeroed(res)


def test_take_all_frees_every_result_before_it_raises():
    def results():
        return [_str_result([b"AC", None]), _str_result([b"G"]), _u32_result([1, 2]), _u32_result([3]), _u32_result([])]

    res = results()
    got = _lib.take_all(res, pa.large_binary())
    assert all(_zeroed(r) for r in res)
    assert [g.to_pylist() for g in got] == [[b"AC", None], [b"G"], [1, 2], [3], []]
    res = results()
    with pytest.raises((pa.ArrowException, ValueError, TypeError)):
        _lib.take_all(res, pa.int32())  # the first conversion fails; the other four are still taken
    assert all(_zeroed(r) for r in res)


# ------------------------------------------------------------------ one implementation of each job
def _sources():
    return {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(PKG, "*.py")))}


@pytest.mark.parametrize("word,allowed", [
    ("rogtk_str_result_free", {"_lib.py"}),
    ("rogtk_u32_result_free", {"_lib.py"}),
    ("StrCol(", {"_lib.py", "columns.py"}),
    ("ctypeslib.as_array", {"_lib.py"}),
    ("from_address", {"_lib.py"}),
    ("string_at", {"_lib.py"}),
])
def test_named_only_in(word, allowed):
    assert {name for name, text in _sources().items() if word in text} <= allowed


def test_no_underscore_name_comes_from_a_sibling():
    found = []
    for name, text in _sources().items():
        for m in re.finditer(r"^\s*from \.(\w+) import (\([^)]*\)|[^\n]*)", text, flags=re.M):
            names = [w.split(" as ")[0].strip() for w in re.sub(r"[()\\]|#[^\n]*", "", m.group(2)).split(",")]
            found += [(name, m.group(1), w) for w in names if w.startswith("_") and m.group(1) != "_lib"]
    assert found == []


def test_the_replaced_helpers_are_gone():
    from rogtk_amd import api, bam, barcode, correct, dedup, strings

    gone = [(strings, "_single"), (strings, "_desc"), (strings, "_take_result"), (strings, "_string_array"),
            (correct, "_desc"), (correct, "_take_str"), (correct, "_take_u32"), (correct, "_text_type"),
            (api, "_ptr"), (api, "group_keys"), (barcode, "_u32_counts"), (dedup, "_host_u32"), (dedup, "_ptr"),
            (bam, "_np_from")]
    assert [(m.__name__, n) for m, n in gone if hasattr(m, n)] == []


# ------------------------------------------------------------------ the side libraries
def test_each_side_library_is_loaded_once_and_is_its_own():
    d, c = _lib.dedup(), _lib.count()
    assert _lib.dedup() is d and _lib.count() is c
    assert d is not c and d is not _lib.hip() and c is not _lib.hip()


def test_call_routes_by_the_prefix_table(monkeypatch):
    class Recorder:
        def __init__(self):
            self.names = []

        def __call__(self):
            return self

        def __getattr__(self, name):
            self.names.append(name)
            return lambda *args: _lib.ROGTK_OK

    rec = {which: Recorder() for which in ("dedup", "count", "hip")}
    for which, r in rec.items():
        monkeypatch.setattr(_lib, which, r)  # call() looks the loaders up when it is called
    sent = {"dedup": ["rogtk_cluster_best_rows", "rogtk_cluster_best_temp_bytes", "rogtk_cluster_best_geometry"],
            "count": ["rogtk_count_matrix", "rogtk_count_matrix_host", "rogtk_count_matrix_set_phases"],
            "hip": ["rogtk_cluster_summary_dev", "rogtk_device_count", "rogtk_barcode_count_dev"]}
    for names in sent.values():
        for name in names:
            _lib.call(name, 1, 2)
    assert {which: r.names for which, r in rec.items()} == sent
    assert set(_lib.SIDE_LIBS) == {"dedup", "count"}
    assert _lib.SIDE_LIBS["dedup"] == (_lib.DEDUP_PREFIX, _lib.DEDUP_LIB_PATH)
    assert _lib.SIDE_LIBS["count"] == (_lib.COUNT_PREFIX, _lib.COUNT_LIB_PATH)
