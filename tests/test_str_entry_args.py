"""The argument rules of the string and fuzzy host entries (include/rogtk_hip.h), in one table in
the style of test_umi_entry_args.py: rogtk_str_transform_host, rogtk_fuzzy_contains_host and
rogtk_fuzzy_replace_host, called through _lib.hip() with one bad argument each on a 3-row
column.

Every refusal comes before the library looks for a device, so the table runs on
a machine without a GPU. The expected codes are the library's answers as they stand. The cases
marked COLUMN are the fuzzy entries' checks of the column itself: before these entries moved
onto the level-2 layer they looked for a device first, and answered these calls with
ROGTK_E_NODEVICE on a machine without one.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from rogtk_amd import _lib
from rogtk_amd.strings import PHRED_STR, REVCOMP

E, U = _lib.ROGTK_E_INVALID, _lib.ROGTK_E_UNSUPPORTED
COLUMN = "column"  # answered only where a device was present, before the shared layer
ARGS = "args"

N = 3
_OFF = np.arange(N + 1, dtype=np.int64) * 4
_OFF32 = _OFF.astype(np.int32)
_OFF_DOWN = np.array([0, 4, 2, 8], dtype=np.int64)
_VAL = np.frombuffer(b"ACGTACGAACGT", dtype=np.uint8).copy()
_BITS = np.zeros(2, dtype=np.uint64)
NULL_OUT, NULL_COLS, NULL_COL, NULL_PROGRAM = "out=NULL", "cols=NULL", "col=NULL", "program=NULL"


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _col(**bad):
    a = {"offsets": _p(_OFF), "ow": 8, "values": _p(_VAL), "values_len": _VAL.size, "validity": None, "voff": 0,
         "n": N, **bad}
    return _lib.StrCol(a["offsets"], a["ow"], a["values"], a["values_len"], a["validity"], a["voff"], a["n"])


def _zeroed(res):
    return not res.offsets and not res.values and not res.validity and res.n == 0


def _str_call(op=REVCOMP, n_cols=1, n_rows=N, param=0, col=None, flag=None):
    lib = _lib.hip()
    res = _lib.StrResult()
    cols = (_lib.StrCol * 3)(*[_col(**(col or {})) for _ in range(3)])
    rc = lib.rogtk_str_transform_host(op, None if flag == NULL_COLS else cols, n_cols, n_rows, param,
                                      None if flag == NULL_OUT else ctypes.byref(res))
    msg = lib.rogtk_last_error().decode() if rc else ""
    zero = _zeroed(res)
    lib.rogtk_str_result_free(ctypes.byref(res))
    return rc, msg, zero


@pytest.fixture(scope="module")
def program():
    h = ctypes.c_void_p()
    _lib.call("rogtk_fuzzy_compile_native", b"ACGT", 4, b".{0,1}", 1, 100, ctypes.byref(h))
    _lib.call("rogtk_fuzzy_set_replacement", h, b"x", 1)
    yield h
    _lib.hip().rogtk_fuzzy_free(h)


def _fuzzy_call(entry, program, col=None, flag=None):
    lib = _lib.hip()
    res = _lib.StrResult()
    desc = _col(**(col or {}))
    p = None if flag == NULL_PROGRAM else program
    c = None if flag == NULL_COL else ctypes.byref(desc)
    if entry == "rogtk_fuzzy_contains_host":
        rc = lib.rogtk_fuzzy_contains_host(p, c, _p(_BITS), _p(_BITS))
    else:
        rc = lib.rogtk_fuzzy_replace_host(p, c, 0, ctypes.byref(res))
    msg = lib.rogtk_last_error().decode() if rc else ""
    zero = _zeroed(res)
    lib.rogtk_str_result_free(ctypes.byref(res))
    return rc, msg, zero


# (name, arguments of _str_call, expected code, substring of the message or None)
STR_CASES = [
    ("unknown-op", dict(op=99), E, "unknown string op 99"),
    ("column-count", dict(n_cols=2), E, "takes 1 input columns, got 2"),
    ("n_rows=-1", dict(n_rows=-1), E, "n_rows"),
    ("ow=3", dict(col=dict(ow=3)), E, "offset_width"),
    ("2-rows-next-to-3", dict(col=dict(n=2)), E, "2 rows"),
    ("phred-base=256", dict(op=PHRED_STR, param=256), E, "u8"),
    (NULL_OUT, dict(flag=NULL_OUT), E, None),
    (NULL_COLS, dict(flag=NULL_COLS), E, None),
]

# (name, arguments of _fuzzy_call, expected code, substring of the message or None, ARGS / COLUMN)
FUZZY_CASES = [
    (NULL_PROGRAM, dict(flag=NULL_PROGRAM), E, None, ARGS),
    (NULL_COL, dict(flag=NULL_COL), E, None, ARGS),
    ("offsets=NULL", dict(col=dict(offsets=None)), E, "null column", COLUMN),
    ("ow=2", dict(col=dict(ow=2)), E, "offset_width", COLUMN),
    ("n=-1", dict(col=dict(n=-1)), U, "2^31 - 2 rows", COLUMN),
    ("n=2^31-1", dict(col=dict(n=(1 << 31) - 1)), U, "2^31 - 2 rows", COLUMN),
    ("offsets-decrease", dict(col=dict(offsets=_p(_OFF_DOWN))), E, "offsets decrease at row 1", COLUMN),
    ("offsets-past-values_len", dict(col=dict(values_len=_VAL.size - 1)), E, "outside values", COLUMN),
]
FUZZY_ENTRIES = ("rogtk_fuzzy_contains_host", "rogtk_fuzzy_replace_host")


def test_the_tables_name_the_entries_of_the_library():
    lib = _lib.hip()
    for e in FUZZY_ENTRIES + ("rogtk_str_transform_host",):
        assert hasattr(lib, e) and e in _lib.SIGNATURES, e
    assert sum(kind == COLUMN for *_, kind in FUZZY_CASES) == 6


@pytest.mark.parametrize("case", STR_CASES, ids=lambda c: c[0])
def test_bad_str_transform_call(case):
    _, args, want, text = case
    rc, msg, zero = _str_call(**args)
    assert rc == want, (rc, msg)
    assert zero
    if text:
        assert text in msg, msg


@pytest.mark.parametrize("entry", FUZZY_ENTRIES)
@pytest.mark.parametrize("case", FUZZY_CASES, ids=lambda c: c[0])
def test_bad_fuzzy_call(case, entry, program):
    _, args, want, text, _ = case
    rc, msg, zero = _fuzzy_call(entry, program, **args)
    assert rc == want, (rc, msg)
    assert zero
    if text:
        assert text in msg, msg


def test_a_32_bit_column_passes_the_same_checks(program):
    """The checks read the offsets in the column's own width: a good int32 column gets past
    them (to the device, or to ROGTK_E_NODEVICE without one)."""
    rc, msg, _ = _fuzzy_call("rogtk_fuzzy_replace_host", program, col=dict(offsets=_p(_OFF32), ow=4))
    assert rc == (_lib.ROGTK_OK if _lib.device_count() else _lib.ROGTK_E_NODEVICE), msg
