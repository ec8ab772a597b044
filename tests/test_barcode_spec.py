"""CPU tests of the cell-barcode correction spec: the two plain-Python
restatements of tests/barcode_spec.py against the hand-derived known answer and against each
other, the invariances, the declared symbols, and every argument error of the Python layer
(all raised before the library is called, so without a GPU)."""
import os
import re

import numpy as np
import pyarrow as pa
import pytest

import barcode_spec as B
from rogtk_amd import _lib, barcode, plugin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESTATEMENTS = [B.correct_dict, B.correct_brute]


@pytest.mark.parametrize("fn", RESTATEMENTS)
@pytest.mark.parametrize("mode", list(B.KNOWN))
def test_known_answer(fn, mode):
    ambiguous, caller = mode
    index, status, totals, counts = B.KNOWN[mode]
    assert len(B.KNOWN_ROWS) == 21
    got = fn(B.KNOWN_ROWS, B.KNOWN_WHITELIST, ambiguous, B.KNOWN_CALLER_COUNTS if caller else None)
    assert got.index == index
    assert got.status == status
    assert got.totals == totals
    assert got.exact_counts == B.KNOWN_EXACT_COUNTS
    assert got.counts == counts
    assert got.corrected == [B.KNOWN_WHITELIST[w] if s <= 1 else None for w, s in zip(index, status)]


def test_known_answer_rows_named_in_the_spec():
    got = B.correct_dict(B.KNOWN_ROWS, B.KNOWN_WHITELIST)
    by_row = {r: (i, s) for r, i, s in zip(B.KNOWN_ROWS, got.index, got.status)}
    assert by_row[b"AAAC"] == (1, B.CORRECTED) and by_row[b"ACGA"] == (0, B.CORRECTED)
    assert by_row[b"TTTN"] == (3, B.CORRECTED) and by_row[b"AAAN"] == (1, B.CORRECTED)
    assert by_row[b"ACGt"] == (0, B.CORRECTED) and by_row[b"CCCA"] == (B.NO_INDEX, B.AMBIGUOUS)
    for r in (b"NCGN", b"GGCC", b"ACG", b"acgt"):
        assert by_row[r] == (B.NO_INDEX, B.NO_MATCH)
    assert by_row[None] == (B.NO_INDEX, B.NULL)


def test_restatements_agree_on_random_cases():
    rng = np.random.default_rng(20240)
    seen = set()
    for _ in range(200):
        rows, wl = B.random_case(rng)
        prior = [int(x) for x in rng.integers(0, 3, len(wl))] if rng.integers(0, 3) == 0 else None
        for ambiguous in ("counts", "reject"):
            a = B.correct_dict(rows, wl, ambiguous, prior)
            b = B.correct_brute(rows, wl, ambiguous, prior)
            assert a == b
            assert sum(a.totals) == len(rows)
            assert sum(a.counts) == a.totals[B.EXACT] + a.totals[B.CORRECTED]
            assert sum(a.exact_counts) == a.totals[B.EXACT]
            seen.update(a.status)
    assert seen == {0, 1, 2, 3, 4}


def test_shuffling_rows_or_whitelist_only_relabels():
    rng = np.random.default_rng(7)
    for _ in range(20):
        rows, wl = B.random_case(rng, n=50)
        base = B.correct_dict(rows, wl)
        p = rng.permutation(len(rows))
        shuf = B.correct_dict([rows[i] for i in p], wl)
        assert shuf.index == [base.index[i] for i in p] and shuf.status == [base.status[i] for i in p]
        assert (shuf.counts, shuf.exact_counts, shuf.totals) == (base.counts, base.exact_counts, base.totals)
        q = rng.permutation(len(wl))  # new position k holds old entry q[k]
        new_of_old = {int(old): k for k, old in enumerate(q)}
        re_wl = B.correct_dict(rows, [wl[i] for i in q])
        assert re_wl.status == base.status and re_wl.corrected == base.corrected
        assert re_wl.index == [new_of_old[w] if w != B.NO_INDEX else w for w in base.index]
        assert re_wl.counts == [base.counts[i] for i in q]
        assert re_wl.totals == base.totals


SYMBOLS = ["rogtk_barcode_whitelist_create", "rogtk_barcode_whitelist_free", "rogtk_barcode_whitelist_info",
           "rogtk_barcode_correct_dev", "rogtk_barcode_correct_host", "rogtk_barcode_count_dev",
           "rogtk_barcode_count_host", "rogtk_barcode_set_probe"]


def test_symbols_are_declared():
    header = open(os.path.join(ROOT, "include", "rogtk_hip.h")).read()
    declared = {**_lib.SIGNATURES, **_lib.VOID_SIGNATURES}
    lib = _lib.hip()
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\(", header), s
        assert s in declared, s
        assert hasattr(lib, s), s
    for name, value in (("EXACT", 0), ("CORRECTED", 1), ("AMBIGUOUS", 2), ("NO_MATCH", 3), ("NULL", 4)):
        assert re.search(rf"#define ROGTK_BC_{name} {value}\b", header)
    assert "barcode_correct_expr" in plugin.EXPRESSIONS
    assert barcode.STATUS == ("exact", "corrected", "ambiguous", "no_match", "null")


def test_plugin_field_is_uint32():
    f = plugin.call_plugin_field("barcode_correct_expr", [pa.field("cbc", pa.string()), pa.field("wl", pa.string())],
                                 {"ambiguous": "reject"})
    assert f.name == "cbc" and f.type == pa.uint32()


@pytest.mark.parametrize("whitelist,row", [
    ([], None),                                  # empty
    (["ACGT", "ACG"], 1),                        # mixed lengths
    (["ACGT", "AAAA", "ACGN"], 2),               # another byte
    (["ACGT", "acgt"], 1),                       # lower case
    (["ACGT", None, "AAAA"], 1),                 # a null
    ([b"ACGT", b"AC\x00T"], 1),                  # a NUL byte
    (["ACGT", "AAAA", "TTTT", "AAAA", "ACGT"], 3),  # duplicates: the first row that repeats one
    ([""], 0),                                   # L = 0
    (["A" * 33], 0),                             # L = 33
])
def test_whitelist_refusals(whitelist, row):
    with pytest.raises(ValueError) as e:
        barcode.BarcodeWhitelist(whitelist)
    if row is not None:
        assert f"row {row} " in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        barcode.barcode_correct(["ACGT"], whitelist)


class _NoDevice(barcode.BarcodeWhitelist):
    """The argument checks of correct / count alone: a whitelist object without a device handle."""

    def __init__(self, W):
        self.size, self.barcode_len, self._h = W, 4, None


def test_correct_argument_errors():
    wl = _NoDevice(3)
    with pytest.raises(ValueError, match="ambiguous"):
        wl.correct(["ACGT"], ambiguous="majority")
    with pytest.raises(ValueError, match="ambiguous"):
        barcode.barcode_correct(["ACGT"], wl, ambiguous="")
    with pytest.raises(ValueError, match="shape"):
        wl.correct(["ACGT"], counts=np.zeros(4, np.uint32))
    with pytest.raises(ValueError, match="integer"):
        wl.correct(["ACGT"], counts=np.zeros(3, np.float64))
    with pytest.raises(ValueError, match=r"0\.\.2\^32-1"):
        wl.correct(["ACGT"], counts=np.array([1, -1, 0]))
    with pytest.raises(ValueError, match=r"0\.\.2\^32-1"):
        wl.correct(["ACGT"], counts=np.array([1, 2**32, 0], dtype=np.int64))
    with pytest.raises(ValueError, match="nulls"):
        wl.correct(["ACGT"], counts=pa.array([1, None, 0], type=pa.uint32()))
    with pytest.raises(ValueError, match="into"):
        wl.count(["ACGT"], into=np.zeros(3, np.int64))
    with pytest.raises(ValueError, match="into"):
        wl.count(["ACGT"], into=np.zeros(2, np.uint32))


def test_plugin_argument_errors_come_before_device_work():
    col, wl = pa.array(["ACGT"]), pa.array(["ACGT", "AAAA"])
    with pytest.raises(_lib.RogtkError, match="two input series"):
        plugin.call_plugin("barcode_correct_expr", [col])
    with pytest.raises(_lib.RogtkError, match="ambiguous"):
        plugin.call_plugin("barcode_correct_expr", [col, wl], {"ambiguous": "maybe"})
    with pytest.raises(_lib.RogtkError, match="row 1 "):
        plugin.call_plugin("barcode_correct_expr", [col, pa.array(["ACGT", "ACG"])])
    with pytest.raises(_lib.RogtkError, match="String"):
        plugin.call_plugin("barcode_correct_expr", [col, pa.array([1, 2])])
