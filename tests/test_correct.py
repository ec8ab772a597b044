"""UMI correction, CPU side: the spec's known answer through the pure-Python
restatement (tests/correct_spec.py), the exported symbols, the plugin expression's field
and kwargs, and the argument errors, which are all reported before any device work."""
import ctypes
import subprocess

import numpy as np
import pyarrow as pa
import pytest

import rogtk_amd as rg
from correct_spec import KNOWN_ROWS, KNOWN_TABLE, restate
from rogtk_amd import _lib, plugin

C_SYMBOLS = ["rogtk_cluster_summary_temp_bytes", "rogtk_cluster_summary_packed", "rogtk_cluster_correct_packed",
             "rogtk_cluster_summary_set_method", "rogtk_cluster_summary_dev", "rogtk_cluster_representatives_fill",
             "rogtk_umi_correct_dev", "rogtk_umi_correct_host", "rogtk_cluster_summary_host", "rogtk_u32_result_free",
             "_polars_plugin_umi_correct_expr", "_polars_plugin_field_umi_correct_expr"]


def test_restatement_reproduces_the_known_answer():
    ids, k, table, corrected = restate(KNOWN_ROWS, 4, 1)
    assert k == 7
    assert table == KNOWN_TABLE
    assert corrected == [None if x is None else KNOWN_TABLE[c][0] for x, c in zip(KNOWN_ROWS, ids)]
    # what each case shows
    assert corrected[KNOWN_ROWS.index(b"AAAT")] == b"AAAA"    # count tie: the smaller code
    assert corrected[KNOWN_ROWS.index(b"GGGN")] == b"GGGT"    # count tie: regular first (bytes: GGGN)
    assert corrected[KNOWN_ROWS.index(b"TTTT")] == b"TTTN"    # count wins over regular
    assert corrected[KNOWN_ROWS.index(b"AAAAC")] == b"AAAAA"  # irregular-only, another length
    assert sum(t[1] for t in table) == sum(x is not None for x in KNOWN_ROWS)
    assert sum(t[2] for t in table) == len({x for x in KNOWN_ROWS if x is not None})


def test_restatement_exact_mode():
    ids, k, table, corrected = restate(KNOWN_ROWS, 4, 0)
    assert k == 14
    assert corrected == KNOWN_ROWS
    assert all(t[2] == 1 for t in table)


def test_library_exports_the_correction_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.HIP_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    missing = [s for s in C_SYMBOLS if s not in have]
    assert not missing, missing
    bound = set(_lib.SIGNATURES) | set(_lib.VOID_SIGNATURES)
    assert not [s for s in C_SYMBOLS if s.startswith("rogtk_") and s not in bound]


def test_expression_is_registered():
    assert "umi_correct_expr" in plugin.EXPRESSIONS
    assert hasattr(rg, "umi_correct") and hasattr(rg, "umi_cluster_summary")
    assert hasattr(rg.UmiNamespace, "correct")


@pytest.mark.parametrize("typ", [pa.string(), pa.large_string(), pa.string_view()])
def test_plugin_field_is_a_string_with_the_inputs_name(typ):
    f = plugin.call_plugin_field("umi_correct_expr", [pa.field("umi", typ)], {"umi_len": 12, "max_distance": 1})
    assert f.name == "umi"
    assert f.type == pa.string_view()  # polars' String


@pytest.mark.parametrize("kwargs,text", [
    ({"umi_len": 12, "max_distance": 0}, "max_distance=0\numi_len=12\n"),
    ({"umi_len": 12}, "umi_len=12\n"),
    ({"max_distance": 1}, "max_distance=1\n"),
    (None, ""),
])
def test_kwargs_pickle_parses(kwargs, text):
    assert plugin.kwargs_as_parsed(kwargs) == text


def _col(items):
    from rogtk_amd.columns import one_chunk

    ch = one_chunk(pa.array(items, type=pa.large_binary()))
    return ch, ch.desc()


def test_max_distance_2_is_unsupported():
    with pytest.raises(_lib.RogtkError) as e:
        rg.umi_correct(KNOWN_ROWS, 4, 2)
    assert e.value.code == _lib.ROGTK_E_UNSUPPORTED
    with pytest.raises(_lib.RogtkError) as e:
        rg.col(KNOWN_ROWS).umi.correct(max_distance=2)
    assert e.value.code == _lib.ROGTK_E_UNSUPPORTED
    with pytest.raises(_lib.RogtkError) as e:
        plugin.call_plugin("umi_correct_expr", [pa.array(["ACGT", "ACGA"])], {"max_distance": 2})
    assert "max_distance 2" in str(e.value)
    lib = _lib.hip()
    nk = ctypes.c_int64(0)
    assert lib.rogtk_umi_correct_dev(None, None, None, 0, 4, 2, None, ctypes.byref(nk), None,
                                     None) == _lib.ROGTK_E_UNSUPPORTED


def test_null_outputs_are_invalid():
    lib = _lib.hip()
    ch, desc = _col(KNOWN_ROWS)
    cid = np.zeros(ch.n, np.uint32)
    cor, rep = _lib.StrResult(), _lib.StrResult()
    nr, nd = _lib.U32Result(), _lib.U32Result()
    nk = ctypes.c_int64(0)
    args = [ctypes.byref(cor), ctypes.byref(rep), ctypes.byref(nr), ctypes.byref(nd)]
    for hole in range(4):
        a = list(args)
        a[hole] = None
        rc = lib.rogtk_umi_correct_host(ctypes.byref(desc), 4, 1, cid.ctypes.data, *a, ctypes.byref(nk), None)
        assert rc == _lib.ROGTK_E_INVALID, hole
    assert lib.rogtk_umi_correct_host(ctypes.byref(desc), 4, 1, None, *args, ctypes.byref(nk),
                                      None) == _lib.ROGTK_E_INVALID
    for hole in range(3):
        a = list(args[1:])
        a[hole] = None
        assert lib.rogtk_cluster_summary_host(ctypes.byref(desc), 4, cid.ctypes.data, 1, *a) == _lib.ROGTK_E_INVALID
    one = ctypes.c_int64(0)
    assert lib.rogtk_cluster_summary_dev(None, None, None, 0, 4, None, 0, None, None, None, None, ctypes.byref(one),
                                         None) == _lib.ROGTK_E_INVALID


def test_ids_past_n_clusters_are_invalid():
    rows = [b"ACGT", None, b"ACGA"]
    with pytest.raises(_lib.RogtkError) as e:
        rg.umi_cluster_summary(rows, [0, 0, 1], n_clusters=1)
    assert e.value.code == _lib.ROGTK_E_INVALID and "cluster_id[2]" in str(e.value)
    with pytest.raises(_lib.RogtkError) as e:  # the id of a null row is ignored, the others are not
        rg.umi_cluster_summary(rows, [7, 9, 0], n_clusters=7)
    assert e.value.code == _lib.ROGTK_E_INVALID and "cluster_id[0]" in str(e.value)
    with pytest.raises(ValueError):
        rg.umi_cluster_summary(rows, [0, 0])


def test_packed_entries_reject_what_they_do_not_support():
    lib = _lib.hip()
    b = ctypes.c_int64(0)
    assert lib.rogtk_cluster_summary_temp_bytes(10, 17, 1, ctypes.byref(b)) == _lib.ROGTK_E_UNSUPPORTED
    assert lib.rogtk_cluster_summary_temp_bytes(1 << 31, 12, 1, ctypes.byref(b)) == _lib.ROGTK_E_UNSUPPORTED
    assert lib.rogtk_cluster_summary_packed(None, None, 10, 0, None, 1, None, None, None, None, 0,
                                            None) == _lib.ROGTK_E_UNSUPPORTED
    assert lib.rogtk_cluster_summary_packed(None, None, 10, 12, None, 1, None, None, None, None, 0,
                                            None) == _lib.ROGTK_E_INVALID
    assert lib.rogtk_cluster_correct_packed(None, None, 10, None, 1, None, None) == _lib.ROGTK_E_INVALID
    assert lib.rogtk_cluster_summary_set_method(2) == _lib.ROGTK_E_INVALID
    assert lib.rogtk_cluster_summary_set_method(0) == _lib.ROGTK_OK
