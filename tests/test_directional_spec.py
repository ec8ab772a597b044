"""Directional UMI clustering, CPU side: the two pure-Python restatements of
the spec (tests/directional_spec.py) against the known answer, against each other and against
the transitive clusters; the exported symbols; the argument errors, which are all reported
before any device work."""
import ctypes
import os
import subprocess

import numpy as np
import pyarrow as pa
import pytest

import rogtk_amd as rg
from correct_spec import is_regular
from directional_spec import (KNOWN_GROUPS, KNOWN_ROWS, KNOWN_TABLE, code, ids_of, random_families, regular_counts,
                              restate, roots_bfs, roots_fixed_point)
from oracle import pyoracle as P
from rogtk_amd import _lib, plugin

C_SYMBOLS = ["rogtk_directional_temp_bytes", "rogtk_directional_codes", "rogtk_directional_last_rounds",
             "rogtk_umi_cluster_directional_dev", "rogtk_umi_correct_directional_dev",
             "rogtk_umi_cluster_directional_host", "rogtk_umi_correct_directional_host"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("roots_fn", [roots_bfs, roots_fixed_point])
def test_restatements_reproduce_the_known_answer(roots_fn):
    ids, k, table, corrected = restate(KNOWN_ROWS, 4, roots_fn)
    assert k == 8
    assert table == KNOWN_TABLE
    assert corrected == [None if x is None else KNOWN_TABLE[c][0] for x, c in zip(KNOWN_ROWS, ids)]
    at = {x: c for x, c in zip(KNOWN_ROWS, corrected)}
    assert at[b"ATTT"] == b"AAAA"                         # chain of depth 3
    assert at[b"CCCC"] == b"CCCC" and at[b"CCCG"] == b"CCCG"  # blocked pair: 6 < 2 * 6 - 1
    assert at[b"ACGG"] == b"ACAC"                         # reached through ACAG, not TCGG's (60 < 100)
    assert at[b"GGGA"] == b"AAAA"                         # the plateau hangs below AAAA x10 -> GAAA
    assert at[b"TTTG"] == b"TCGG" == at[b"TTGG"]          # TCGG x60 -> TTGG x8 -> TTTG
    assert at[b"ACGN"] == b"ACGN" and at[b"ACGTA"] == b"ACGTA" and at[None] is None
    assert ids[KNOWN_ROWS.index(b"ACGN")] == 6 and ids[KNOWN_ROWS.index(b"ACGTA")] == 7  # after the regular ones
    # the transitive method joins the blocked pair (and more)
    _, kt = P.py_cluster_bruteforce(KNOWN_ROWS, 4, 1)
    assert kt < k


@pytest.mark.parametrize("name", sorted(KNOWN_GROUPS))
def test_each_group_alone(name):
    rows, want = KNOWN_GROUPS[name]
    counts = regular_counts(rows, 4)
    assert roots_bfs(counts) == want
    assert roots_fixed_point(counts) == want


def small_column(rng):
    """Up to 400 rows: a few parents with skewed weights, substitutions, nulls and irregular rows."""
    L = int(rng.choice([1, 2, 4, 6]))
    n = int(rng.integers(1, 401))
    parents = rng.integers(0, 4, size=(int(rng.integers(1, 9)), L))
    weights = 1.0 / np.arange(1, len(parents) + 1) ** 2
    pick = rng.choice(len(parents), size=n, p=weights / weights.sum())
    reads = parents[pick]
    hit = rng.random(reads.shape) < 0.12
    reads = np.where(hit, rng.integers(0, 4, size=reads.shape), reads)
    rows = [bytes(r) for r in np.frombuffer(b"ACGT", np.uint8)[reads]]
    for i in range(n):
        u = rng.random()
        if u < 0.04:
            rows[i] = None
        elif u < 0.07:
            rows[i] = rows[i][:-1] + b"N"
        elif u < 0.09:
            rows[i] = rows[i] + b"A"
        elif u < 0.10:
            rows[i] = rows[i].lower()
    return rows, L


def test_restatements_agree_on_random_small_columns():
    rng = np.random.default_rng(4)
    for case in range(200):
        rows, L = small_column(rng)
        counts = regular_counts(rows, L)
        ra, rb = roots_bfs(counts), roots_fixed_point(counts)
        assert ra == rb, case
        ids, k, table, corrected = restate(rows, L)
        assert (ids, k) == ids_of(rows, L, ra), case
        # every directional cluster lies in one transitive cluster
        tids, kt = P.py_cluster_bruteforce(rows, L, 1)
        inside = {}
        for d, t in zip(ids, tids):
            if d is not None:
                assert inside.setdefault(d, t) == t, case
        assert k >= kt, case
        # the summary vote names the root; the root has the most rows, ties to the smaller code
        for x, c in zip(rows, ids):
            if x is not None and is_regular(x, L):
                assert table[c][0] == rb[x], case
        for v, r in rb.items():
            assert (counts[r], -code(r)) >= (counts[v], -code(v)), case
        assert sum(t[1] for t in table) == sum(x is not None for x in rows)
        assert sum(t[2] for t in table) == len({x for x in rows if x is not None})


def test_random_families_differ_from_the_transitive_clusters():
    rows = random_families()
    assert 15_000 < len(rows) < 25_000
    _, k, _, _ = restate(rows, 8)
    _, _, kt, _ = P.umi_cluster(P.StrCol.from_list(rows), 8, 1)
    assert k > kt, (k, kt)


def test_library_exports_the_directional_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.HIP_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not [s for s in C_SYMBOLS if s not in have]
    assert not [s for s in C_SYMBOLS if s not in _lib.SIGNATURES]
    header = open(os.path.join(ROOT, "include", "rogtk_hip.h")).read()
    assert not [s for s in C_SYMBOLS if s + "(" not in header]


def test_unknown_method_is_a_value_error():
    for call in (lambda: rg.umi_cluster(KNOWN_ROWS, 4, 1, method="nonsense"),
                 lambda: rg.umi_correct(KNOWN_ROWS, 4, 1, method="nonsense"),
                 lambda: rg.col(KNOWN_ROWS).umi.cluster(4, method="nonsense"),
                 lambda: rg.col(KNOWN_ROWS).umi.correct(4, method="nonsense")):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(_lib.RogtkError) as e:
        plugin.call_plugin("umi_correct_expr", [pa.array(["ACGT", "ACGA"])], {"method": "nonsense"})
    assert "method" in str(e.value)


def test_kwargs_pickle_carries_the_method():
    assert plugin.kwargs_as_parsed({"umi_len": 4, "method": "directional"}) == "method='directional'\numi_len=4\n"


def test_max_distance_2_is_unsupported():
    with pytest.raises(_lib.RogtkError) as e:
        rg.umi_correct(KNOWN_ROWS, 4, 2, method="directional")
    assert e.value.code == _lib.ROGTK_E_UNSUPPORTED
    with pytest.raises(_lib.RogtkError) as e:
        rg.umi_cluster(KNOWN_ROWS, 4, 2, method="directional")
    assert e.value.code == _lib.ROGTK_E_UNSUPPORTED
    with pytest.raises(_lib.RogtkError) as e:
        plugin.call_plugin("umi_correct_expr", [pa.array(["ACGT", "ACGA"])],
                           {"max_distance": 2, "method": "directional"})
    assert "max_distance 2" in str(e.value)


def test_code_entries_reject_what_they_do_not_support():
    lib = _lib.hip()
    b, k, r = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    assert lib.rogtk_directional_temp_bytes(10, 0, ctypes.byref(b)) == _lib.ROGTK_E_UNSUPPORTED
    assert lib.rogtk_directional_temp_bytes(10, 33, ctypes.byref(b)) == _lib.ROGTK_E_UNSUPPORTED
    assert lib.rogtk_directional_temp_bytes(1 << 31, 12, ctypes.byref(b)) == _lib.ROGTK_E_UNSUPPORTED
    assert lib.rogtk_directional_temp_bytes(10, 12, None) == _lib.ROGTK_E_INVALID
    assert lib.rogtk_directional_codes(None, None, 10, 33, None, None, ctypes.byref(k), ctypes.byref(r), None, 0,
                                       None) == _lib.ROGTK_E_UNSUPPORTED
    assert lib.rogtk_directional_codes(None, None, 10, 12, None, None, ctypes.byref(k), ctypes.byref(r), None, 0,
                                       None) == _lib.ROGTK_E_INVALID
    assert lib.rogtk_directional_codes(None, None, 10, 12, None, None, None, None, None, 0,
                                       None) == _lib.ROGTK_E_INVALID
    assert lib.rogtk_umi_cluster_directional_dev(None, None, None, 5, 4, None, ctypes.byref(k), None,
                                                 None) == _lib.ROGTK_E_INVALID
    assert lib.rogtk_umi_cluster_directional_dev(None, None, None, 1 << 31, 4, None, ctypes.byref(k), None,
                                                 None) == _lib.ROGTK_E_UNSUPPORTED
    assert lib.rogtk_umi_correct_directional_dev(None, None, None, 5, 4, None, ctypes.byref(k), None,
                                                 None) == _lib.ROGTK_E_INVALID
