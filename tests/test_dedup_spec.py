"""The UMI deduplication spec without a GPU: the two restatements of
tests/dedup_spec.py against each other, the invariant under row permutations, the exported
symbols, and every refusal that the C ABI and the Python layer make before any device work."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pyarrow as pa
import pytest

import dedup_spec as S
import rogtk_amd as rg
from rogtk_amd import _lib, dedup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_SYMBOLS = ("rogtk_cluster_best_temp_bytes", "rogtk_cluster_best_rows", "rogtk_cluster_best_rows_host")


def test_known_case():
    #          row  0  1  2  3           4  5  6  7
    ids = np.array([1, 0, 1, 0xFFFFFFFF, 3, 1, 7, 0], dtype=np.uint32)
    score = np.array([5, 2, 9, 99, 0, 9, 50, 2], dtype=np.uint32)
    for f in (S.best_dict, S.best_lexsort):
        d = f(ids, score, 4)
        assert d.best_row.tolist() == [1, 2, -1, 4]  # id 0: tie, the smaller row; id 2: no rows
        assert d.best_score.tolist() == [2, 9, 0, 0]
        assert d.n_reads.tolist() == [2, 3, 0, 1]  # rows 3 (null) and 6 (id >= 4) are not counted
        assert d.keep.tolist() == [False, True, True, False, True, False, False, False]
        assert d.keep_words.tolist() == [0b10110]
        assert d.rows.tolist() == [1, 2, 4] and d.n_kept == 3
        d = f(ids, None, 4)
        assert d.best_row.tolist() == [1, 0, -1, 4] and d.best_score.tolist() == [0, 0, 0, 0]


def test_the_two_restatements_agree_on_random_cases():
    seen = {"ties": 0, "skipped": 0, "empty": 0, "no_score": 0}
    for seed in range(400):
        ids, score, k = S.random_case(seed)
        a, b = S.best_dict(ids, score, k), S.best_lexsort(ids, score, k)
        assert S.same(a, b), seed
        assert a.n_kept == int(np.count_nonzero(a.n_reads)) == int(np.count_nonzero(a.best_row >= 0))
        assert int(a.n_reads.sum()) == int(np.count_nonzero(ids.astype(np.int64) < k))
        assert S.unpack_words(a.keep_words, ids.size)[ids.size:].sum() == 0
        live = ids.astype(np.int64) < k
        seen["skipped"] += int((~live).any())
        seen["empty"] += int((a.best_row == -1).any())
        seen["no_score"] += int(score is None)
        if score is not None and live.any():
            pairs = set(zip(ids[live].tolist(), score[live].tolist()))
            seen["ties"] += int(len(pairs) < int(live.sum()))
    assert all(v >= 20 for v in seen.values()), seen


def test_row_permutations():
    """The kept multiset of (id, score) does not depend on the order of the rows; and where the
    scores of a cluster's rows all differ, the keep mask moves with the rows."""
    for seed in range(100):
        ids, score, k = S.random_case(seed)
        n = ids.size
        rng = np.random.default_rng(1000 + seed)
        perm = rng.permutation(n)
        sc = np.zeros(n, np.uint32) if score is None else score
        a = S.best_dict(ids, sc, k)
        b = S.best_dict(ids[perm], sc[perm], k)
        kept_a = sorted(zip(ids[a.rows].tolist(), sc[a.rows].tolist()))
        kept_b = sorted(zip(ids[perm][b.rows].tolist(), sc[perm][b.rows].tolist()))
        assert kept_a == kept_b, seed
        assert np.array_equal(a.n_reads, b.n_reads) and np.array_equal(a.best_score, b.best_score)
        distinct = rng.permutation(n).astype(np.uint32)  # no two rows share a score
        a = S.best_dict(ids, distinct, k)
        b = S.best_dict(ids[perm], distinct[perm], k)
        assert np.array_equal(b.keep, a.keep[perm]), seed


def test_library_exports_the_dedup_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.DEDUP_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not [s for s in C_SYMBOLS if s not in have]
    assert not [s for s in C_SYMBOLS if s not in _lib.SIGNATURES]
    header = open(os.path.join(ROOT, "include", "rogtk_dedup.h")).read()  # the library's own header
    assert not [s for s in C_SYMBOLS if s + "(" not in header]
    assert rg.umi_dedup is dedup.umi_dedup and rg.cluster_best_rows is dedup.cluster_best_rows
    assert hasattr(rg.col(["ACGT"]).umi, "dedup")


def test_geometry_is_exposed():
    g = dedup.geometry()
    assert g["select_tile"] > 0 and g["select_tile"] % 256 == 0
    assert g["keep_tile"] > 0 and g["keep_tile"] % 64 == 0
    assert g["slots"] & (g["slots"] - 1) == 0 and g["probes"] >= 1


def test_temp_bytes_is_the_arithmetic_of_the_design():
    """the u64 votes of every cluster, then the popcount and the offset of every keep
    tile, each piece rounded up to 256 bytes (an empty piece takes 256)."""
    tile = dedup.geometry()["keep_tile"]
    al = lambda b: (max(b, 1) + 255) // 256 * 256
    lib = _lib.dedup()
    b = ctypes.c_int64(0)
    for n, k in ((0, 0), (1, 1), (tile, 7), (tile + 1, 7), (10_000_000, 93_790)):
        tiles = (n + tile - 1) // tile
        assert lib.rogtk_cluster_best_temp_bytes(n, k, ctypes.byref(b)) == _lib.ROGTK_OK
        assert b.value == al(8 * k) + 2 * al(4 * tiles), (n, k)


def _refused(lib, fn, *args, word):
    """The call returns ROGTK_E_INVALID and the message names what was wrong."""
    assert getattr(lib, fn)(*args) == _lib.ROGTK_E_INVALID, (fn, word)
    message = _lib.hip().rogtk_last_error().decode()  # one error string for both libraries
    assert word in message, (fn, word, message)


def test_every_refusal_comes_before_any_device_work():
    """Null pointers, or the address of a host scratch block where a pointer has to be present:
    nothing here reaches a device, because every call is refused first."""
    lib = _lib.dedup()
    b = ctypes.c_int64(0)
    big, huge = 1 << 31, (1 << 32) - 1
    _refused(lib, "rogtk_cluster_best_temp_bytes", -1, 4, ctypes.byref(b), word="n -1")
    _refused(lib, "rogtk_cluster_best_temp_bytes", big, 4, ctypes.byref(b), word="n 2147483648")
    _refused(lib, "rogtk_cluster_best_temp_bytes", 10, -1, ctypes.byref(b), word="n_clusters -1")
    _refused(lib, "rogtk_cluster_best_temp_bytes", 10, huge, ctypes.byref(b), word="n_clusters 4294967295")
    _refused(lib, "rogtk_cluster_best_temp_bytes", 10, 4, None, word="NULL bytes")
    assert lib.rogtk_cluster_best_temp_bytes(10, 4, ctypes.byref(b)) == _lib.ROGTK_OK and b.value > 0
    need = b.value
    assert lib.rogtk_cluster_best_temp_bytes(0, 0, ctypes.byref(b)) == _lib.ROGTK_OK and b.value > 0
    assert lib.rogtk_cluster_best_temp_bytes(big - 1, huge - 1, ctypes.byref(b)) == _lib.ROGTK_OK

    block = (ctypes.c_uint64 * 64)()
    x = ctypes.c_void_p(ctypes.addressof(block))  # "present"; never dereferenced by a refused call
    odd = ctypes.c_void_p(ctypes.addressof(block) + 4)
    hk = ctypes.c_int64(0)

    def dev(ids=x, score=None, n=10, k=4, best_row=x, best_score=None, n_reads=None, keep=x, kept=None, n_kept=None,
            temp=x, temp_bytes=1 << 20, *, word):
        _refused(lib, "rogtk_cluster_best_rows", ids, score, n, k, best_row, best_score, n_reads, keep, kept, n_kept,
                 temp, temp_bytes, None, word=word)

    def host(ids=x, score=None, n=10, k=4, best_row=x, best_score=None, n_reads=None, keep=x, kept=None, n_kept=None,
             *, word):
        _refused(lib, "rogtk_cluster_best_rows_host", ids, score, n, k, best_row, best_score, n_reads, keep, kept,
                 n_kept, word=word)

    for call in (dev, host):
        call(n=-1, word="n -1")
        call(n=big, word="n 2147483648")
        call(k=-1, word="n_clusters -1")
        call(k=huge, word="n_clusters 4294967295")
        call(ids=None, word="cluster_id is NULL")
        call(keep=None, word="keep_bits is NULL")
        call(best_row=None, word="best_row is NULL")
        call(kept=x, n_kept=None, word="kept_rows without n_kept")
        call(kept=None, n_kept=ctypes.byref(hk), word="n_kept without kept_rows")
    # all of them null, as a caller without a device would pass them
    _refused(lib, "rogtk_cluster_best_rows", None, None, 5, 3, None, None, None, None, None, None, None, 0, None,
             word="NULL")
    _refused(lib, "rogtk_cluster_best_rows_host", None, None, 5, 3, None, None, None, None, None, None, word="NULL")
    dev(temp=None, word="temp is NULL")
    dev(temp=odd, word="8-byte aligned")
    dev(temp_bytes=need - 1, word="too small")
    dev(temp_bytes=0, word="too small")
    dev(n=0, k=0, ids=None, best_row=None, keep=None, temp_bytes=0, word="too small")


def test_python_refusals_are_value_errors_before_any_library_call(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "call", no_library)
    monkeypatch.setattr(_lib, "hip", no_library)
    monkeypatch.setattr(_lib, "dedup", no_library)
    ids = np.array([0, 1, 1, 0], dtype=np.uint32)
    bad_scores = [
        np.zeros(3, np.uint32),                                  # another length
        np.zeros(5, np.uint32),
        np.zeros(4, np.float32),                                 # float
        np.array([1, -1, 0, 0], dtype=np.int32),                 # negative
        np.array([1, 1 << 32, 0, 0], dtype=np.int64),            # past u32
        pa.array([1, None, 2, 3], type=pa.uint32()),             # nulls
        pa.array([1.0, 2.0, 3.0, 4.0]),                          # Arrow float
        np.zeros((4, 1), np.uint32),                             # not 1-D
    ]
    for sc in bad_scores:
        with pytest.raises(ValueError):
            rg.cluster_best_rows(ids, sc)
        with pytest.raises(ValueError):
            rg.umi_dedup(["ACGT", "ACGA", "TTTT", None], 4, score=sc)
        with pytest.raises(ValueError):
            rg.col(["ACGT", "ACGA", "TTTT", None]).umi.dedup(4, score=sc)
    for cid in (np.zeros((2, 2), np.uint32), np.zeros((), np.uint32), np.zeros(4, np.float64),
                np.array([0, -1, 0, 0]), np.array([0, 1 << 32, 0, 0])):
        with pytest.raises(ValueError):
            rg.cluster_best_rows(cid)
    with pytest.raises(ValueError):
        rg.cluster_best_rows(ids, n_clusters=(1 << 32) - 1)
    # device tensors: the shared checker's one wording per fault (the table of tests/test_count_spec.py)
    import torch

    from count_spec import bad_u32_tensors

    t = torch.tensor([0, 1, 1, 0], dtype=torch.int32)
    for bad, wording in bad_u32_tensors(ids):
        with pytest.raises(ValueError, match="score " + wording):
            rg.cluster_best_rows(t, bad, 2)
    for bad, wording in bad_u32_tensors(ids)[1:5]:
        with pytest.raises(ValueError, match="cluster_id " + wording):
            rg.cluster_best_rows(bad, None, 2)
        with pytest.raises(ValueError, match="cluster_id " + wording):
            rg.cluster_best_rows(bad, bad, 2)
