"""The UMI count matrix spec without a GPU: the two restatements of
tests/count_spec.py against each other, the invariants under row permutations and molecule
relabelling, the key-width arithmetic, the exported symbols, and every refusal that the C ABI
and the Python layer make before any device work."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pyarrow as pa
import pytest

import count_spec as S
import rogtk_amd as rg
from rogtk_amd import _lib, count

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_SYMBOLS = ("rogtk_count_matrix_temp_bytes", "rogtk_count_matrix", "rogtk_count_matrix_host",
             "rogtk_count_matrix_geometry")
NO_ID = S.NO_ID


def test_known_case():
    #               row  0  1  2  3      4  5  6  7  8  9
    cell = np.array([2, 0, 2, NO_ID, 2, 0, 2, 3, 2, 2], dtype=np.uint32)
    feat = np.array([1, 5, 1, 0, 0, 5, 1, 0, 1, 9], dtype=np.uint32)
    mol = np.array([7, 3, 7, 1, 7, 4, 2, 0, 50, 1], dtype=np.uint32)
    for f in (S.count_dict, S.count_lexsort):
        d = f(cell, feat, mol, 4, 6, 10)
        # row 3: null cell; row 8: molecule >= 10; row 9: feature >= 6
        assert d.cell.tolist() == [0, 2, 2, 3] and d.feature.tolist() == [5, 0, 1, 0]
        assert d.n_umis.tolist() == [2, 1, 2, 1]      # molecule 7 counts under (2, 0) and under (2, 1)
        assert d.n_reads.tolist() == [2, 1, 3, 1]
        assert d.totals.tolist() == [4, 7, 6]
        assert d.indptr.tolist() == [0, 1, 1, 3, 4]   # cell 1 is empty
        d = f(cell, feat, mol, 4, 6, 10, capacity=2)
        assert d.cell.tolist() == [0, 2] and d.n_umis.tolist() == [2, 1] and d.n_reads.tolist() == [2, 1]
        assert d.totals.tolist() == [4, 7, 6] and d.indptr.tolist() == [0, 1, 1, 2, 2]
        assert f(cell, feat, mol, 0, 6, 10).totals.tolist() == [0, 0, 0]


def test_the_two_restatements_agree_on_random_cases():
    seen = {"skipped_cell": 0, "skipped_feature": 0, "skipped_molecule": 0, "repeats": 0, "shared": 0, "empty": 0,
            "cut": 0}
    for seed in range(400):
        c, f, m, nc, nf, nm = S.random_case(seed)
        a, b = S.count_dict(c, f, m, nc, nf, nm), S.count_lexsort(c, f, m, nc, nf, nm)
        assert S.same(a, b), seed
        live = (c.astype(np.int64) < nc) & (f.astype(np.int64) < nf) & (m.astype(np.int64) < nm)
        assert int(a.n_reads.sum()) == int(live.sum()) == int(a.totals[1])
        assert int(a.n_umis.sum()) == int(a.totals[2]) and a.cell.size == int(a.totals[0])
        assert (a.n_umis >= 1).all() and (a.n_umis <= a.n_reads).all()
        # indptr against entry_cell
        assert a.indptr[0] == 0 and a.indptr[-1] == a.cell.size and (np.diff(a.indptr) >= 0).all()
        for cc in range(nc):
            assert (a.cell[a.indptr[cc]:a.indptr[cc + 1]] == cc).all()
        pair = a.cell.astype(np.int64) * max(nf, 1) + a.feature
        assert (np.diff(pair) > 0).all()  # ascending, no pair twice
        cap = int(a.totals[0]) // 2
        ca, cb = S.count_dict(c, f, m, nc, nf, nm, cap), S.count_lexsort(c, f, m, nc, nf, nm, cap)
        assert S.same(ca, cb) and np.array_equal(ca.n_umis, a.n_umis[:cap]) and ca.indptr[-1] == cap
        assert np.array_equal(ca.totals, a.totals)
        seen["skipped_cell"] += int((c.astype(np.int64) >= nc).any())
        seen["skipped_feature"] += int((f.astype(np.int64) >= nf).any())
        seen["skipped_molecule"] += int((m.astype(np.int64) >= nm).any())
        seen["repeats"] += int(int(a.totals[2]) < int(a.totals[1]))
        triples = {(x, y, z) for x, y, z in zip(c[live].tolist(), f[live].tolist(), m[live].tolist())}
        seen["shared"] += int(len({(x, z) for x, _, z in triples}) < len(triples))
        seen["empty"] += int((np.diff(a.indptr) == 0).any())
        seen["cut"] += int(cap < int(a.totals[0]))
    assert all(v >= 20 for v in seen.values()), seen


def test_row_permutations_and_molecule_relabelling():
    for seed in range(100):
        c, f, m, nc, nf, nm = S.random_case(seed)
        rng = np.random.default_rng(5000 + seed)
        a = S.count_dict(c, f, m, nc, nf, nm)
        perm = rng.permutation(c.size)
        assert S.same(a, S.count_dict(c[perm], f[perm], m[perm], nc, nf, nm)), seed
        assert S.same(a, S.count_lexsort(c[perm], f[perm], m[perm], nc, nf, nm)), seed
        relabel = rng.permutation(nm).astype(np.uint32)  # a bijection of 0..n_molecules-1; skipped ids stay
        m2 = m.copy()
        inside = m.astype(np.int64) < nm
        m2[inside] = relabel[m[inside]]
        assert S.same(a, S.count_dict(c, f, m2, nc, nf, nm)), seed


def test_width_arithmetic():
    assert [S.bit_width(v) for v in (0, 1, 2, 3, 4, 255, 256, (1 << 32) - 1)] == [0, 1, 2, 2, 3, 8, 9, 32]
    assert S.key_bits(1, 1, 1) == 1 and S.key_bits(5, 1, 1) == 3 and S.key_bits(4, 4, 4) == 3 + 2 + 2
    lib = _lib.count()
    b = ctypes.c_int64(0)
    nf, nm = 1 << 16, 1 << 24
    assert S.key_bits((1 << 24) - 1, nf, nm) == 64
    assert lib.rogtk_count_matrix_temp_bytes(10, (1 << 24) - 1, nf, nm, 10, ctypes.byref(b)) == _lib.ROGTK_OK
    assert b.value > 0
    assert S.key_bits(1 << 24, nf, nm) == 65
    assert lib.rogtk_count_matrix_temp_bytes(10, 1 << 24, nf, nm, 10, ctypes.byref(b)) == _lib.ROGTK_E_UNSUPPORTED
    message = _lib.hip().rogtk_last_error().decode()
    assert "65 bits" in message and "cells 25" in message and "features 16" in message and "molecules 24" in message
    # the widest sizes of two fields leave none for the third but its zero-width form
    top = (1 << 32) - 1
    assert lib.rogtk_count_matrix_temp_bytes(10, top, top, 1, 10, ctypes.byref(b)) == _lib.ROGTK_OK
    assert lib.rogtk_count_matrix_temp_bytes(10, top, top, 2, 10, ctypes.byref(b)) == _lib.ROGTK_E_UNSUPPORTED
    # a size of 0: no entries whatever the other widths
    assert lib.rogtk_count_matrix_temp_bytes(10, top, top, 0, 10, ctypes.byref(b)) == _lib.ROGTK_OK


def test_library_exports_the_count_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.COUNT_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not [s for s in C_SYMBOLS if s not in have]
    assert not [s for s in C_SYMBOLS if s not in _lib.SIGNATURES]
    header = open(os.path.join(ROOT, "include", "rogtk_count.h")).read()  # the library's own header
    assert not [s for s in C_SYMBOLS if s + "(" not in header]
    assert "rogtk_count_matrix" not in open(os.path.join(ROOT, "include", "rogtk_hip.h")).read()
    assert rg.count_matrix is count.count_matrix and rg.umi_count is count.umi_count
    assert rg.CountMatrix is count.CountMatrix


def test_geometry_is_exposed():
    g = count.geometry()
    assert g["tile"] > 0 and g["tile"] % 64 == 0
    assert g["scan_block"] > 0 and g["scan_block"] % 64 == 0


def _refused(lib, fn, *args, word, code=_lib.ROGTK_E_INVALID):
    """The call returns its code and the message names what was wrong."""
    assert getattr(lib, fn)(*args) == code, (fn, word)
    message = _lib.hip().rogtk_last_error().decode()  # one error string for the libraries
    assert word in message, (fn, word, message)


def test_every_refusal_comes_before_any_device_work():
    """Null pointers, or the address of a host scratch block where a pointer has to be present:
    nothing here reaches a device, because every call is refused first."""
    lib = _lib.count()
    b = ctypes.c_int64(0)
    big, huge = 1 << 31, 1 << 32
    tb = lambda n=10, nc=4, nf=4, nm=4, cap=10, out=ctypes.byref(b), **kw: _refused(
        lib, "rogtk_count_matrix_temp_bytes", n, nc, nf, nm, cap, out, **kw)
    tb(n=-1, word="n -1")
    tb(n=big, word="n 2147483648")
    tb(nc=-1, word="n_cells -1")
    tb(nc=huge, word="n_cells 4294967296")
    tb(nf=-1, word="n_features -1")
    tb(nf=huge, word="n_features 4294967296")
    tb(nm=-1, word="n_molecules -1")
    tb(nm=huge, word="n_molecules 4294967296")
    tb(cap=-1, word="capacity -1")
    tb(out=None, word="NULL bytes")
    tb(nc=1 << 30, nf=1 << 30, nm=1 << 30, word="91 bits", code=_lib.ROGTK_E_UNSUPPORTED)
    assert lib.rogtk_count_matrix_temp_bytes(10, 4, 4, 4, 10, ctypes.byref(b)) == _lib.ROGTK_OK and b.value > 0
    need = b.value
    assert lib.rogtk_count_matrix_temp_bytes(0, 0, 0, 0, 0, ctypes.byref(b)) == _lib.ROGTK_OK and b.value > 0

    block = (ctypes.c_uint64 * 64)()
    x = ctypes.c_void_p(ctypes.addressof(block))  # "present"; never dereferenced by a refused call
    odd = ctypes.c_void_p(ctypes.addressof(block) + 4)

    def dev(cell=x, feature=x, molecule=x, n=10, nc=4, nf=4, nm=4, ec=x, ef=x, nu=x, nr=None, cap=10, indptr=None,
            totals=x, temp=x, temp_bytes=1 << 20, *, word, code=_lib.ROGTK_E_INVALID):
        _refused(lib, "rogtk_count_matrix", cell, feature, molecule, n, nc, nf, nm, ec, ef, nu, nr, cap, indptr,
                 totals, temp, temp_bytes, None, word=word, code=code)

    def host(cell=x, feature=x, molecule=x, n=10, nc=4, nf=4, nm=4, ec=x, ef=x, nu=x, nr=None, cap=10, indptr=None,
             totals=x, *, word, code=_lib.ROGTK_E_INVALID):
        _refused(lib, "rogtk_count_matrix_host", cell, feature, molecule, n, nc, nf, nm, ec, ef, nu, nr, cap, indptr,
                 totals, word=word, code=code)

    for call in (dev, host):
        call(n=-1, word="n -1")
        call(n=big, word="n 2147483648")
        call(nc=-1, word="n_cells -1")
        call(nc=huge, word="n_cells 4294967296")
        call(nf=-1, word="n_features -1")
        call(nf=huge, word="n_features 4294967296")
        call(nm=-1, word="n_molecules -1")
        call(nm=huge, word="n_molecules 4294967296")
        call(cell=None, word="cell is NULL")
        call(feature=None, word="feature is NULL")
        call(molecule=None, word="molecule is NULL")
        call(ec=None, word="entry_cell is NULL")
        call(ef=None, word="entry_feature is NULL")
        call(nu=None, word="n_umis is NULL")
        call(totals=None, word="totals is NULL")
        call(nc=1 << 24, nf=1 << 16, nm=1 << 24, word="65 bits", code=_lib.ROGTK_E_UNSUPPORTED)
    dev(cap=-1, word="capacity -1")
    host(cap=-1, ec=None, word="entry_cell is NULL")  # the host entry's default capacity, min(n, cells x features)
    # all of them null, as a caller without a device would pass them
    _refused(lib, "rogtk_count_matrix", None, None, None, 5, 3, 3, 3, None, None, None, None, 5, None, None, None, 0,
             None, word="NULL")
    _refused(lib, "rogtk_count_matrix_host", None, None, None, 5, 3, 3, 3, None, None, None, None, 5, None, None,
             word="NULL")
    dev(temp=None, word="temp is NULL")
    dev(temp=odd, word="8-byte aligned")
    dev(temp_bytes=need - 1, word="too small")
    dev(temp_bytes=0, word="too small")
    dev(n=0, nc=0, nf=0, nm=0, cap=0, cell=None, feature=None, molecule=None, ec=None, ef=None, nu=None,
        temp_bytes=0, word="too small")
    _refused(lib, "rogtk_count_matrix_geometry", None, word="NULL")


def test_python_refusals_are_value_errors_before_any_library_call(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "call", no_library)
    monkeypatch.setattr(_lib, "hip", no_library)
    monkeypatch.setattr(_lib, "count", no_library)
    good = np.array([0, 1, 1, 0], dtype=np.uint32)
    bad_columns = [
        np.zeros(3, np.uint32),                                  # another length
        np.zeros(5, np.uint32),
        np.zeros(4, np.float32),                                 # float
        np.array([1, -1, 0, 0], dtype=np.int32),                 # negative
        np.array([1, 1 << 32, 0, 0], dtype=np.int64),            # past u32
        pa.array([1.0, 2.0, 3.0, 4.0]),                          # Arrow float
        np.zeros((4, 1), np.uint32),                             # not 1-D
    ]
    umis = ["ACGT", "ACGA", "TTTT", None]
    for bad in bad_columns:
        for slot in range(3):
            cols = [good, good, good]
            cols[slot] = bad  # (a first column of another length makes the other two the odd ones)
            with pytest.raises(ValueError):
                rg.count_matrix(*cols)
        with pytest.raises(ValueError):
            rg.umi_count(umis, 4, bad, good, 2, 2)
        with pytest.raises(ValueError):
            rg.umi_count(umis, 4, good, bad, 2, 2)
    with pytest.raises(ValueError):
        rg.count_matrix(np.zeros(3, np.uint32), good, good)
    for sizes in ((1 << 32, 2, 2), (2, 1 << 32, 2), (2, 2, 1 << 32)):
        with pytest.raises(ValueError):
            rg.count_matrix(good, good, good, *sizes)
    with pytest.raises(ValueError, match="rank the"):
        rg.umi_count(umis, 4, good, good, 1 << 16, 1 << 16)  # 2^32 pairs: one more than a u32 key holds
    with pytest.raises(ValueError):
        rg.umi_count(umis, 4, good, good, -1, 2)

    import torch

    t = torch.tensor([0, 1, 1, 0], dtype=torch.int32)
    bad_tensors = S.bad_u32_tensors(good)  # with the one wording of each fault
    for bad, wording in bad_tensors:
        for name, cols in (("feature ", (t, bad, t)), ("molecule ", (t, t, bad))):
            with pytest.raises(ValueError, match=name + wording):
                rg.count_matrix(*cols, 2, 2, 2)
    for bad, wording in bad_tensors[1:5]:
        with pytest.raises(ValueError, match="cell " + wording):
            rg.count_matrix(bad, bad, bad, 2, 2, 2)


def test_to_scipy_and_the_per_cell_sums():
    want = S.count_dict([2, 0, 2, 2, 3], [1, 5, 1, 0, 0], [7, 3, 8, 7, 0], 4, 6, 10)
    u32 = lambda a: pa.array(a, type=pa.uint32())
    m = count.CountMatrix(u32(want.cell), u32(want.feature), u32(want.n_umis), u32(want.n_reads),
                          pa.array(want.indptr, type=pa.int64()), (4, 6), 4, 5, 5)
    dense = np.zeros((4, 6), dtype=np.int64)
    dense[0, 5], dense[2, 0], dense[2, 1], dense[3, 0] = 1, 1, 2, 1
    for with_indptr in (True, False):
        if not with_indptr:
            m.indptr = None
        sp = m.to_scipy()
        assert sp.shape == (4, 6) and sp.format == "csr" and np.array_equal(sp.toarray(), dense)
    assert m.umis_per_cell().tolist() == [1, 0, 3, 1] and m.features_per_cell().tolist() == [1, 0, 2, 1]
