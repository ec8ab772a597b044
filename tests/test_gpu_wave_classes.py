"""The wave-per-group k-mer kernel (k_kmer_wave, classes 2 and 6) at its table, sort and row
limits: the groups of tests/wave_cases.py (pinned on the CPU by tests/test_wave_cases.py)
through rogtk_amd.kmer_spectrum and the fixed-stride entry points.

Every output array equals the oracle's; the class each group starts and ends in
(rogtk_kmer_debug_classes, tests only) equals the prediction made from the documented caps,
group by group; and the same calls without the wave class (rogtk_kmer_set_path(2)) and on the
global path (0) give the same outputs. A group that silently stopped reaching a limit, or a
bail-out that left the wave's table, its all-T counter or the group's class wrong for whoever
runs next, fails here.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pyarrow as pa
import pytest

import wave_cases as W

pytestmark = pytest.mark.gpu

FIELDS = ("kmer_hi", "kmer_lo", "exts", "counts")


@functools.lru_cache(maxsize=None)
def _calls():
    """name -> (k, min_cov, groups): the ordered layouts and one call per (k, min_coverage)."""
    out = {"state": (16, 2, W.layout_state()), "pipeline": (16, 2, W.layout_pipeline())}
    for (k, mc), groups in W.general_layouts().items():
        out[f"cases_k{k}_mc{mc}"] = (k, mc, groups)
    return out


@functools.lru_cache(maxsize=None)
def _reference(name, fixed=False):
    """(items, group offsets, the oracle's result) of a call, computed once."""
    from oracle import pyoracle as P

    k, mc, groups = (_calls()[name] if not fixed else _fixed_calls()[name])
    items, go = W.flatten(groups)
    ref = P.kmer_spectrum(P.StrCol.from_list(items), k, mc, False, np.array(go, np.int64))
    return items, go, ref


@functools.lru_cache(maxsize=None)
def _fixed_calls():
    return {f"k{k}_mc{mc}": (k, mc, groups) for (k, mc), groups in W.layouts_fixed_stride().items()}


def _same(got, ref, what):
    """The comparison of tests/test_gpu_kmer.py::_check: offsets, stats and the four arrays."""
    assert np.array_equal(got["entry_offsets"], ref["group_offsets"]), what
    assert np.array_equal(got["stats"], ref["stats"]), what
    for f in FIELDS:
        assert np.array_equal(got[f], ref[f]), (what, f)


class _Classes:
    """Registers a host buffer with rogtk_kmer_debug_classes and sets the path; restores both."""

    def __init__(self, G, path):
        self.G, self.path = G, path
        self.buf = np.full(2 * G, 0xFF, np.uint8)

    def __enter__(self):
        from rogtk_amd import _lib

        _lib.call("rogtk_kmer_debug_classes", self.buf.ctypes.data_as(ctypes.c_void_p), self.G)
        _lib.call("rogtk_kmer_set_path", self.path)
        return self

    def __exit__(self, *exc):
        from rogtk_amd import _lib

        try:
            _lib.call("rogtk_kmer_set_path", 1)
        finally:
            _lib.call("rogtk_kmer_debug_classes", None, 0)

    @property
    def initial(self):
        return self.buf[:self.G].astype(np.int64)

    @property
    def final(self):
        return self.buf[self.G:].astype(np.int64)


def _assert_classes(cl, groups, stride, wave, what):
    pred = [c.predict(stride, wave) for c in groups]
    want_i, want_f = np.array([p[0] for p in pred]), np.array([p[1] for p in pred])
    bad = np.flatnonzero((cl.initial != want_i) | (cl.final != want_f))
    assert bad.size == 0, (what, [(int(g), groups[g].name, (int(cl.initial[g]), int(cl.final[g])), pred[g])
                                  for g in bad[:8]])


@pytest.mark.parametrize("name", ["state", "pipeline", "cases_k16_mc1", "cases_k16_mc2", "cases_k8_mc1",
                                  "cases_k8_mc2", "cases_k4_mc1"])
def test_ragged_vs_oracle_and_classes(name):
    import rogtk_amd

    assert set(_calls()) == {"state", "pipeline", "cases_k16_mc1", "cases_k16_mc2", "cases_k8_mc1", "cases_k8_mc2",
                             "cases_k4_mc1"}
    k, mc, groups = _calls()[name]
    items, go, ref = _reference(name)
    col = pa.array(items, type=pa.large_binary())
    G = len(groups)
    outs = {}
    for path in (1, 2, 0):
        with _Classes(G, path) as cl:
            got = rogtk_amd.kmer_spectrum(col, k, mc, False, go)
        _same(got, ref, (name, path))
        outs[path] = got
        if path == 1:
            _assert_classes(cl, groups, 0, True, name)
            # the cases are still on the wave path: the restated classifier says so, and the hook agrees
            assert np.count_nonzero(cl.initial == 2) == sum(c.init == 2 for c in groups) > 0
        elif path == 2:
            assert not np.isin(cl.initial, (2, 6)).any() and not np.isin(cl.final, (2, 6)).any()
            _assert_classes(cl, groups, 0, False, name)
        else:
            assert (cl.buf == 0xFF).all()  # the global path classifies nothing
    for path in (2, 0):
        for f in FIELDS + ("entry_offsets", "stats"):
            assert np.array_equal(outs[1][f], outs[path][f]), (name, path, f)


def test_hook_is_off_when_unregistered():
    """NULL / 0 unregisters: a later call leaves an earlier buffer alone; a buffer too small
    for the call's groups is not written."""
    import rogtk_amd
    from rogtk_amd import _lib

    k, mc, groups = _calls()["cases_k4_mc1"]
    items, go, ref = _reference("cases_k4_mc1")
    col = pa.array(items, type=pa.large_binary())
    G = len(groups)
    with _Classes(G, 1) as cl:
        pass
    _same(rogtk_amd.kmer_spectrum(col, k, mc, False, go), ref, "unregistered")
    assert (cl.buf == 0xFF).all()
    small = np.full(2 * G, 0xFF, np.uint8)
    _lib.call("rogtk_kmer_debug_classes", small.ctypes.data_as(ctypes.c_void_p), G - 1)
    try:
        _same(rogtk_amd.kmer_spectrum(col, k, mc, False, go), ref, "small buffer")
    finally:
        _lib.call("rogtk_kmer_debug_classes", None, 0)
    assert (small == 0xFF).all()
    with pytest.raises(_lib.RogtkError):
        _lib.call("rogtk_kmer_debug_classes", None, 5)


@pytest.mark.parametrize("name", ["k16_mc1", "k16_mc2"])
def test_fixed_stride_vs_oracle_and_classes(name):
    """The limits of rows, words, claim, valid and deep, the all-T cases and the state-carrying
    layout through rogtk_kmer_spectrum_blocks and rogtk_kmer_spectrum_fused (stride 5: a row
    counts 5 packed words whatever its length)."""
    import torch

    from rogtk_amd import device as D

    assert set(_fixed_calls()) == {"k16_mc1", "k16_mc2"}
    k, mc, groups = _fixed_calls()[name]
    items, go, ref = _reference(name, True)
    G = len(groups)
    lens = np.array([0 if x is None else len(x) for x in items], np.int64)
    stride = (int(lens.max()) + 31) // 32
    assert stride == 5
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)])).cuda()
    vals = torch.from_numpy(np.frombuffer(b"".join(x for x in items if x is not None), np.uint8).copy()).cuda()
    valid = np.array([x is not None for x in items])
    vbits = torch.from_numpy(np.packbits(np.concatenate([valid, np.zeros(7, bool)]), bitorder="little")).cuda()
    pk = D.PackedReads(off, vals, validity=vbits)
    assert pk.max_len == int(lens.max())
    gsel = torch.tensor(go, dtype=torch.int64).cuda()
    cap = int(np.clip(lens - 3, 0, None).sum())
    outs = {}
    for fused in (False, True):
        for path in (1, 2, 0):
            with _Classes(G, path) as cl:
                if fused:
                    r = D.kmer_spectrum_fused(off, vals, gsel, k, mc, cap, -1, validity=vbits)
                else:
                    r = D.kmer_spectrum_blocks(pk, off, vals, gsel, k, mc, cap, validity=vbits)
                torch.cuda.synchronize()
            km = r["kmers"].cpu().numpy().view(np.uint64)
            got = {"kmer_hi": km[:, 0], "kmer_lo": km[:, 1], "exts": r["exts"].cpu().numpy(),
                   "counts": r["counts"].cpu().numpy().view(np.uint16),
                   "entry_offsets": r["entry_offsets"].cpu().numpy(), "stats": r["stats"].cpu().numpy()}
            _same(got, ref, (name, fused, path))
            outs[fused, path] = got
            if path == 1:
                _assert_classes(cl, groups, stride, True, (name, fused))
            elif path == 2:
                assert not np.isin(cl.initial, (2, 6)).any()
                _assert_classes(cl, groups, stride, False, (name, fused))
    for key, got in outs.items():
        for f in FIELDS + ("entry_offsets", "stats"):
            assert np.array_equal(outs[False, 1][f], got[f]), (name, key, f)
