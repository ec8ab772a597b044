"""GPU: every word-label form of the max-distance-1 assign at the limits of its label field.

k_word_label writes one u32 per 64-code word in one of five forms (decode_word_label,
rogtk_internal.h; DESIGN.md "Word-label forms and their limits"): the inline one-exception
form holds labels below 2^24, the inline two-exception form labels below 2^17, the mask
form the rest. tests/word_label_cases.py plants words of every shape (uniform, one, two,
three and five exceptions, exceptions at bits 0 and 63, exceptions below the majority, no
majority, clusters over two words, a word made uniform by its neighbour, a single code)
below, at and above a threshold T, with T-1 and T the majority labels of words with one,
two and three exceptions. The planted ids are the oracle's (tests/test_word_label_cases.py
proves that on the CPU at small sizes), so no oracle runs over the large sets here. Ids are
compared exactly, from every assign entry point: ClusterEngine.assign, the deferred assign
after a single speculative round, and the fused score + assign (the one-pass kernel for
L <= 13, score then assign above), plus the exact ids of max_distance 0.

At L = 16 the gadget codes start with TT, so they have the top bit set and are negative
as torch int32: the device entry points take the bit pattern.

mark_bitmap serves 7 <= L <= 13; at L = 14 and 16 the bitmap comes from mark +
build_local_bitmap, as in cluster_batch.
"""
from __future__ import annotations

import os
import subprocess
import sys
import time

import numpy as np
import pyarrow as pa
import pytest

import word_label_cases as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def P():
    from oracle import pyoracle

    return pyoracle


def _target(pl):
    """The Hamming target: a majority code of the first one-exception word, so its word
    mates are within distance 1."""
    w = next(w for w in pl.words if w["kind"] == "b_exc1")
    return bytes(W.codes_to_ascii(w["codes"][:1], pl.L)[0])


def _bitmap(eng, batch):
    if 7 <= batch.umi_len <= 13:
        eng.mark_bitmap(batch)
    else:
        eng.mark(batch)
        eng.build_local_bitmap()
    return eng.local_bitmap


def _assert_stats(eng, n_clusters, what):
    stats = eng.stats()
    assert stats["n_clusters"] == n_clusters, (what, stats)
    assert stats["overflow"] == 0 and stats["error"] == 0, (what, stats)


def _assert_ids(got, want, what):
    import torch

    if not torch.equal(got, want):
        bad = torch.nonzero(got != want).flatten()
        k = bad[:5]
        raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} rows differ; rows {k.tolist()} "
                             f"got {got[k].tolist()} want {want[k].tolist()}")


def _check_entry_points(pl, seed=1, knob_out=None):
    """Ids of every assign entry point on the planted rows against the planted ids; the
    within bits and combined_score of the fused call against the oracle on the gadget rows
    and 2,000 other rows."""
    import torch

    from rogtk_amd import device as D

    L = pl.L
    codes, ids, rank, is_gadget = W.device_rows(pl, seed, "cuda")
    n = codes.numel()
    assert n % 4 == 3
    want, want0 = ids.to(torch.int32), rank.to(torch.int32)
    batch = D.PackedBatch(codes, L)
    eng = D.ClusterEngine(L, pl.n_distinct, "cuda")
    bitmap = _bitmap(eng, batch)

    cid = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    eng.resolve(bitmap, 1, 1)
    eng.assign(batch, cid)
    _assert_stats(eng, pl.n_clusters, "assign")
    _assert_ids(cid, want, "assign")

    cid.fill_(-7)
    try:
        D.set_spec_rounds(1)
        eng.resolve(bitmap, 1, 1)
        eng.assign(batch, cid, deferred=True)
        eng.sync()
    finally:
        D.set_spec_rounds(0)
    _assert_stats(eng, pl.n_clusters, "deferred assign")
    _assert_ids(cid, want, "deferred assign, 1 speculative round")

    cid.fill_(-7)
    target = _target(pl)
    scores = {"combined_score": torch.empty(n, dtype=torch.float64, device="cuda")}
    hw = torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda")
    eng.resolve(bitmap, 1, 1)
    D.score_assign_packed(batch, eng, cid, scores, target, 1, None, hw)
    _assert_stats(eng, pl.n_clusters, "score + assign")
    _assert_ids(cid, want, "score + assign")
    rows = torch.cat([torch.nonzero(is_gadget).flatten(),
                      torch.randint(0, n, (2000,), device="cuda", generator=torch.Generator("cuda").manual_seed(seed))])
    within = ((hw[rows >> 6] >> (rows & 63)) & 1).cpu().numpy().astype(bool)
    comb = scores["combined_score"][rows].cpu().numpy()
    col = P().StrCol.from_fixed(W.codes_to_ascii(codes[rows].cpu().numpy().view(np.uint32), L))
    _, rw, _ = P().hamming(col, target, 1)
    assert rw.sum() >= 3 and np.array_equal(within, rw)
    assert np.array_equal(comb.view(np.uint64), P().umi_complexity(col)["combined_score"].view(np.uint64))
    if knob_out is not None:
        knob_out["fused"] = cid.cpu().numpy()
        knob_out["codes"] = codes.cpu().numpy()

    cid.fill_(-7)
    eng.resolve(bitmap, 1, 0)
    eng.assign(batch, cid)
    _assert_stats(eng, pl.n_distinct, "exact ids")
    _assert_ids(cid, want0, "exact ids (max_distance 0)")
    return n


CASES = [(10, 1 << 17), (12, 1 << 17), (13, 1 << 17), (16, 1 << 17), (12, None)]


def _build(L, T, sparse=False):
    pl = W.build(L, F=0, sparse=sparse) if T is None else W.build(L, T=T, sparse=sparse)
    if T is not None:  # before the GPU is touched: the cases still sit on the boundary
        assert pl.on_boundary(T)
    return pl


@pytest.mark.parametrize("L,T", CASES, ids=lambda v: str(v))
def test_forms_at_label_limit(L, T):
    """Dense fillers (mask form with 15 exceptions at every label magnitude below T) and
    the gadget words around T; T = None: no fillers, every label below 2^17."""
    _check_entry_points(_build(L, T))


def test_forms_at_label_limit_sparse_fillers():
    """One filler per word: plain labels at every magnitude below T = 2^17 (L = 12)."""
    _check_entry_points(_build(12, 1 << 17, sparse=True))


def test_forms_at_2p24_index_space():
    """Labels reach 2^24 only at L >= 14 (clusters <= 4^(L-1)) and with more than 2^24 rows:
    16,777,362 distinct codes, 16,780,551 rows, labels by rank (k_assign MODE 1). A
    one-exception word whose majority label is 2^24 - 1 takes the inline form, the one at
    2^24 the mask form. Fillers, expected ids and the shuffle are made on the device; only
    the gadget rows and a 2,000-row sample reach the host. The sparse variant (one filler
    per word, plain labels) follows; a code space of 4^11 words holds 2,359,296 of those,
    so it runs at T = 2^21.

    Wall time measured on an MI355X (printed below): 0.02 s for the 2^24 case and 0.01 s for
    the sparse one, every kernel and the host-side sample check included."""
    import torch

    t0 = time.perf_counter()
    n = _check_entry_points(_build(14, 1 << 24))
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    m = _check_entry_points(_build(14, 1 << 21, sparse=True))
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(f"2^24 case: {n} rows {t1 - t0:.2f} s; sparse 2^21 case: {m} rows {t2 - t1:.2f} s")


# ------------------------------------------------------------------ host entry, k_lookup
def _host_column(pl, seed):
    """The planted codes as an Arrow large_binary column built from the byte matrix, plus
    irregular rows aimed at the gadgets: every gadget code once with one base replaced by N
    (the last base for every other one, so the probes of the irregular merge hit the code's
    word mates: majority codes, exception codes and codes of words without majority), a
    lowercase copy, a copy one base longer, and a null."""
    L = pl.L
    rng = np.random.default_rng(seed)
    codes = pl.codes()
    reg = W.codes_to_ascii(np.concatenate([codes, rng.choice(codes, 3000)]), L)
    irr = W.codes_to_ascii(pl.gadget_codes, L).copy()
    g = np.arange(len(irr))
    irr[g, np.where(g % 2 == 0, L - 1, g % L)] = ord("N")
    lower = W.codes_to_ascii(pl.gadget_codes[:1], L) | 0x20
    body = np.concatenate([reg, irr, lower])
    body = body[rng.permutation(len(body))]
    longer = np.append(W.codes_to_ascii(pl.gadget_codes[-1:], L)[0], np.uint8(ord("A")))
    n = len(body) + 2
    offsets = np.concatenate([np.arange(len(body) + 1, dtype=np.int64) * L,
                              np.array([len(body) * L + L + 1] * 2, dtype=np.int64)])
    values = np.concatenate([body.reshape(-1), longer])
    valid = np.ones(n, bool)
    valid[-1] = False
    vbits = np.packbits(valid, bitorder="little")
    arrow = pa.Array.from_buffers(pa.large_binary(), n, [pa.py_buffer(vbits), pa.py_buffer(offsets),
                                                         pa.py_buffer(values)])
    return arrow, P().StrCol(offsets, values, vbits, n)


@pytest.mark.parametrize("L,T", [(12, None), (12, 1 << 17), (13, 1 << 17)], ids=lambda v: str(v))
def test_host_entry_with_irregular_rows(L, T):
    """umi_cluster on a host column: the irregular merge looks the neighbours of its N rows up
    through k_lookup, which decodes the same word labels; ids, validity and count equal the
    oracle's."""
    import rogtk_amd as rg

    pl = _build(L, T)
    arrow, col = _host_column(pl, L)
    got, k, rl = rg.umi_cluster(arrow, L, 1)
    rc, rv, rk, _ = P().umi_cluster(col, L, 1, threads=min(16, os.cpu_count() or 1))
    assert rl == L and k == rk
    assert np.array_equal(np.asarray(got.is_valid().to_numpy(zero_copy_only=False)), rv)
    assert not rv[-1] and rv[:-1].all()
    ids = np.asarray(got.fill_null(0).to_numpy(zero_copy_only=False)).astype(np.uint32)
    assert np.array_equal(ids[rv], rc[rv])


# ------------------------------------------------------------------ ROGTK_WORD_EXC1=0
CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import test_gpu_word_labels as T
out = {{}}
T._check_entry_points(T._build(12, 1 << 17), knob_out=out)
np.savez({path!r}, **out)
"""


def test_mask_form_only_knob(tmp_path):
    """ROGTK_WORD_EXC1=0 (read once per process, so a child): words with one or two
    exceptions take the mask form too; every entry point still gives the planted ids (the
    child asserts that), and the parent compares the fused ids it saved with the table."""
    path = str(tmp_path / "out.npz")
    env = dict(os.environ, ROGTK_WORD_EXC1="0")
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), path=path)],
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    z = np.load(path)
    pl = _build(12, 1 << 17)
    at = np.searchsorted(pl.codes(), z["codes"].view(np.uint32).astype(np.int64))
    assert np.array_equal(z["fused"].astype(np.int64), pl.ids()[at])
