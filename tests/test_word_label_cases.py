"""CPU checks of tests/word_label_cases.py: the planted ids are the oracle's, so the GPU tests
that use them at sizes the oracle cannot reach compare with the truth."""
from __future__ import annotations

import numpy as np
import pytest

import word_label_cases as W

LS = [10, 12, 13, 14, 16]


def _oracle(pl, md):
    from oracle import pyoracle as P

    col = P.StrCol.from_fixed(W.codes_to_ascii(pl.codes(), pl.L))
    cid, valid, k, _ = P.umi_cluster(col, pl.L, md)
    assert valid.all()
    return cid.astype(np.int64), k


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("F", [0, 5000])
@pytest.mark.parametrize("L", LS)
def test_planted_ids_equal_oracle(L, F, sparse):
    pl = W.build(L, F=F, sparse=sparse)
    codes = pl.codes()
    assert len(codes) == pl.n_distinct and np.all(np.diff(codes) > 0)  # ascending, distinct
    cid, k = _oracle(pl, 1)
    assert k == pl.n_clusters
    assert np.array_equal(cid, pl.ids())
    cid0, k0 = _oracle(pl, 0)
    assert k0 == pl.n_distinct
    assert np.array_equal(cid0, pl.exact_ids())
    # the word table agrees with the ids: the majority label is the id of the majority codes
    for w in pl.words:
        ids = pl.gadget_ids[np.searchsorted(pl.gadget_codes, w["codes"])]
        if w["majority_label"] is None:
            assert np.bincount(ids - ids.min()).max() * 2 <= len(ids), w["kind"]
        else:
            assert np.count_nonzero(ids == w["majority_label"]) == w["majority_size"], w["kind"]
            assert w["majority_size"] * 2 > len(ids), w["kind"]
            assert len(set(ids.tolist())) == 1 + w["n_other"], w["kind"]


def test_every_kind_is_planted():
    pl = W.build(12, F=0)
    kinds = [w["kind"] for w in pl.words]
    for kind, words in W.WORDS.items():
        assert kinds.count(kind) >= 2 * len(words), kind  # below and above the boundary block
    by = {w["kind"]: w for w in pl.words}
    assert by["e_exc1_bit0"]["codes"][0] & 63 == 0 and by["e_exc1_bit63"]["codes"][-1] & 63 == 63
    assert {int(c) & 63 for c in by["e_exc2_bit0_bit63"]["codes"]} >= {0, 63}
    assert by["j_single"]["codes"].size == 1
    # kinds f: the exceptions' ids are below the word's
    for kind in ("f_exc1_lower", "f_exc2_lower"):
        w = by[kind]
        ids = pl.gadget_ids[np.searchsorted(pl.gadget_codes, w["codes"])]
        assert (ids[ids != w["majority_label"]] < w["majority_label"]).all()
    # kind h: two words share their majority label; kind i: so do p and p'
    for kind in ("h_span", "i_global"):
        assert len({w["majority_label"] for w in pl.words if w["kind"] == kind}) == 2  # below, above
    assert len(set(kinds)) == len(W.WORDS)


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("L", LS)
def test_fillers_are_singletons_apart_from_gadgets(L, sparse):
    pl = W.build(L, F=5000, sparse=sparse)
    f = pl.fillers()
    assert np.all(np.diff(f) > 0)
    words = f >> 6
    per_word = np.bincount(np.unique(words, return_inverse=True)[1])
    assert per_word.max() == (1 if sparse else 16)
    rng = np.random.default_rng(L)
    # the lowest fillers (dense words), a random sample, and fillers from the top of the range
    cap = W.filler_capacity(L, sparse)
    top = W.fillers(L, cap, sparse)[-300:] if cap <= 1 << 20 else f[-300:]
    sample = np.unique(np.concatenate([f[:300], rng.choice(f, 400, replace=False), top]))
    W.check_separation(pl, sample)
    assert ((f >> (2 * (L - 1))) < 3).all() and (((f >> (2 * (L - 2))) & 3) < 3).all()
    assert (pl.gadget_codes >> (2 * (L - 2)) == 15).all()  # gadgets start with TT


@pytest.mark.parametrize("L,T,sparse", [(10, 1 << 17, False), (12, 1 << 17, False), (13, 1 << 17, False),
                                        (16, 1 << 17, False), (14, 1 << 24, False), (12, 1 << 17, True),
                                        (14, 1 << 21, True)])
def test_boundary_labels(L, T, sparse):
    """T-1 and T are majority labels of words of kinds b, c and d, from the arithmetic of F
    alone (no filler is generated)."""
    pl = W.build(L, T=T, sparse=sparse)
    assert 0 < pl.F <= W.filler_capacity(L, sparse)
    assert pl.on_boundary(T)
    for letter in "bcd":
        labels = pl.majority_labels(letter)
        assert min(labels) < T - 1 and max(labels) > T  # and words of the kind on both sides
    # the parities mix
    assert {x & 1 for x in pl.majority_labels("b")} == {0, 1}
    assert not W.build(L, F=pl.F + 1, sparse=sparse).on_boundary(T)


def test_device_rows_carry_their_ids():
    pl = W.build(16, F=5000)
    codes, ids, rank, is_gadget = (t.numpy() for t in W.device_rows(pl, 7, "cpu"))
    n = len(codes)
    assert n % 4 == 3 and n > pl.n_distinct + 3000
    at = np.searchsorted(pl.codes(), codes.view(np.uint32).astype(np.int64))
    assert np.array_equal(at, rank) and np.array_equal(pl.ids()[at], ids)
    assert np.array_equal(np.unique(rank), np.arange(pl.n_distinct))  # every code occurs
    assert np.array_equal(is_gadget, codes < 0)  # L = 16: exactly the gadget codes are negative
    assert np.bincount(rank[is_gadget]).max() >= 2


def test_torch_fillers_equal_numpy():
    import torch

    for L, sparse in ((10, False), (14, False), (16, False), (12, True)):
        a = W.fillers(L, 70_001, sparse)
        b = W.fillers(L, 70_001, sparse, device="cpu")
        assert np.array_equal(a, b.numpy())
        assert np.array_equal(W.to_int32(a), W.to_int32(b).numpy())
    g = W.build(16, F=0).gadget_codes
    assert (W.to_int32(g) < 0).all()
    assert np.array_equal(W.to_int32(g), W.to_int32(torch.from_numpy(g)).numpy())
