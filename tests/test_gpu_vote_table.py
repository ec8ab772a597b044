"""The per-workgroup vote table of correct.hip where it overflows: a vote that finds no LDS slot
goes straight to the global tables, and that fallback alone keeps the representative, n_reads
and n_distinct right once a 4096-row tile votes for more than 1024 clusters.

The entries take the caller's cluster ids, so the cases (tests/backend_cases.py) decide how many
clusters a tile sees; tests/test_backend_cases.py proves on the CPU that each case enters the
branch. Expected tables and corrected codes come from correct_spec.summarize: exact equality."""
from __future__ import annotations

import ctypes

import numpy as np
import pyarrow as pa
import pytest

import backend_cases as B
from correct_spec import summarize, table_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rg():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import rogtk_amd

    assert rogtk_amd.device_count() >= 1
    return rogtk_amd


def _encode(s):
    c = 0
    for b in s:
        c = (c << 2) | b"ACGT".index(b)
    return c


def _packed(case, all_regular, method):
    """rogtk_cluster_summary_packed + rogtk_cluster_correct_packed on the case's rows against
    summarize() of the same rows and ids."""
    import torch
    from rogtk_amd import _lib

    n, k, L = case.n, case.k, case.L
    table, corrected = summarize(case.items(all_regular), case.spec_ids(all_regular), k, L)
    want_rep = np.array([_encode(t[0]) if t[1] else 0xFFFFFFFF for t in table], dtype=np.uint32)
    want_cor = np.array([0xFFFFFFFF if x is None else _encode(x) for x in corrected], dtype=np.uint32)

    dev = torch.device("cuda:0")
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    d_codes = torch.from_numpy(case.codes.view(np.int32).copy()).to(dev)
    d_ids = torch.from_numpy(case.ids.view(np.int32).copy()).to(dev)
    bits = np.packbits(np.concatenate([case.reg, np.zeros(-n % 64, bool)]), bitorder="little").view(np.int64)
    d_reg = None if all_regular else torch.from_numpy(bits.copy()).to(dev)
    tb = ctypes.c_int64(0)
    _lib.call("rogtk_cluster_summary_temp_bytes", n, L, k, ctypes.byref(tb))
    temp = torch.empty(tb.value, dtype=torch.uint8, device=dev)
    rep = torch.full((k,), -2, dtype=torch.int32, device=dev)
    n_reads = torch.full((k,), -2, dtype=torch.int32, device=dev)
    n_distinct = torch.full((k,), -2, dtype=torch.int32, device=dev)
    out = torch.full((n,), 7, dtype=torch.int32, device=dev)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.call("rogtk_cluster_summary_set_method", method)
    try:
        _lib.call("rogtk_cluster_summary_packed", p(d_codes), p(d_reg), n, L, p(d_ids), k, p(rep), p(n_reads),
                  p(n_distinct), p(temp), tb.value, s)
    finally:
        _lib.call("rogtk_cluster_summary_set_method", 0)
    _lib.call("rogtk_cluster_correct_packed", p(d_ids), p(d_reg), n, p(rep), k, p(out), s)
    torch.cuda.synchronize()
    assert np.array_equal(rep.cpu().numpy().view(np.uint32), want_rep)
    assert n_reads.cpu().numpy().tolist() == [t[1] for t in table]
    assert n_distinct.cpu().numpy().tolist() == [t[2] for t in table]
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want_cor)
    assert int(n_reads.sum()) == (n if all_regular else int(case.reg.sum()))
    return table


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("all_regular", [True, False])
def test_own_id_every_code_its_own_cluster(rg, all_regular, method):
    """4096 cluster ids in one tile of 1024 slots: at least 3 000 votes take the fallback."""
    case = B.vote_case("own_id")
    table = _packed(case, all_regular, method)
    if all_regular:
        assert table[0] == (b"AAAAAA", 2, 1) and all(t[1:] == (1, 1) for t in table[1:])
    else:
        assert sum(t == (b"", 0, 0) for t in table) > 150  # clusters whose only row has its bit off


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("all_regular", [True, False])
def test_interleaved_large_clusters_among_singletons(rg, all_regular, method):
    """40 clusters that get votes from all three tiles, among singletons that fill the slots;
    the largest count of a large cluster is tied between two tiles and the smaller code wins."""
    case = B.vote_case("interleaved")
    table = _packed(case, all_regular, method)
    if all_regular:
        big = [t for t in table if t[2] > 1]
        assert len(big) == 40 and all(t[2] >= 56 for t in big)
        for rep, _, _ in big:  # the representative is the earlier of the two codes with 5 rows
            cid = case.ids[case.codes == _encode(rep)][0]
            assert _encode(rep) == np.unique(case.codes[case.ids == cid])[1]


@pytest.mark.parametrize("method", [0, 1])
def test_same_home_twelve_ids_one_probe_window(rg, method):
    """White box: this case reads the kernel's hash (backend_cases.vote_home restates
    `(id * 2654435761u) >> 22` of vote() in correct.hip). Its 12 cluster ids share one home slot,
    so they compete for one window of 8 probes and at least 4 of them vote through the fallback
    while the table is almost empty. If the hash changes the case still passes but no longer aims
    at the branch. Clusters without rows stay (b"", 0, 0)."""
    case = B.vote_case("same_home")
    table = _packed(case, True, method)
    ids = B.same_home_ids()
    assert [c for c, t in enumerate(table) if t[1]] == ids
    assert all(table[c][1:] == (5, 3) for c in ids)


@pytest.mark.parametrize("name", ["own_id", "interleaved", "same_home"])
def test_general_path_string_columns(rg, name):
    """The same cases as string columns with irregular strings and nulls: the tile is 4096 rows
    in (cluster id, string rank) order."""
    rows, ids, k, L = B.vote_strings(name)
    table, _ = summarize(rows, [None if x is None else i for x, i in zip(rows, ids)], k, L)
    got = rg.umi_cluster_summary(pa.array(rows, type=pa.large_binary()), np.array(ids, dtype=np.uint32),
                                 n_clusters=k, umi_len=L)
    assert table_of(got) == table
    assert sum(t[1] for t in table) == sum(x is not None for x in rows)
    # irregular representatives occur (more rows than every regular member), and so do regular
    # ones that won a count tie against an irregular string
    irregular = lambda s: len(s) != L or any(c not in b"ACGT" for c in s)
    assert any(t[1] and irregular(t[0]) for t in table)
    assert any(t[1] and not irregular(t[0]) and t[2] > 1 for t in table)
