"""Directional UMI clustering and correction on the GPU (rogtk_amd/csrc/directional.hip,
DESIGN.md §4c) against the pure-Python restatement of the spec (tests/directional_spec.py):
exact equality everywhere (ids, n_clusters, clusters table, corrected values, null count).

Shapes are tiny and chosen where the kernels can break: u32 and u64 sort keys (umi_len 16 with
the all-T code 0xFFFFFFFF, 17, 32 with the top bits in use), row counts around the wave and
block widths, a run of one UMI longer than a workgroup, a 300-step path for the relaxation,
count-1 plateaus and contested vertices in a crowded code space, and the degenerate columns."""
from __future__ import annotations

import ctypes

import numpy as np
import pyarrow as pa
import pytest

from correct_spec import as_bytes, table_of
from directional_spec import (KNOWN_ROWS, KNOWN_TABLE, code, random_families, regular_counts, restate,
                              roots_fixed_point)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rg():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import rogtk_amd

    assert rogtk_amd.device_count() >= 1
    return rogtk_amd


def _bin(items):
    return pa.array(items, type=pa.large_binary())


def _rounds():
    from rogtk_amd import _lib

    r = ctypes.c_int64(-1)
    _lib.call("rogtk_directional_last_rounds", ctypes.byref(r))
    return r.value


def _check(rg, items, umi_len):
    """umi_correct and umi_cluster with method="directional" against the restatement, and the
    invariants of the spec."""
    ids, k, table, corrected = restate(items, umi_len)
    res = rg.umi_correct(_bin(items), umi_len, 1, method="directional")
    assert res.n_clusters == k
    assert res.cluster_id.to_pylist() == ids
    assert table_of(res.clusters) == table
    assert as_bytes(res.corrected) == corrected
    assert res.corrected.null_count == sum(x is None for x in items)
    cid, kc, _ = rg.umi_cluster(_bin(items), umi_len, 1, method="directional")
    assert kc == k and cid.to_pylist() == ids
    got = table_of(res.clusters)
    assert sum(t[1] for t in got) == sum(x is not None for x in items)
    assert sum(t[2] for t in got) == len({x for x in items if x is not None})
    per = {}
    for x, c in zip(items, ids):  # every representative is its cluster's most frequent member
        if x is not None:
            per.setdefault(c, {}).setdefault(bytes(x), 0)
            per[c][bytes(x)] += 1
    for c, members in per.items():
        assert members[got[c][0]] == max(members.values())
    return res, ids, k, table, corrected


# ------------------------------------------------------------ the known answer
def test_known_answer_eager(rg):
    res, ids, k, table, corrected = _check(rg, KNOWN_ROWS, 4)
    assert k == 8 and table == KNOWN_TABLE and res.umi_len == 4
    assert _rounds() >= 1
    assert as_bytes(rg.umi_correct(_bin(KNOWN_ROWS), 0, 1, method="directional").corrected) == corrected
    assert as_bytes(rg.col(_bin(KNOWN_ROWS)).umi.correct(4, 1, method="directional")) == corrected
    assert rg.col(_bin(KNOWN_ROWS)).umi.cluster(4, method="directional").to_pylist() == ids
    # the default method is today's: the transitive clusters, fewer of them
    assert rg.umi_correct(_bin(KNOWN_ROWS), 4, 1).n_clusters < k
    assert as_bytes(rg.umi_correct(_bin(KNOWN_ROWS), 4, 1, method="cluster").corrected) == as_bytes(
        rg.umi_correct(_bin(KNOWN_ROWS), 4, 1).corrected)


@pytest.mark.parametrize("n_chunks", [1, 3])
def test_known_answer_plugin(rg, n_chunks):
    from rogtk_amd import plugin

    strs = [None if x is None else x.decode() for x in KNOWN_ROWS]
    cuts = np.linspace(0, len(strs), n_chunks + 1).astype(int)
    col = pa.chunked_array([pa.array(strs[a:b], type=pa.string()) for a, b in zip(cuts[:-1], cuts[1:])])
    _, _, _, corrected = restate(KNOWN_ROWS, 4)
    out, name = plugin.call_plugin_named("umi_correct_expr", [col],
                                         {"umi_len": 4, "max_distance": 1, "method": "directional"}, ["umi"])
    assert name == "umi" and as_bytes(out.combine_chunks()) == corrected
    out = plugin.call_plugin("umi_correct_expr", [col], {"method": "directional"})
    assert as_bytes(out.combine_chunks()) == corrected
    # method omitted, or "cluster": today's answer
    today = as_bytes(rg.umi_correct(_bin(KNOWN_ROWS), 4, 1).corrected)
    assert today != corrected
    for kwargs in ({"umi_len": 4, "max_distance": 1}, {"umi_len": 4, "method": "cluster"}, None):
        out = plugin.call_plugin("umi_correct_expr", [col], kwargs)
        assert as_bytes(out.combine_chunks()) == today


def _device_column(items):
    import torch

    dense = [u if u is not None else b"" for u in items]
    off = torch.tensor(np.concatenate([[0], np.cumsum([len(u) for u in dense])]), dtype=torch.int64).cuda()
    val = torch.tensor(np.frombuffer(b"".join(dense) or b"\0", np.uint8).copy()).cuda()
    vbits = torch.from_numpy(np.packbits(np.array([u is not None for u in items] + [False] * 7),
                                         bitorder="little")).cuda()
    return off, val, vbits


def test_known_answer_device_column(rg):
    import torch
    from rogtk_amd import _lib

    items = KNOWN_ROWS
    n = len(items)
    ids, k, table, corrected = restate(items, 4)
    off, val, vbits = _device_column(items)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    cid = torch.empty(n, dtype=torch.int32, device="cuda")
    root_code = torch.empty(n, dtype=torch.int64, device="cuda")
    nk = ctypes.c_int64(0)
    _lib.call("rogtk_umi_cluster_directional_dev", p(off), p(val), p(vbits), n, 4, p(cid), ctypes.byref(nk),
              p(root_code), s)
    torch.cuda.synchronize()
    assert nk.value == k and _rounds() >= 1
    want_ids = [0xFFFFFFFF if i is None else i for i in ids]
    assert cid.cpu().numpy().view(np.uint32).tolist() == want_ids
    rc = root_code.cpu().numpy().view(np.uint64)
    for i, x in enumerate(items):
        regular = x is not None and len(x) == 4 and all(c in b"ACGT" for c in x)
        assert int(rc[i]) == (code(corrected[i]) if regular else 0xFFFFFFFFFFFFFFFF), i
    # without the optional output; then ids + summary + gather in one call
    cid2 = torch.empty(n, dtype=torch.int32, device="cuda")
    _lib.call("rogtk_umi_cluster_directional_dev", p(off), p(val), p(vbits), n, 4, p(cid2), ctypes.byref(nk), None, s)
    torch.cuda.synchronize()
    assert torch.equal(cid, cid2)
    out = torch.zeros(val.numel(), dtype=torch.uint8, device="cuda")
    cid3 = torch.empty(n, dtype=torch.int32, device="cuda")
    _lib.call("rogtk_umi_correct_directional_dev", p(off), p(val), p(vbits), n, 4, p(cid3), ctypes.byref(nk), p(out), s)
    torch.cuda.synchronize()
    assert nk.value == k and torch.equal(cid, cid3)
    o, data = off.cpu().numpy(), out.cpu().numpy().tobytes()
    for i, x in enumerate(items):
        if x is not None:
            assert data[o[i]:o[i + 1]] == corrected[i], i


def _codes_entry(counts, L):
    """rogtk_directional_codes on the distinct codes of `counts`: (root, labels, n_clusters, rounds)."""
    import torch
    from rogtk_amd import _lib

    verts = sorted(counts, key=code)
    m = len(verts)
    D = torch.from_numpy(np.array([code(v) for v in verts], dtype=np.uint64).view(np.int64)).cuda()
    C = torch.from_numpy(np.array([counts[v] for v in verts], dtype=np.uint32).view(np.int32)).cuda()
    root = torch.empty(m, dtype=torch.int32, device="cuda")
    labels = torch.empty(m, dtype=torch.int32, device="cuda")
    tb = ctypes.c_int64(0)
    _lib.call("rogtk_directional_temp_bytes", m, L, ctypes.byref(tb))
    temp = torch.empty(tb.value, dtype=torch.uint8, device="cuda")
    nk, rounds = ctypes.c_int64(0), ctypes.c_int64(0)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.call("rogtk_directional_codes", p(D), p(C), m, L, p(root), p(labels), ctypes.byref(nk), ctypes.byref(rounds),
              p(temp), tb.value, s)
    torch.cuda.synchronize()
    # a temp one byte short is refused, not overrun
    with pytest.raises(_lib.RogtkError) as e:
        _lib.call("rogtk_directional_codes", p(D), p(C), m, L, p(root), p(labels), ctypes.byref(ctypes.c_int64(0)),
                  ctypes.byref(ctypes.c_int64(0)), p(temp), tb.value - 1, s)
    assert e.value.code == _lib.ROGTK_E_INVALID
    return verts, root.cpu().numpy().tolist(), labels.cpu().numpy().tolist(), nk.value, rounds.value


def _check_codes(counts, L):
    verts, root, labels, nk, rounds = _codes_entry(counts, L)
    want = roots_fixed_point(counts)
    at = {v: j for j, v in enumerate(verts)}
    assert root == [at[want[v]] for v in verts]
    order = {r: c for c, r in enumerate(sorted(set(want.values()), key=code))}
    assert labels == [order[want[v]] for v in verts]
    assert nk == len(order) and rounds >= 1
    return rounds


def test_known_answer_codes_entry(rg):
    _check_codes(regular_counts(KNOWN_ROWS, 4), 4)
    _check_codes({b"ACGT": 3}, 4)  # one vertex: one round that changes nothing


# ------------------------------------------------------------ every length class
def _families(seed, L, n_parents=24, include=()):
    """About 300 rows: parents (the first ones given) with skewed family sizes, one substitution
    per erroneous read, a few two-step errors, nulls and irregular rows."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    parents = list(include) + [bytes(acgt[rng.integers(0, 4, L)]) for _ in range(n_parents - len(include))]
    rows = []
    for j, par in enumerate(parents):
        size = max(1, int(40 / (1 + j % 7)))
        for _ in range(size):
            r = bytearray(par)
            u = rng.random()
            if u < 0.35:
                for _ in range(1 if u < 0.28 else 2):
                    q = int(rng.integers(0, L))
                    r[q] = int(rng.choice([b for b in b"ACGT" if b != r[q]]))
            rows.append(bytes(r))
    for i in range(0, len(rows), 29):
        rows[i] = None
    for i in range(7, len(rows), 41):
        rows[i] = rows[i][:-1] + b"N"
    rows.append(parents[0] + b"A")
    rows.append(b"")
    order = rng.permutation(len(rows))
    return [rows[i] for i in order]


@pytest.mark.parametrize("L", [1, 12, 16, 17, 32])
def test_every_length_class(rg, L):
    include = ()
    if L == 16:
        include = (b"T" * 16, b"T" * 15 + b"G")  # code 0xFFFFFFFF and its neighbour
    if L == 32:
        include = (b"T" * 32, b"G" + b"T" * 31, b"TG" + b"A" * 30)  # the top bits of a u64 code
    items = _families(L, L, include=include)
    assert 250 < len(items) < 400
    _, _, _, table, _ = _check(rg, items, L)
    if include:
        assert include[0] in [t[0] for t in table]


# ------------------------------------------------------------ convergence
def _walk(L, steps, seed):
    rng = np.random.default_rng(seed)
    cur = bytearray(bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)]))
    out, seen = [bytes(cur)], {bytes(cur)}
    while len(out) < steps:
        q = int(rng.integers(0, L))
        b = int(rng.choice([b for b in b"ACGT" if b != cur[q]]))
        nxt = bytearray(cur)
        nxt[q] = b
        if bytes(nxt) in seen:
            continue
        cur = nxt
        seen.add(bytes(cur))
        out.append(bytes(cur))
    return out


def test_long_path_converges(rg):
    walk = _walk(16, 300, 9)
    res, ids, k, table, corrected = _check(rg, walk, 16)
    rounds = _rounds()
    assert k == 1 and table == [(min(walk), 300, 300)] and 1 <= rounds <= 300
    assert _check_codes(regular_counts(walk, 16), 16) <= 300
    # counts halving along the first steps: the head of the walk absorbs everything
    heavy = []
    for j, u in enumerate(walk):
        heavy += [u] * max(1, 256 >> j)
    res, ids, k, table, corrected = _check(rg, heavy, 16)
    assert k == 1 and table == [(walk[0], len(heavy), 300)] and 1 <= _rounds() <= 300


# ------------------------------------------------------------ awkward sizes
@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_awkward_row_counts(rg, n):
    items = _families(n, 12)[:n]
    assert len(items) == n
    _check(rg, items, 12)


def test_a_run_longer_than_a_workgroup(rg):
    big = b"ACGTACGTACGT"
    items = [big] * 5000 + [b"ACGTACGTACGA", b"ACGTACGTACGA", b"CCGTACGTACGT"]
    perm = np.random.default_rng(1).permutation(len(items))
    items = [items[j] for j in perm]
    assert len(items) == 5003
    _, _, k, table, _ = _check(rg, items, 12)
    assert k == 1 and table == [(big, 5003, 3)]  # 5000 >= 2 * 2 - 1: the run's count is whole


# ------------------------------------------------------------ degenerate columns
def test_degenerate_columns(rg):
    for col in (_bin([]), pa.chunked_array([], type=pa.large_string())):
        res = rg.umi_correct(col, 4, 1, method="directional")
        assert res.n_clusters == 0 and len(res.clusters) == 0 and len(res.corrected) == 0
        assert rg.umi_cluster(col, 4, 1, method="directional")[1] == 0
    res = rg.umi_correct(_bin([None] * 5), 4, 1, method="directional")
    assert res.n_clusters == 0 and len(res.clusters) == 0
    assert res.corrected.to_pylist() == [None] * 5 and res.cluster_id.to_pylist() == [None] * 5
    irregular = [b"ACGN", b"ACG", None, b"acgt", b"ACGN", b"", b"ACGTA"]
    _, ids, k, table, _ = _check(rg, irregular, 4)
    assert k == 5 and ids == [2, 1, None, 4, 2, 0, 3]  # byte-lexicographic
    assert _rounds() == 0


# ------------------------------------------------------------ random families
@pytest.fixture(scope="module")
def families():
    rows = random_families()
    return rows, restate(rows, 8)


def test_random_families(rg, families):
    rows, (ids, k, table, corrected) = families
    res = rg.umi_correct(_bin(rows), 8, 1, method="directional")
    assert res.n_clusters == k
    assert res.cluster_id.to_pylist() == ids
    assert table_of(res.clusters) == table
    assert as_bytes(res.corrected) == corrected
    # every directional cluster lies in one transitive cluster, and there are more of them
    tid, kt, _ = rg.umi_cluster(_bin(rows), 8, 1)
    inside = {}
    for d, t in zip(ids, tid.to_pylist()):
        assert inside.setdefault(d, t) == t
    assert k > kt


def test_row_order_and_chunking_invariance(rg, families):
    rows, (ids, k, table, corrected) = families
    rows, corrected = rows[:6000], None
    base = rg.umi_correct(_bin(rows), 8, 1, method="directional")
    bc = as_bytes(base.corrected)
    perm = np.random.default_rng(5).permutation(len(rows))
    got = rg.umi_correct(_bin([rows[j] for j in perm]), 8, 1, method="directional")
    assert table_of(got.clusters) == table_of(base.clusters)
    assert as_bytes(got.corrected) == [bc[j] for j in perm]
    cuts = [0, 7, 7, 1000, len(rows)]
    chunked = pa.chunked_array([_bin(rows[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
    again = rg.umi_correct(chunked, 8, 1, method="directional")
    assert as_bytes(again.corrected) == bc and table_of(again.clusters) == table_of(base.clusters)


# ------------------------------------------------------------ max_distance and method
def test_max_distance_0_is_the_exact_grouping(rg):
    items = _families(2, 12)
    a = rg.umi_correct(_bin(items), 12, 0, method="directional")
    b = rg.umi_correct(_bin(items), 12, 0, method="cluster")
    assert a.n_clusters == b.n_clusters and a.cluster_id.to_pylist() == b.cluster_id.to_pylist()
    assert table_of(a.clusters) == table_of(b.clusters) and as_bytes(a.corrected) == as_bytes(b.corrected)
    ca = rg.umi_cluster(_bin(items), 12, 0, method="directional")
    cb = rg.umi_cluster(_bin(items), 12, 0)
    assert ca[1] == cb[1] and ca[0].to_pylist() == cb[0].to_pylist()


def test_bad_arguments_raise(rg):
    from rogtk_amd import _lib

    for fn in (rg.umi_correct, rg.umi_cluster):
        with pytest.raises(_lib.RogtkError) as e:
            fn(_bin(KNOWN_ROWS), 4, 2, method="directional")
        assert e.value.code == _lib.ROGTK_E_UNSUPPORTED
        with pytest.raises(ValueError):
            fn(_bin(KNOWN_ROWS), 4, 1, method="nonsense")


# ------------------------------------------------------------ dense code sets, large counts
# k_dir_edges bounds each binary search by |index(q) - v| <= |q - code|, which is tight only when
# the code set is dense; and need = 2 count - 1 must not wrap at a u32 count (backend_cases.py).
@pytest.mark.parametrize("L", [1, 2, 3, 4, 5])
def test_full_grid_of_codes(rg, L):
    """Every one of the 4^L codes is present: the search window of a neighbour d apart in value
    is exactly d entries, its end is index m for the largest codes and index 0 for the smallest."""
    from backend_cases import grid_counts
    from directional_spec import roots_bfs

    counts = dict(grid_counts(L))
    assert len(counts) == 4 ** L
    assert roots_fixed_point(counts) == roots_bfs(counts)
    _check_codes(counts, L)


@pytest.mark.parametrize("percent", [50, 90])
def test_most_of_the_grid_at_length_6(rg, percent):
    from backend_cases import grid_counts

    counts = dict(grid_counts(6, percent))
    assert len(counts) == 4096 * percent // 100
    _check_codes(counts, 6)


@pytest.mark.parametrize("name", ["edge_at_2_pow_31", "no_edge_above", "equal_maxima"])
def test_counts_at_the_top_of_u32(rg, name):
    """One pair of neighbours per case; the restatement computes 2 * count - 1 in Python integers."""
    from backend_cases import LARGE_COUNT_PAIRS
    from directional_spec import passes

    (a, b), edge = LARGE_COUNT_PAIRS[name]
    counts = {b"ACGA": a, b"ACGT": b}
    assert passes(a, b) == edge and not passes(b, a)
    want = roots_fixed_point(counts)
    assert want[b"ACGT"] == (b"ACGA" if edge else b"ACGT") and want[b"ACGA"] == b"ACGA"
    _check_codes(counts, 4)
