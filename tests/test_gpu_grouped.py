"""UMI clustering and correction within groups on the GPU (rogtk_amd/csrc/grouped.hip, DESIGN.md
§4d) against the pure-Python restatement (tests/grouped_spec.py): exact equality of ids,
n_clusters, the clusters table with its group field, corrected values and null count.

Shapes are tiny and sit where the kernels can break: the search window at the edge of a group
(two groups holding the same dense code set under adjacent keys), sort keys of 2 to 64 bits,
row counts around the wave and the pack tile, one long relaxation next to a short one, and the
degenerate columns."""
from __future__ import annotations

import ctypes

import numpy as np
import pyarrow as pa
import pytest

import directional_spec as D
import grouped_spec as G
from correct_spec import as_bytes, table_of

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


def _u32(keys):
    return np.asarray([int(k) for k in keys], dtype=np.uint32)


def _rounds():
    from rogtk_amd import _lib

    r = ctypes.c_int64(-1)
    _lib.call("rogtk_directional_last_rounds", ctypes.byref(r))
    return r.value


def _table4(clusters):
    assert [f.name for f in clusters.type] == ["representative", "n_reads", "n_distinct", "group"]
    assert clusters.type.field("group").type == pa.uint32()
    return [t + (g,) for t, g in zip(table_of(clusters), clusters.field("group").to_pylist())]


def _same(res, want, items):
    ids, k, table, corrected = want
    assert res.n_clusters == k
    assert res.cluster_id.to_pylist() == ids
    assert _table4(res.clusters) == table
    assert as_bytes(res.corrected) == corrected
    assert res.corrected.null_count == sum(x is None for x in items)


def _check(rg, items, keys, umi_len, max_distance=1, method="directional"):
    want = G.restate(items, keys, umi_len, max_distance)
    res = rg.umi_correct(_bin(items), umi_len, max_distance, method=method, groups=_u32(keys))
    _same(res, want, items)
    cid, kc, _ = rg.umi_cluster(_bin(items), umi_len, max_distance, method=method, groups=_u32(keys))
    assert kc == want[1] and cid.to_pylist() == want[0]
    return res, want


def _rows(n, L, seed, nulls=True):
    """n rows from n // 8 + 2 parents with one substitution in a third of them, some nulls and
    some irregular rows."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    parents = [bytes(acgt[rng.integers(0, 4, L)]) for _ in range(n // 8 + 2)]
    rows = []
    for i in range(n):
        r = bytearray(parents[int(rng.integers(0, len(parents))) if rng.random() < 0.7 else 0])
        if rng.random() < 0.33:
            q = int(rng.integers(0, L))
            r[q] = int(rng.choice([b for b in b"ACGT" if b != r[q]]))
        rows.append(bytes(r))
    if nulls:
        for i in range(3, n, 31):
            rows[i] = None
        for i in range(5, n, 43):
            rows[i] = rows[i - 1][:-1] + b"N" if rows[i - 1] else b"N"
    return rows


# ------------------------------------------------------------ the known answer, every entry
def test_known_answer_eager(rg):
    res, want = _check(rg, D.KNOWN_ROWS, G.KNOWN_KEYS, 4)
    assert want[1] == 11 and want[2] == G.KNOWN_TABLE and res.umi_len == 4 and _rounds() >= 1
    corrected = want[3]
    for groups in (_u32(G.KNOWN_KEYS), pa.array(G.KNOWN_KEYS, type=pa.int64()),
                   pa.chunked_array([pa.array(G.KNOWN_KEYS[:100], type=pa.uint32()),
                                     pa.array(G.KNOWN_KEYS[100:], type=pa.uint32())]),
                   np.asarray(G.KNOWN_KEYS, dtype=np.int64)):
        _same(rg.umi_correct(_bin(D.KNOWN_ROWS), 0, 1, method="directional", groups=groups), want, D.KNOWN_ROWS)
        c = rg.col(_bin(D.KNOWN_ROWS))
        assert as_bytes(c.umi.correct(4, 1, method="directional", groups=groups)) == corrected
        assert c.umi.cluster(4, method="directional", groups=groups).to_pylist() == want[0]
    # the ungrouped call still gives its 8 clusters
    assert rg.umi_correct(_bin(D.KNOWN_ROWS), 4, 1, method="directional").n_clusters == 8


@pytest.mark.parametrize("key_type", [pa.int64(), pa.uint32()])
@pytest.mark.parametrize("n_chunks", [1, 3])
def test_known_answer_plugin(rg, n_chunks, key_type):
    from rogtk_amd import plugin

    strs = [None if x is None else x.decode() for x in D.KNOWN_ROWS]
    cuts = np.linspace(0, len(strs), n_chunks + 1).astype(int)
    col = pa.chunked_array([pa.array(strs[a:b], type=pa.string()) for a, b in zip(cuts[:-1], cuts[1:])])
    keys = pa.chunked_array([pa.array(G.KNOWN_KEYS[a:b], type=key_type) for a, b in zip(cuts[:-1], cuts[1:])])
    corrected = G.restate(D.KNOWN_ROWS, G.KNOWN_KEYS, 4)[3]
    out, name = plugin.call_plugin_named("umi_correct_expr", [col, keys],
                                         {"umi_len": 4, "max_distance": 1, "method": "directional"}, ["umi", "cell"])
    assert name == "umi" and as_bytes(out.combine_chunks()) == corrected
    # one input: today's answer
    today = as_bytes(rg.umi_correct(_bin(D.KNOWN_ROWS), 4, 1, method="directional").corrected)
    assert today != corrected
    out = plugin.call_plugin("umi_correct_expr", [col], {"umi_len": 4, "method": "directional"})
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

    items, n = D.KNOWN_ROWS, len(D.KNOWN_ROWS)
    ids, k, table, corrected = G.restate(items, G.KNOWN_KEYS, 4)
    off, val, vbits = _device_column(items)
    keys = torch.from_numpy(_u32(G.KNOWN_KEYS).view(np.int32)).cuda()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    cid = torch.empty(n, dtype=torch.int32, device="cuda")
    root_code = torch.empty(n, dtype=torch.int64, device="cuda")
    cgroup = torch.full((n,), -2, dtype=torch.int32, device="cuda")
    nk = ctypes.c_int64(0)
    _lib.call("rogtk_umi_cluster_grouped_dev", p(off), p(val), p(vbits), n, p(keys), 4, 1, 1, p(cid), ctypes.byref(nk),
              p(root_code), p(cgroup), s)
    torch.cuda.synchronize()
    assert nk.value == k and _rounds() >= 1
    want_ids = [0xFFFFFFFF if i is None else i for i in ids]
    assert cid.cpu().numpy().view(np.uint32).tolist() == want_ids
    assert cgroup.cpu().numpy().view(np.uint32)[:k].tolist() == [t[3] for t in table]
    rc = root_code.cpu().numpy().view(np.uint64)
    for i, x in enumerate(items):  # the root's code without the key
        regular = x is not None and len(x) == 4 and all(c in b"ACGT" for c in x)
        assert int(rc[i]) == (D.code(corrected[i]) if regular else 0xFFFFFFFFFFFFFFFF), i
    # without the optional outputs; then ids + summary + gather in one call
    cid2 = torch.empty(n, dtype=torch.int32, device="cuda")
    _lib.call("rogtk_umi_cluster_grouped_dev", p(off), p(val), p(vbits), n, p(keys), 4, 1, 1, p(cid2), ctypes.byref(nk),
              None, None, s)
    torch.cuda.synchronize()
    assert torch.equal(cid, cid2)
    out = torch.zeros(val.numel(), dtype=torch.uint8, device="cuda")
    cid3 = torch.empty(n, dtype=torch.int32, device="cuda")
    cgroup3 = torch.empty(n, dtype=torch.int32, device="cuda")
    _lib.call("rogtk_umi_correct_grouped_dev", p(off), p(val), p(vbits), n, p(keys), 4, 1, 1, p(cid3), ctypes.byref(nk),
              p(out), p(cgroup3), s)
    torch.cuda.synchronize()
    assert nk.value == k and torch.equal(cid, cid3) and torch.equal(cgroup[:k], cgroup3[:k])
    o, data = off.cpu().numpy(), out.cpu().numpy().tobytes()
    for i, x in enumerate(items):
        if x is not None:
            assert data[o[i]:o[i + 1]] == corrected[i], i


# ------------------------------------------------------------ one key, one key per row
@pytest.fixture(scope="module")
def families():
    """directional_spec.random_families() with the family of every row (the same draws)."""
    rng = np.random.default_rng(20)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    par = rng.integers(0, 4, size=(2000, 8))
    sizes = rng.geometric(1.0 / 10.0, size=2000)
    reads = np.repeat(par, sizes, axis=0)
    family = np.repeat(np.arange(2000), sizes)
    hit = rng.random(reads.shape) < 0.05
    reads = np.where(hit, (reads + rng.integers(1, 4, size=reads.shape)) % 4, reads)
    order = rng.permutation(len(reads))
    rows = [bytes(r) for r in acgt[reads][order]]
    assert rows == D.random_families()
    return rows, family[order]


def test_all_keys_equal_is_the_ungrouped_call(rg, families):
    rows, _ = families
    base = rg.umi_correct(_bin(rows), 8, 1, method="directional")
    for key in (0, 0xFFFFFFFF):
        got = rg.umi_correct(_bin(rows), 8, 1, method="directional", groups=np.full(len(rows), key, np.uint32))
        assert got.n_clusters == base.n_clusters and got.cluster_id.equals(base.cluster_id)
        assert got.corrected.equals(base.corrected)
        assert _table4(got.clusters) == [t + (key,) for t in table_of(base.clusters)]
    cid, k, _ = rg.umi_cluster(_bin(rows), 8, 1, method="directional", groups=np.zeros(len(rows), np.uint32))
    assert k == base.n_clusters and cid.equals(base.cluster_id)


def test_every_row_in_its_own_key(rg):
    items = _rows(500, 6, 1)
    _, (ids, k, table, corrected) = _check(rg, items, np.arange(len(items)), 6)
    assert k == sum(x is not None for x in items) and corrected == items
    assert len({x for x in items if x is not None}) < k  # the same string under two keys: two clusters


@pytest.mark.parametrize("mod", [1, 7, 1000])
def test_random_families(rg, families, mod):
    rows, family = families
    _check(rg, rows, family % mod, 8)


# ------------------------------------------------------------ the search window
def _dense(seed, L=4):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    out = []
    for c in range(4 ** L):
        s = bytes(acgt[[(c >> (2 * (L - 1 - j))) & 3 for j in range(L)]])
        out += [s] * int(rng.integers(1, 12))
    return out


@pytest.mark.parametrize("k0", [0, 5, 0xFFFFFFFE])
def test_window_two_dense_groups_under_adjacent_keys(rg, k0):
    """Both groups hold all 4^4 codes: a search that leaves its group finds the same code with
    another count next door."""
    a, b = _dense(1), _dense(2)
    items, keys = a + b, [k0] * len(a) + [k0 + 1] * len(b)
    perm = np.random.default_rng(3).permutation(len(items))
    res, want = _check(rg, [items[j] for j in perm], [keys[j] for j in perm], 4)
    assert {t[3] for t in want[2]} == {k0, k0 + 1}


def test_window_one_code_between_dense_groups(rg):
    a, b = _dense(4), _dense(5)
    items = a + [b"ACGT"] * 3 + b
    keys = [8] * len(a) + [9] * 3 + [10] * len(b)
    _, want = _check(rg, items, keys, 4)
    assert (b"ACGT", 3, 1, 9) in want[2]


def test_window_keys_0_and_max_together(rg):
    a, b = _dense(6, 3), _dense(7, 3)
    items = a + b + [b"ACG", b"ACT"]
    keys = [0] * len(a) + [0xFFFFFFFF] * len(b) + [0x7FFFFFFF, 0x80000000]
    _check(rg, items, keys, 3)


@pytest.mark.parametrize("window", [0, 1, 2])
def test_window_variants_agree(rg, window):
    """The three ways to bound the edge search (value distance alone, the table of key heads, a
    galloped range) give the one answer, at the edges of the array and of every group."""
    from rogtk_amd import _lib

    a, b, c = _dense(8), _dense(9, 3), _rows(600, 9, 10)
    items = a + [x + b"A" for x in b] + c + [b"AAAA", b"TTTT", b"TTTG"]
    keys = [0] * len(a) + [1] * len(b) + [2 + i % 50 for i in range(len(c))] + [0xFFFFFFFF] * 3
    want4 = G.restate(items, keys, 4)
    want9 = G.restate(items, keys, 9)
    _lib.call("rogtk_grouped_set_window", window)
    try:
        for L, want in ((4, want4), (9, want9)):
            _same(rg.umi_correct(_bin(items), L, 1, method="directional", groups=_u32(keys)), want, items)
    finally:
        _lib.call("rogtk_grouped_set_window", 2)  # the default
    with pytest.raises(_lib.RogtkError):
        _lib.call("rogtk_grouped_set_window", 3)


# ------------------------------------------------------------ sort width
def test_sort_width_64_bits(rg):
    items = [b"T" * 16] * 5 + [b"T" * 15 + b"G"] * 2 + [b"T" * 16] * 2 + [b"A" * 16, b"A" * 15 + b"C", None]
    keys = [0xFFFFFFFF] * 7 + [0] * 2 + [0xFFFFFFFF, 0, 0xFFFFFFFF]
    _, want = _check(rg, items, keys, 16)
    assert (b"T" * 16, 7, 2, 0xFFFFFFFF) in want[2] and (b"T" * 16, 2, 1, 0) in want[2]


def test_sort_width_length_1(rg):
    items = [b"A"] * 9 + [b"C"] * 2 + [b"G", b"T", b"N", None] + [b"A", b"C", b"C"]
    keys = [2] * 15 + [1, 1, 0]
    _check(rg, items, keys, 1)


def test_sort_width_length_20(rg):
    from rogtk_amd import _lib

    items = _rows(300, 20, 8)
    keys = [(0xFFFFFF, 0, 77)[i % 3] for i in range(len(items))]  # 24 bits: 40 + 24 = 64
    _check(rg, items, keys, 20)
    keys[10] = 1 << 24
    assert items[10] is not None and len(items[10]) == 20 and b"N" not in items[10]
    for fn in (rg.umi_correct, rg.umi_cluster):
        with pytest.raises(_lib.RogtkError) as e:
            fn(_bin(items), 20, 1, method="directional", groups=_u32(keys))
        assert e.value.code == _lib.ROGTK_E_UNSUPPORTED
    _check(rg, items, [0] * len(items), 20)  # the library still works after the refusal


def test_sort_width_length_32_takes_key_0_alone(rg):
    """64 code bits leave none for a key: key 0 is the ungrouped call, any other is refused."""
    from rogtk_amd import _lib

    items = _rows(200, 32, 14) + [b"T" * 32, b"G" + b"T" * 31]
    _check(rg, items, [0] * len(items), 32)
    with pytest.raises(_lib.RogtkError) as e:
        rg.umi_correct(_bin(items), 32, 1, method="directional", groups=_u32([0] * (len(items) - 1) + [1]))
    assert e.value.code == _lib.ROGTK_E_UNSUPPORTED


@pytest.mark.parametrize("top", [1, 255, 256, 0x80000000])
def test_sort_width_of_the_largest_key(rg, top):
    """bit widths 1, 8, 9 and 32"""
    items = _rows(400, 12, top % 97)
    rng = np.random.default_rng(2)
    keys = [int(k) for k in rng.integers(0, top + 1, len(items))]
    keys[0] = top
    _check(rg, items, keys, 12)


# ------------------------------------------------------------ shapes around the wave and tile
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 4097])
@pytest.mark.parametrize("n_groups", ["1", "2", "n/3"])
def test_row_counts(rg, n, n_groups):
    items = _rows(n, 6, n)
    g = {"1": 1, "2": 2, "n/3": max(1, n // 3)}[n_groups]
    keys = np.random.default_rng(n).integers(0, g, n)
    _check(rg, items, keys, 6)


def test_a_run_longer_than_a_workgroup_next_to_single_rows(rg):
    big = b"ACGTACGTACGT"
    items = [big] * 5000 + [b"ACGTACGTACGA"] * 40
    keys = [3] * 5000 + list(range(100, 140))
    perm = np.random.default_rng(1).permutation(len(items))
    _, want = _check(rg, [items[j] for j in perm], [keys[j] for j in perm], 12)
    assert want[1] == 41 and (big, 5000, 1, 3) in want[2]


def _walk(L, steps, seed):
    rng = np.random.default_rng(seed)
    cur = bytearray(bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)]))
    out, seen = [bytes(cur)], {bytes(cur)}
    while len(out) < steps:
        q = int(rng.integers(0, L))
        nxt = bytearray(cur)
        nxt[q] = int(rng.choice([b for b in b"ACGT" if b != cur[q]]))
        if bytes(nxt) in seen:
            continue
        cur = nxt
        seen.add(bytes(cur))
        out.append(bytes(cur))
    return out


def test_a_long_path_in_one_group_a_short_one_in_another(rg):
    walk = _walk(16, 300, 9)
    items = walk + [walk[0]] * 4 + [walk[1]]
    keys = [6] * 300 + [2] * 5
    _, want = _check(rg, items, keys, 16)
    assert want[1] == 2 and want[2] == [(walk[0], 5, 2, 2), (min(walk), 300, 300, 6)]
    assert 1 <= _rounds() <= 300


# ------------------------------------------------------------ irregular rows, degenerate columns
def test_irregular_rows(rg):
    items = [b"ACGN", b"ACGN", b"ACGN", b"ACGN", b"ACGT", b"", b"acgt", None, b"ACGTA", b""]
    keys = [9, 2, 9, 0xFFFFFFFF, 2, 2, 0, 1, 0, 9]
    _, (ids, k, table, _) = _check(rg, items, keys, 4)
    assert k == 8 and ids == [6, 4, 6, 7, 0, 3, 2, None, 1, 5]  # regular first, then (key, bytes)
    only = [b"ACGN", b"AC", b"ACGN", b"N", b"AC"]
    _, (ids, k, _, _) = _check(rg, only, [1, 0, 0, 1, 0], 4)
    assert k == 4 and ids == [2, 0, 1, 3, 0] and _rounds() == 0


def test_degenerate_columns(rg):
    res = rg.umi_correct(_bin([None] * 5), 4, 1, method="directional", groups=_u32([1, 2, 3, 4, 5]))
    assert res.n_clusters == 0 and len(res.clusters) == 0 and _table4(res.clusters) == []
    assert res.corrected.to_pylist() == [None] * 5 and res.cluster_id.to_pylist() == [None] * 5
    for col in (_bin([]), pa.chunked_array([], type=pa.large_string())):
        res = rg.umi_correct(col, 4, 1, method="directional", groups=np.zeros(0, np.uint32))
        assert res.n_clusters == 0 and _table4(res.clusters) == [] and len(res.corrected) == 0
        assert rg.umi_cluster(col, 4, 1, method="directional", groups=np.zeros(0, np.int64))[1] == 0


def test_umi_len_40_makes_every_string_irregular(rg):
    items = _rows(200, 6, 12)
    keys = [i % 3 for i in range(len(items))]
    _, want = _check(rg, items, keys, 40)
    assert want[1] == len({(k, x) for k, x in zip(keys, items) if x is not None}) and _rounds() == 0


# ------------------------------------------------------------ max_distance 0, invariance
@pytest.mark.parametrize("method", ["directional", "cluster"])
def test_max_distance_0_is_the_distinct_pairs(rg, method):
    items = _rows(700, 6, 21)
    keys = np.random.default_rng(4).integers(0, 5, len(items))
    _, want = _check(rg, items, keys, 6, 0, method)
    assert want[1] == len({(int(k), x) for k, x in zip(keys, items) if x is not None}) and _rounds() == 0


def test_row_order_and_chunking_invariance(rg):
    items = _rows(3000, 7, 30)
    keys = np.random.default_rng(6).integers(0, 40, len(items)).astype(np.uint32)
    base, want = _check(rg, items, keys, 7)
    perm = np.random.default_rng(5).permutation(len(items))
    got = rg.umi_correct(_bin([items[j] for j in perm]), 7, 1, method="directional", groups=keys[perm])
    assert _table4(got.clusters) == want[2]
    assert got.cluster_id.to_pylist() == [want[0][j] for j in perm]
    assert as_bytes(got.corrected) == [want[3][j] for j in perm]
    cuts = [0, 7, 7, 1000, len(items)]
    chunked = pa.chunked_array([_bin(items[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
    kchunks = pa.chunked_array([pa.array(keys[a:b]) for a, b in zip([0, 1500], [1500, len(items)])])
    _same(rg.umi_correct(chunked, 7, 1, method="directional", groups=kchunks), want, items)


# ------------------------------------------------------------ refusals, the default path
def test_refusals(rg):
    from rogtk_amd import _lib, plugin

    col, n = _bin(D.KNOWN_ROWS), len(D.KNOWN_ROWS)
    good = _u32(G.KNOWN_KEYS)
    for fn in (rg.umi_correct, rg.umi_cluster):
        with pytest.raises(_lib.RogtkError) as e:
            fn(col, 4, 1, method="cluster", groups=good)
        assert e.value.code == _lib.ROGTK_E_UNSUPPORTED and 'method="directional"' in str(e.value)
        with pytest.raises(_lib.RogtkError) as e:
            fn(col, 4, 2, method="directional", groups=good)
        assert e.value.code == _lib.ROGTK_E_UNSUPPORTED
        with pytest.raises(ValueError):
            fn(col, 4, 1, method="nonsense", groups=good)
        bad = [good[:-1], pa.array([None] + G.KNOWN_KEYS[1:], type=pa.int64()),
               np.array([-1] + G.KNOWN_KEYS[1:], dtype=np.int64), np.array([1 << 32] + G.KNOWN_KEYS[1:], dtype=np.int64),
               np.zeros(n, dtype=np.float64)]
        for groups in bad:
            with pytest.raises(ValueError):
                fn(col, 4, 1, method="directional", groups=groups)
    # the library's own checks come before any device work: no buffer is looked at
    nk = ctypes.c_int64(0)
    for method, maxd, code in ((0, 1, _lib.ROGTK_E_UNSUPPORTED), (1, 2, _lib.ROGTK_E_UNSUPPORTED),
                               (2, 1, _lib.ROGTK_E_INVALID)):
        with pytest.raises(_lib.RogtkError) as e:
            _lib.call("rogtk_umi_cluster_grouped_dev", None, None, None, n, None, 4, method, maxd, None,
                      ctypes.byref(nk), None, None, None)
        assert e.value.code == code
        if method == 0:
            assert 'method="directional"' in str(e.value)
    # the plugin's key series
    strs = pa.array([None if x is None else x.decode() for x in D.KNOWN_ROWS], type=pa.string())
    for keys in (pa.array([None] + G.KNOWN_KEYS[1:], type=pa.int64()), pa.array([-1] + G.KNOWN_KEYS[1:], type=pa.int64()),
                 pa.array([1 << 32] + G.KNOWN_KEYS[1:], type=pa.uint64()), pa.array(G.KNOWN_KEYS[1:], type=pa.int64()),
                 pa.array([0.5] * n, type=pa.float64())):
        with pytest.raises(_lib.RogtkError):
            plugin.call_plugin("umi_correct_expr", [strs, keys], {"umi_len": 4, "method": "directional"})
    with pytest.raises(_lib.RogtkError) as e:
        plugin.call_plugin("umi_correct_expr", [strs, pa.array(G.KNOWN_KEYS, type=pa.int64())], {"umi_len": 4})
    assert "directional" in str(e.value)


def test_default_path_untouched(rg):
    for method in ("cluster", "directional"):
        res = rg.umi_correct(_bin(D.KNOWN_ROWS), 4, 1, method=method)
        assert [f.name for f in res.clusters.type] == ["representative", "n_reads", "n_distinct"]
    assert table_of(rg.umi_correct(_bin(D.KNOWN_ROWS), 4, 1, method="directional").clusters) == D.KNOWN_TABLE
