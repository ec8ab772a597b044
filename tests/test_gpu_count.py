"""The UMI count matrix on the GPU (rogtk_amd/csrc/count_matrix.hip) against the
restatements of tests/count_spec.py: exact equality of every output (entry_cell, entry_feature,
n_umis, n_reads, totals, indptr).

Shapes are small and sit where the kernels can break: row counts around a wave and the flag /
emit tile (taken from the library's own constants), entries and runs of one molecule that cross
tile edges, entries that meet exactly at one, every row its own entry, one triple for all rows,
rows skipped for each cause, zero-width fields, the 64-bit key, a capacity below the entry count,
unaligned columns, a dirty temp buffer used twice, and a stream of the caller's."""
from __future__ import annotations

import ctypes

import numpy as np
import pyarrow as pa
import pytest

import count_spec as S

pytestmark = pytest.mark.gpu

NO_ID = S.NO_ID
SENTINEL = 0x5EED5EED
FAR = -7


@pytest.fixture(scope="module")
def rg():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import rogtk_amd

    assert rogtk_amd.device_count() >= 1
    return rogtk_amd


@pytest.fixture(scope="module")
def tile(rg):
    from rogtk_amd import count

    return count.geometry()["tile"]


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def _want(c, f, m, sizes, capacity=None, indptr=True):
    want = S.count_lexsort(c, f, m, *sizes, capacity, indptr)
    if len(c) <= 20_000:
        assert S.same(want, S.count_dict(c, f, m, *sizes, capacity, indptr))
    return want


def _check_host(rg, c, f, m, sizes):
    """The host entry (Arrow out) against restatement (b); restatement (a) on small cases."""
    c, f, m = _u32(c), _u32(f), _u32(m)
    want = _want(c, f, m, sizes)
    got = rg.count_matrix(c, f, m, *sizes)
    for name in ("cell", "feature", "n_umis", "n_reads"):
        arr = getattr(got, name)
        assert arr.type == pa.uint32() and arr.null_count == 0
        assert np.array_equal(arr.to_numpy(), getattr(want, name)), name
    assert got.indptr.type == pa.int64() and np.array_equal(got.indptr.to_numpy(), want.indptr)
    assert [got.nnz, got.n_live, got.n_molecules_counted] == want.totals.tolist()
    assert got.shape == (sizes[0], sizes[1])
    return want


class Level1:
    """rogtk_count_matrix on torch buffers: outputs pre-filled so that what the call does not
    write shows, nullable outputs left out on request, the temp buffer the caller's and dirty."""

    def __init__(self, n, sizes, capacity, temp_fill=0xA5):
        import torch

        from rogtk_amd import _lib

        self.torch, self.lib, self.n, self.sizes, self.cap = torch, _lib, n, tuple(sizes), capacity
        tb = ctypes.c_int64(0)
        _lib.call("rogtk_count_matrix_temp_bytes", n, *self.sizes, capacity, ctypes.byref(tb))
        self.tb = tb.value
        self.temp = torch.full((self.tb,), temp_fill, dtype=torch.uint8, device="cuda")

    def __call__(self, c, f, m, n_reads=True, indptr=True, shift=False, stream=None):
        torch, n, cap = self.torch, self.n, self.cap
        assert len(c) == n

        def dev(a):
            if not shift:
                return torch.from_numpy(_u32(a).view(np.int32)).cuda()
            t = torch.from_numpy(np.concatenate([[0], _u32(a)]).astype(np.uint32).view(np.int32)).cuda()[1:]
            assert (t.data_ptr() % 16 == 4 or not t.numel()) and t.is_contiguous()  # the loads' scalar path
            return t

        cols = [dev(c), dev(f), dev(m)]
        fill = np.array(SENTINEL, dtype=np.uint32).view(np.int32).item()
        out = {
            "cell": torch.full((cap,), fill, dtype=torch.int32, device="cuda"),
            "feature": torch.full((cap,), fill, dtype=torch.int32, device="cuda"),
            "n_umis": torch.full((cap,), fill, dtype=torch.int32, device="cuda"),
            "n_reads": torch.full((cap,), fill, dtype=torch.int32, device="cuda") if n_reads else None,
            "indptr": torch.full((self.sizes[0] + 1,), FAR, dtype=torch.int64, device="cuda") if indptr else None,
            "totals": torch.full((3,), FAR, dtype=torch.int64, device="cuda"),
        }
        p = lambda t: None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())
        s = stream if stream is not None else torch.cuda.current_stream()
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())  # the fills and uploads above
        self.lib.call("rogtk_count_matrix", *(p(t) for t in cols), n, *self.sizes, p(out["cell"]), p(out["feature"]),
                      p(out["n_umis"]), p(out["n_reads"]), cap, p(out["indptr"]), p(out["totals"]), p(self.temp),
                      self.tb, ctypes.c_void_p(s.cuda_stream))
        s.synchronize()
        torch.cuda.synchronize()
        host = {}
        for name, t in out.items():
            host[name] = None if t is None else t.cpu().numpy()
            if host[name] is not None and name not in ("indptr", "totals"):
                host[name] = host[name].view(np.uint32)
        return host

    def check(self, got, want):
        """want: the restatement cut at this capacity."""
        w = want.cell.size
        assert w == min(int(want.totals[0]), self.cap)
        assert np.array_equal(got["totals"], want.totals)
        for name in ("cell", "feature", "n_umis", "n_reads"):
            if got[name] is None:
                continue
            assert np.array_equal(got[name][:w], getattr(want, name)), name
            assert (got[name][w:] == SENTINEL).all(), name  # left untouched
        if got["indptr"] is not None:
            assert np.array_equal(got["indptr"], want.indptr)


def _level1(c, f, m, sizes, capacity=None, **kw):
    c, f, m = _u32(c), _u32(f), _u32(m)
    n = c.size
    cap = n if capacity is None else capacity
    run = Level1(n, sizes, cap)
    want = _want(c, f, m, sizes, cap, kw.get("indptr", True))
    got = run(c, f, m, **kw)
    run.check(got, want)
    return want, got


def _random_columns(rng, n, sizes, skip=0.1):
    """Ids drawn a little past their sizes and some 0xFFFFFFFF: all three skip causes, repeats."""
    cols = []
    for k in sizes:
        v = rng.integers(0, k + max(1, k // 8), size=n).astype(np.uint32)
        v[rng.random(n) < skip / 3] = NO_ID
        cols.append(v)
    return cols


def test_row_counts_at_the_kernels_boundaries(rg, tile):
    rng = np.random.default_rng(1)
    for n in sorted({0, 1, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 1}):
        sizes = (max(1, n // 40), 7, max(1, n // 9))
        c, f, m = _random_columns(rng, n, sizes)
        _check_host(rg, c, f, m, sizes)
        _level1(c, f, m, sizes)
        _level1(c, f, m, sizes, shift=True)  # columns at offset 1: the scalar loads


def test_one_entry_whose_rows_span_three_tiles(rg, tile):
    n = 3 * tile + 40
    rng = np.random.default_rng(2)
    c = np.full(n, 5, np.uint32)
    f = np.full(n, 3, np.uint32)
    c[:20], c[-20:] = 1, 9          # a short entry in front and one behind
    m = rng.integers(0, 50, size=n).astype(np.uint32)
    want = _check_host(rg, c, f, m, (12, 4, 50))
    assert want.n_reads.tolist() == [20, n - 40, 20] and want.n_umis[1] == 50
    _level1(c, f, m, (12, 4, 50))


def test_one_triple_repeated_across_a_tile_edge_is_one_molecule(rg, tile):
    # sorted order: tile - 3 rows of molecule 0, then 6 rows of molecule 1 (three on each side of the
    # edge), then molecule 2
    m = np.concatenate([np.zeros(tile - 3), np.ones(6), np.full(tile, 2)]).astype(np.uint32)
    n = m.size
    c, f = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    perm = np.random.default_rng(3).permutation(n)
    want, _ = _level1(c[perm], f[perm], m[perm], (1, 1, 3))
    assert want.n_umis.tolist() == [3] and want.n_reads.tolist() == [n]
    _check_host(rg, c[perm], f[perm], m[perm], (1, 1, 3))


def test_two_entries_meet_exactly_at_a_tile_edge(rg, tile):
    # (0, 4) fills the first tile, (0, 5) starts at the first position of the second
    f = np.concatenate([np.full(tile, 4), np.full(tile // 2, 5)]).astype(np.uint32)
    n = f.size
    c = np.zeros(n, np.uint32)
    m = (np.arange(n) % 17).astype(np.uint32)
    want, _ = _level1(c, f, m, (1, 6, 17))
    assert want.feature.tolist() == [4, 5] and want.n_reads.tolist() == [tile, tile // 2]
    assert want.n_umis.tolist() == [17, 17]
    _check_host(rg, c[::-1], f[::-1], m[::-1], (1, 6, 17))


def test_every_row_its_own_entry(rg, tile):
    n = 2 * tile + 77
    rng = np.random.default_rng(4)
    pair = rng.permutation(n)
    c, f = (pair // 64).astype(np.uint32), (pair % 64).astype(np.uint32)
    m = rng.integers(0, 9, size=n).astype(np.uint32)
    sizes = (n // 64 + 1, 64, 9)
    want = _check_host(rg, c, f, m, sizes)
    assert int(want.totals[0]) == n and (want.n_umis == 1).all() and (want.n_reads == 1).all()
    _level1(c, f, m, sizes)


def test_all_rows_one_triple(rg, tile):
    n = 2 * tile + 5
    c, f, m = np.full(n, 2, np.uint32), np.full(n, 1, np.uint32), np.full(n, 6, np.uint32)
    want = _check_host(rg, c, f, m, (3, 2, 7))
    assert want.totals.tolist() == [1, n, 1] and want.n_reads.tolist() == [n]
    _level1(c, f, m, (3, 2, 7))


def test_skipped_rows(rg, tile):
    n = tile + 300
    rng = np.random.default_rng(5)
    sizes = (30, 11, 200)
    base = [rng.integers(0, k, size=n).astype(np.uint32) for k in sizes]
    full = _check_host(rg, *base, sizes)
    assert int(full.totals[1]) == n
    for which in (0, 1, 2):  # each cause alone: past the size, exactly the size, 0xFFFFFFFF
        cols = [b.copy() for b in base]
        r = rng.random(n)
        cols[which][r < 0.1] = NO_ID
        cols[which][(r >= 0.1) & (r < 0.2)] = sizes[which]
        cols[which][(r >= 0.2) & (r < 0.3)] = sizes[which] + 1000
        want = _check_host(rg, *cols, sizes)
        assert int(want.totals[1]) == int((r >= 0.3).sum()) < n
        _level1(*cols, sizes)
    mixed = [b.copy() for b in base]
    for which in (0, 1, 2):
        mixed[which][rng.random(n) < 0.15] = rng.choice(np.array([NO_ID, sizes[which], 0xFFFFFFFE], dtype=np.uint32))
    _check_host(rg, *mixed, sizes)
    _level1(*mixed, sizes)
    # nothing but skipped rows
    nothing = [np.full(n, NO_ID, np.uint32), base[1], base[2]]
    want = _check_host(rg, *nothing, sizes)
    assert want.totals.tolist() == [0, 0, 0] and (want.indptr == 0).all()
    _level1(*nothing, sizes)


def test_no_rows_or_a_size_of_zero(rg):
    for n, sizes in ((0, (0, 0, 0)), (0, (5, 3, 2)), (70, (0, 3, 2)), (70, (5, 0, 2)), (70, (5, 3, 0))):
        c = np.zeros(n, np.uint32)
        want, got = _level1(c, c, c, sizes)
        assert got["totals"].tolist() == [0, 0, 0] and (got["indptr"] == 0).all()
        assert got["indptr"].size == sizes[0] + 1
        _check_host(rg, c, c, c, sizes)


def test_empty_leading_interior_and_trailing_cells(rg, tile):
    n = tile + 9
    rng = np.random.default_rng(6)
    c = rng.choice(np.array([3, 4, 7, 8, 12], dtype=np.uint32), size=n)  # 0-2, 5-6, 9-11 and 13-19 stay empty
    f = rng.integers(0, 5, size=n).astype(np.uint32)
    m = rng.integers(0, 40, size=n).astype(np.uint32)
    want = _check_host(rg, c, f, m, (20, 5, 40))
    steps = np.diff(want.indptr)
    assert steps[[0, 1, 2, 5, 6, 9, 10, 11, 13, 19]].tolist() == [0] * 10 and (steps[[3, 4, 7, 8, 12]] == 5).all()
    _level1(c, f, m, (20, 5, 40))


def test_nullable_outputs_left_out(rg, tile):
    n = tile + 100
    rng = np.random.default_rng(7)
    sizes = (9, 9, 30)
    c, f, m = _random_columns(rng, n, sizes)
    for n_reads, indptr in ((False, True), (True, False), (False, False)):
        _level1(c, f, m, sizes, n_reads=n_reads, indptr=indptr)
    got = rg.count_matrix(c, f, m, *sizes, indptr=False)
    assert got.indptr is None and np.array_equal(got.n_umis.to_numpy(), S.count_lexsort(c, f, m, *sizes).n_umis)


def test_capacity_below_the_entry_count(rg, tile):
    n = 2 * tile + 50
    rng = np.random.default_rng(8)
    sizes = (40, 25, 60)
    c, f, m = _random_columns(rng, n, sizes)
    full = S.count_lexsort(c, f, m, *sizes)
    entries = int(full.totals[0])
    assert entries > 600
    for cap in (0, 1, entries // 2, entries - 1, entries, entries + 3):
        want, got = _level1(c, f, m, sizes, capacity=cap)
        w = min(cap, entries)
        assert int(got["totals"][0]) == entries and int(got["indptr"][-1]) == w  # the true count; the cut
        if w:
            assert got["n_reads"][w - 1] == full.n_reads[w - 1] and got["n_umis"][w - 1] == full.n_umis[w - 1]
        assert (got["cell"][w:] == SENTINEL).all() and (got["n_umis"][w:] == SENTINEL).all()


def test_host_entry_with_its_default_capacity(rg):
    """capacity < 0: min(n, n_cells x n_features), here both ways round; the arrays' tails stay."""
    from rogtk_amd import _lib

    rng = np.random.default_rng(15)
    for n, sizes in ((500, (3, 4, 50)), (40, (30, 30, 5)), (300, ((1 << 32) - 1, (1 << 31) + 5, 1))):
        cap = min(n, sizes[0] * sizes[1])
        c, f, m = (rng.integers(0, min(k, 40) + 1, size=n).astype(np.uint32) for k in sizes)
        want = _want(c, f, m, sizes, indptr=False)
        out = [np.full(cap + 2, SENTINEL, np.uint32) for _ in range(4)]
        totals = np.full(3, FAR, np.int64)
        _lib.call("rogtk_count_matrix_host", *(_lib.ptr(x) for x in (c, f, m)), n, *sizes, *(_lib.ptr(a) for a in out),
                  -1, None, _lib.ptr(totals))
        assert np.array_equal(totals, want.totals) and want.cell.size <= cap
        for a, name in zip(out, ("cell", "feature", "n_umis", "n_reads")):
            assert np.array_equal(a[:want.cell.size], getattr(want, name)), name
            assert (a[want.cell.size:] == SENTINEL).all(), name


def test_zero_width_fields(rg, tile):
    n = tile + 33
    rng = np.random.default_rng(9)
    for sizes in ((50, 1, 20), (50, 20, 1), (50, 1, 1), (1, 1, 1)):
        c, f, m = _random_columns(rng, n, sizes, skip=0.2)
        want = _check_host(rg, c, f, m, sizes)
        if sizes[2] == 1:
            assert (want.n_umis == 1).all()
        _level1(c, f, m, sizes)


def test_the_64_bit_key(rg):
    sizes = ((1 << 24) - 1, 1 << 16, 1 << 24)
    assert S.key_bits(*sizes) == 64
    top = [s - 1 for s in sizes]
    rows = [(top[0], top[1], top[2]), (top[0], top[1], top[2]), (top[0], top[1], 0), (top[0], 0, top[2]),
            (0, top[1], top[2]), (0, 0, 0), (top[0], top[1], top[2] - 1), (sizes[0], 0, 0), (0, sizes[1], 0),
            (0, 0, sizes[2]), (NO_ID, NO_ID, NO_ID), (top[0] - 1, top[1], top[2])]
    c, f, m = (np.array(col, dtype=np.uint32) for col in zip(*rows))
    want, got = _level1(c, f, m, sizes, indptr=False)
    assert want.totals.tolist() == [5, 8, 7]
    assert got["cell"][4] == top[0] and got["feature"][4] == top[1] and got["n_umis"][4] == 3


def test_two_calls_in_a_row_on_one_temp(rg, tile):
    n = 2 * tile + 100
    sizes = (20, 20, 300)
    rng = np.random.default_rng(10)
    run = Level1(n, sizes, n, temp_fill=0xFF)  # the first call meets garbage, the later ones a call's leftovers
    for _ in range(2):
        c, f, m = _random_columns(rng, n, sizes)
        run.check(run(c, f, m), _want(c, f, m, sizes, n))
    z = np.zeros(n, np.uint32)  # one entry: every temporary of the earlier calls is stale
    run.check(run(z, z, z), _want(z, z, z, sizes, n))


def test_a_call_on_a_non_default_stream(rg, tile):
    import torch

    n = tile + 500
    sizes = (15, 15, 100)
    c, f, m = _random_columns(np.random.default_rng(11), n, sizes)
    _level1(c, f, m, sizes, stream=torch.cuda.Stream())


def test_device_tensors_in_the_python_call(rg, tile):
    import torch

    n = tile + 200
    sizes = (12, 8, 90)
    c, f, m = _random_columns(np.random.default_rng(12), n, sizes, skip=0.0)
    c[:5] = NO_ID
    dev = lambda a: torch.from_numpy(a.view(np.int32)).cuda()
    for given in (sizes, (-1, -1, -1)):
        host = rg.count_matrix(c, f, m, *given)
        got = rg.count_matrix(dev(c), dev(f), dev(m), *given)
        assert got.shape == host.shape and [got.nnz, got.n_live, got.n_molecules_counted] == [
            host.nnz, host.n_live, host.n_molecules_counted]
        for name in ("cell", "feature", "n_umis", "n_reads"):
            t = getattr(got, name)
            assert t.device.type == "cuda" and t.dtype == torch.int32 and t.numel() == host.nnz
            assert np.array_equal(t.cpu().numpy().view(np.uint32), getattr(host, name).to_numpy()), name
        assert np.array_equal(got.indptr.cpu().numpy(), host.indptr.to_numpy())
        assert (got.to_scipy() != host.to_scipy()).nnz == 0
        assert np.array_equal(got.umis_per_cell(), host.umis_per_cell())
    want = S.count_lexsort(c, f, m, *sizes)
    host = rg.count_matrix(c, f, m, *sizes)
    assert np.array_equal(host.umis_per_cell(), np.bincount(want.cell, weights=want.n_umis, minlength=12))
    assert np.array_equal(host.features_per_cell(), np.diff(want.indptr))


def test_umi_count_against_cluster_then_restatement(rg):
    from conftest import irregular_families

    items = irregular_families(31, 60, 8)
    n = len(items)
    assert 100 < n < 600 and any(x is None for x in items)
    rng = np.random.default_rng(13)
    col = pa.array(items, type=pa.large_binary())
    n_cells, n_features = 6, 4
    cells = rng.integers(0, n_cells + 1, size=n).astype(np.uint32)      # n_cells itself: out of range
    feats = rng.integers(0, n_features, size=n).astype(np.uint32)
    feats[rng.random(n) < 0.1] = NO_ID                                   # a null gene
    ok = (cells < n_cells) & (feats < n_features)
    key = np.where(ok, cells.astype(np.uint64) * n_features + feats, NO_ID).astype(np.uint32)
    for method, md in (("directional", 1), ("cluster", 0)):
        ids, k, _ = rg.umi_cluster(col, 8, md, method, key)
        res = rg.umi_count(col, 8, cells, feats, n_cells, n_features, md, method)
        assert res.n_clusters == k and res.cluster_id.equals(ids)
        plain = np.asarray(ids.fill_null(NO_ID).to_numpy(zero_copy_only=False), dtype=np.uint32)
        want = _want(cells, feats, plain, (n_cells, n_features, k))
        assert np.array_equal(res.cell.to_numpy(), want.cell) and np.array_equal(res.feature.to_numpy(), want.feature)
        assert np.array_equal(res.n_umis.to_numpy(), want.n_umis) and np.array_equal(res.n_reads.to_numpy(), want.n_reads)
        assert np.array_equal(res.indptr.to_numpy(), want.indptr)
        nulls = np.array([x is None for x in items])
        assert res.n_live == int((ok & ~nulls).sum()) and res.shape == (n_cells, n_features)
        assert res.to_scipy().sum() == res.n_molecules_counted == int(want.totals[2])


def test_barcode_keys_as_the_cell_column(rg):
    rng = np.random.default_rng(14)
    alphabet = np.frombuffer(b"ACGT", np.uint8)
    white = sorted({bytes(rng.choice(alphabet, 10)) for _ in range(40)})
    wl = rg.BarcodeWhitelist(pa.array(white, type=pa.large_binary()))
    n = 700
    cbcs = [white[int(i)] for i in rng.integers(0, len(white), size=n)]
    for i in range(0, n, 9):
        cbcs[i] = b"N" * 10          # no match: key 0xFFFFFFFF
    cbcs[5] = None
    keys = wl.correct(pa.array(cbcs, type=pa.large_binary())).keys
    assert keys.dtype == np.uint32 and (keys == NO_ID).sum() >= n // 9
    feats = rng.integers(0, 6, size=n).astype(np.uint32)
    mols = rng.integers(0, 25, size=n).astype(np.uint32)
    sizes = (len(white), 6, 25)
    want = _check_host(rg, keys, feats, mols, sizes)
    assert int(want.totals[1]) == int((keys != NO_ID).sum())


@pytest.mark.parametrize("first_chunk", ["distinct", "one_triple"])
def test_the_tile_scan_carries_across_its_chunks(rg, tile, first_chunk):
    """More flag tiles than the scan's one workgroup takes at once. distinct: every row its own
    entry, so the second chunk's offsets are its position. one_triple: the first chunk's sorted
    positions hold one triple, so the second chunk's entry and molecule offsets are 1."""
    from rogtk_amd import count

    scan_block = count.geometry()["scan_block"]
    n = (scan_block + 1) * tile + 5
    row = np.arange(n, dtype=np.int64)
    c, f = row // 1000, row % 1000
    sizes = (int(c[-1]) + 1, 1000, 1 << 20)  # 12 + 10 + 20 bits of key
    m = row * 7919 % sizes[2]
    if first_chunk == "one_triple":
        same = scan_block * tile  # (0, 0, 0) sorts first; behind it (1 + j // 1000, j % 1000) for j = 0, 1, ..
        c, f, m = c + 1, f.copy(), m.copy()
        c[:same], f[:same], m[:same] = 0, 0, 0
        c[same:], f[same:] = 1 + (row[same:] - same) // 1000, (row[same:] - same) % 1000
    perm = np.random.default_rng(16).permutation(n)
    want, got = _level1(c[perm], f[perm], m[perm], sizes)  # every output, indptr and totals included
    entries = n if first_chunk == "distinct" else n - scan_block * tile + 1
    assert want.totals.tolist() == [entries, n, entries]
    assert got["totals"].tolist() == [entries, n, entries] and int(got["indptr"][-1]) == entries
