"""UMI deduplication on the GPU (rogtk_amd/csrc/dedup.hip) against the
restatements of tests/dedup_spec.py: exact equality of all six outputs (best_row, best_score,
n_reads, the keep words, the kept rows, n_kept).

Shapes are small and sit where the kernels can break: row counts around a wave, a keep word, the
select tile and the compaction tile (taken from the library's own constants), id layouts that
take the uniform-wave shortcut, the LDS table, its overflow to the global tables and one slot's
probe chain, and scores at both ends of u32 with ties across tile edges and past row 65,535."""
from __future__ import annotations

import ctypes
import itertools

import numpy as np
import pyarrow as pa
import pytest

import dedup_spec as S

pytestmark = pytest.mark.gpu

NO_ID = S.NO_ID


@pytest.fixture(scope="module")
def rg():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import rogtk_amd

    assert rogtk_amd.device_count() >= 1
    return rogtk_amd


@pytest.fixture(scope="module")
def geo(rg):
    from rogtk_amd import dedup

    return dedup.geometry()


def _check_host(rg, ids, score, k):
    """The host entry (Arrow / numpy out) against restatement (b); restatement (a) on small cases."""
    ids = np.asarray(ids, dtype=np.uint32)
    want = S.best_lexsort(ids, score, k)
    if ids.size <= 20_000:
        assert S.same(want, S.best_dict(ids, score, k))
    got = rg.cluster_best_rows(ids, score, k)
    n = ids.size
    assert got.keep.type == pa.bool_() and len(got.keep) == n and got.keep.null_count == 0
    assert got.rows.type == pa.int64()
    assert got.best.type == pa.struct([("best_row", pa.int64()), ("best_score", pa.uint32()), ("n_reads", pa.uint32())])
    words = np.frombuffer(got.keep.buffers()[1], dtype=np.uint64, count=(n + 63) // 64)
    assert np.array_equal(words, want.keep_words)
    assert np.array_equal(np.asarray(got.keep.to_numpy(zero_copy_only=False), dtype=bool), want.keep)
    assert np.array_equal(got.rows.to_numpy(), want.rows)
    assert got.n_kept == want.n_kept
    assert np.array_equal(got.best.field("best_row").to_numpy(), want.best_row)
    assert np.array_equal(got.best.field("best_score").to_numpy(), want.best_score)
    assert np.array_equal(got.best.field("n_reads").to_numpy(), want.n_reads)
    return want


class Level1:
    """rogtk_cluster_best_rows on torch buffers: outputs pre-filled so that what the call does
    not write shows, nullable outputs left out on request, the temp buffer the caller's."""

    SENTINEL = -7

    def __init__(self, n, k, temp_fill=0xA5):
        import torch

        from rogtk_amd import _lib

        self.torch, self.lib, self.n, self.k = torch, _lib, n, k
        tb = ctypes.c_int64(0)
        _lib.call("rogtk_cluster_best_temp_bytes", n, k, ctypes.byref(tb))
        self.tb = tb.value
        self.temp = torch.full((self.tb,), temp_fill, dtype=torch.uint8, device="cuda")

    def __call__(self, ids, score, best_score=True, n_reads=True, kept=True):
        torch, n, k = self.torch, self.n, self.k
        assert ids.size == n
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()
        d_ids = dev(ids)
        d_score = None if score is None else dev(score)
        out = {
            "best_row": torch.full((k,), 12345, dtype=torch.int64, device="cuda"),
            "best_score": torch.full((k,), 77, dtype=torch.int32, device="cuda") if best_score else None,
            "n_reads": torch.full((k,), 77, dtype=torch.int32, device="cuda") if n_reads else None,
            "keep": torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device="cuda"),  # all ones
            "kept": torch.full((min(n, k),), self.SENTINEL, dtype=torch.int64, device="cuda") if kept else None,
            "n_kept": torch.full((1,), -1, dtype=torch.int64, device="cuda") if kept else None,
        }
        p = lambda t: None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())
        self.lib.call("rogtk_cluster_best_rows", p(d_ids), p(d_score), n, k, p(out["best_row"]), p(out["best_score"]),
                      p(out["n_reads"]), p(out["keep"]), p(out["kept"]), p(out["n_kept"]), p(self.temp), self.tb,
                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return {name: None if t is None else t.cpu().numpy() for name, t in out.items()}

    def check(self, got, want, best_score=True, n_reads=True, kept=True):
        assert np.array_equal(got["best_row"], want.best_row)
        assert np.array_equal(got["keep"].view(np.uint64), want.keep_words)
        if best_score:
            assert np.array_equal(got["best_score"].view(np.uint32), want.best_score)
        if n_reads:
            assert np.array_equal(got["n_reads"].view(np.uint32), want.n_reads)
        if kept:
            m = int(got["n_kept"][0])
            assert m == want.n_kept
            assert np.array_equal(got["kept"][:m], want.rows)
            assert (got["kept"][m:] == self.SENTINEL).all()  # left untouched


def _scores(rng, n, hi=4):
    return rng.integers(0, hi, size=n).astype(np.uint32)


def _boundary_counts(geo):
    t, c = geo["select_tile"], geo["keep_tile"]
    return sorted({0, 1, 63, 64, 65, 127, 128, 129, t - 1, t, t + 1, c - 1, c, c + 1})


def test_row_counts_at_the_kernels_boundaries(rg, geo):
    rng = np.random.default_rng(1)
    for n in _boundary_counts(geo):
        k = max(1, n // 5)
        ids = rng.integers(0, k + 2, size=n).astype(np.uint32)  # k and k + 1: skipped
        if n:
            ids[n - 1] = 0
        score = _scores(rng, n)
        _check_host(rg, ids, score, k)
        _check_host(rg, ids, None, k)
        _check_host(rg, ids, score, 0)  # no cluster at all: every row skipped


def test_last_word_padding_is_written_as_zero(rg, geo):
    for n in (5, 64 * 3 + 5, geo["keep_tile"] + 1, 2 * geo["keep_tile"] + 63):
        rng = np.random.default_rng(n)
        k = 7
        ids = rng.integers(0, k, size=n).astype(np.uint32)
        score = _scores(rng, n)
        score[n - 1] = 100  # the last row wins its cluster
        want = S.best_lexsort(ids, score, k)
        assert want.keep[n - 1] and n % 64
        run = Level1(n, k)
        got = run(ids, score)  # keep_bits pre-filled with all ones
        run.check(got, want)
        last = int(got["keep"].view(np.uint64)[-1])
        assert last >> (n % 64) == 0 and (last >> ((n - 1) % 64)) & 1


def _n3(geo):
    return 3 * geo["select_tile"] + 17


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_id_for_all_rows(rg, geo, where):
    n, t = _n3(geo), geo["select_tile"]
    w = {"first": 5, "middle": t + t // 2 + 3, "last": n - 1}[where]
    ids = np.zeros(n, dtype=np.uint32)
    score = np.full(n, 3, dtype=np.uint32)
    score[w] = 9
    want = _check_host(rg, ids, score, 1)
    assert want.best_row.tolist() == [w] and want.n_reads.tolist() == [n]
    ids5 = np.full(n, 4, dtype=np.uint32)  # the same with empty ids around it
    assert _check_host(rg, ids5, score, 6).best_row.tolist() == [-1, -1, -1, -1, w, -1]


def test_every_row_its_own_id(rg, geo):
    n = _n3(geo)
    rng = np.random.default_rng(2)
    want = _check_host(rg, rng.permutation(n).astype(np.uint32), _scores(rng, n), n)
    assert want.n_kept == n
    _check_host(rg, np.arange(n, dtype=np.uint32), None, n)


def test_lds_table_overflows_to_the_global_tables(rg, geo):
    n = _n3(geo)
    k = geo["slots"] * geo["probes"] + 1000
    assert k > geo["slots"] * geo["probes"] and geo["select_tile"] > geo["slots"]
    rng = np.random.default_rng(3)
    ids = rng.integers(0, k, size=n).astype(np.uint32)  # shuffled: a tile holds more ids than slots
    assert np.unique(ids[:geo["select_tile"]]).size > geo["slots"]
    _check_host(rg, ids, _scores(rng, n), k)


def test_sorted_ids_with_run_boundaries_inside_a_wave(rg, geo):
    n = _n3(geo)
    rng = np.random.default_rng(4)
    lens = rng.choice([1, 5, 37, 256, 300, 700], size=n)
    ids = np.repeat(np.arange(n, dtype=np.uint32), lens)[:n]
    k = int(ids.max()) + 1
    _check_host(rg, ids, _scores(rng, n), k)
    _check_host(rg, ids, None, k)


def test_ids_that_hash_to_the_same_slot(rg, geo):
    n = _n3(geo)
    k = 600_000
    bits = geo["slots"].bit_length() - 1
    every = np.arange(k, dtype=np.uint64)
    home = ((every * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - bits)
    clash = every[home == home[12345]].astype(np.uint32)
    assert clash.size > 4 * geo["probes"]  # more ids than one slot's probe chain holds
    rng = np.random.default_rng(5)
    ids = rng.choice(clash, size=n)
    _check_host(rg, ids, _scores(rng, n), k)
    _check_host(rg, rng.choice(clash[:geo["probes"]], size=n), _scores(rng, n), k)  # the chain exactly full


def test_ids_with_gaps_and_skipped_rows(rg, geo):
    n = _n3(geo)
    rng = np.random.default_rng(6)
    k = 500
    ids = (2 * rng.integers(0, k // 2, size=n)).astype(np.uint32)  # odd ids have no rows
    want = _check_host(rg, ids, _scores(rng, n), k)
    assert (want.best_row[1::2] == -1).all() and (want.n_reads[1::2] == 0).all() and want.n_kept < k
    r = rng.random(n)
    ids[r < 0.2] = NO_ID
    ids[(r >= 0.2) & (r < 0.4)] = rng.integers(k, 2 * k, size=int(((r >= 0.2) & (r < 0.4)).sum())).astype(np.uint32)
    ids[(r >= 0.4) & (r < 0.45)] = 0xFFFFFFFE
    want = _check_host(rg, ids, _scores(rng, n), k)
    assert int(want.n_reads.sum()) == int((ids < k).sum()) < n
    _check_host(rg, np.full(n, NO_ID, dtype=np.uint32), None, k)  # nothing but null rows


def test_scores(rg, geo):
    n, t = _n3(geo), geo["select_tile"]
    rng = np.random.default_rng(7)
    k = 50
    ids = rng.integers(0, k, size=n).astype(np.uint32)
    want = _check_host(rg, ids, None, k)  # absent: the lowest row wins
    assert np.array_equal(want.best_row, [int(np.flatnonzero(ids == c)[0]) for c in range(k)])
    equal = _check_host(rg, ids, np.full(n, 41, np.uint32), k)  # all equal: the same rows
    assert np.array_equal(equal.keep, want.keep) and (equal.best_score == 41).all()
    both = rng.choice(np.array([0, 0xFFFFFFFF], dtype=np.uint32), size=n)  # both ends in every cluster
    want = _check_host(rg, ids, both, k)
    assert (want.best_score == 0xFFFFFFFF).all()
    _check_host(rg, ids, np.full(n, 0xFFFFFFFF, np.uint32), k)
    # the top score on both sides of a tile edge: the smaller row wins
    for rows in ([t - 1, t, 2 * t + 5], [t, 2 * t], [2 * t - 1, 2 * t, n - 1]):
        ids = rng.integers(1, k, size=n).astype(np.uint32)
        score = _scores(rng, n)
        ids[rows] = 0
        score[ids == 0] = 1
        score[rows] = 1000
        assert _check_host(rg, ids, score, k).best_row[0] == rows[0]


def test_tied_scores_past_row_65535(rg):
    n = 140_000
    rng = np.random.default_rng(8)
    ids = rng.integers(3, 40, size=n).astype(np.uint32)
    score = _scores(rng, n)
    for c, rows in enumerate(([65_535, 65_536], [66_000, 131_077], [65_540, 65_541, 139_999])):
        ids[rows] = c
        score[rows] = 5
    want = _check_host(rg, ids, score, 40)
    assert want.best_row[:3].tolist() == [65_535, 66_000, 65_540]


def test_level1_with_nullable_outputs_left_null(rg, geo):
    n = geo["keep_tile"] + 300
    rng = np.random.default_rng(9)
    k = 900  # some ids stay empty: n_kept < capacity, the tail of kept_rows keeps its sentinel
    ids = rng.integers(0, 700, size=n).astype(np.uint32)
    score = _scores(rng, n)
    run = Level1(n, k)
    for with_score, best_score, n_reads, kept in itertools.product([True, False], repeat=4):
        sc = score if with_score else None
        want = S.best_lexsort(ids, sc, k)
        assert want.n_kept < min(n, k)
        run.check(run(ids, sc, best_score, n_reads, kept), want, best_score, n_reads, kept)


def test_level1_without_rows_or_clusters(rg):
    for n, k in ((0, 0), (0, 5), (70, 0)):
        ids = np.arange(n, dtype=np.uint32)
        run = Level1(n, k)
        want = S.best_lexsort(ids, None, k)
        got = run(ids, None)
        run.check(got, want)
        assert int(got["n_kept"][0]) == 0
        assert (got["best_row"] == -1).all() and (got["best_score"] == 0).all() and (got["n_reads"] == 0).all()
        assert (got["keep"] == 0).all()


def test_level1_twice_on_the_same_temp_buffer(rg, geo):
    n = 2 * geo["keep_tile"] + 100
    k = 300
    rng = np.random.default_rng(10)
    run = Level1(n, k, temp_fill=0xFF)  # the first call meets garbage, the second the first call's tables
    for _ in range(3):
        ids = rng.integers(0, k + 3, size=n).astype(np.uint32)
        score = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        run.check(run(ids, score), S.best_lexsort(ids, score, k))
    low = np.zeros(n, dtype=np.uint32)  # every key smaller than what the tables held before
    run.check(run(low, None), S.best_lexsort(low, None, k))


@pytest.mark.parametrize("method,grouped", [("cluster", False), ("directional", False), ("directional", True)])
def test_umi_dedup_end_to_end(rg, method, grouped):
    from conftest import irregular_families

    items = irregular_families(21, 70, 8)
    n = len(items)
    assert 150 < n < 600 and any(x is None for x in items)
    rng = np.random.default_rng(11)
    col = pa.array(items, type=pa.large_binary())
    score = rng.integers(0, 61, size=n).astype(np.uint32)
    groups = rng.integers(0, 3, size=n).astype(np.uint32) if grouped else None
    ids, k, rl = rg.umi_cluster(col, 8, 1, method, groups)
    res = rg.umi_dedup(col, 8, score, 1, method, groups)
    assert res.n_clusters == k and res.umi_len == rl and res.cluster_id.equals(ids)
    plain = np.asarray(ids.fill_null(NO_ID).to_numpy(zero_copy_only=False), dtype=np.uint32)
    want = S.best_dict(plain, score, k)
    assert S.same(want, S.best_lexsort(plain, score, k))
    keep = np.asarray(res.keep.to_numpy(zero_copy_only=False), dtype=bool)
    assert res.keep.null_count == 0 and np.array_equal(keep, want.keep)
    assert np.array_equal(res.rows.to_numpy(), want.rows) and res.n_kept == want.n_kept == k
    assert np.array_equal(res.rows.to_numpy(), np.flatnonzero(keep))
    assert np.array_equal(res.best.field("best_row").to_numpy(), want.best_row)
    assert np.array_equal(res.best.field("best_score").to_numpy(), want.best_score)
    assert np.array_equal(res.best.field("n_reads").to_numpy(), want.n_reads)
    nulls = np.array([x is None for x in items])
    assert not keep[nulls].any()
    mask = rg.col(col).umi.dedup(8, score, 1, method, groups)
    assert mask.equals(res.keep)
    # without scores the first row of every cluster is kept
    first = rg.umi_dedup(col, 8, None, 1, method, groups)
    assert np.array_equal(first.rows.to_numpy(), S.best_dict(plain, None, k).rows)


def test_device_entry_matches_the_host_entry(rg, geo):
    import torch

    n = _n3(geo)
    rng = np.random.default_rng(12)
    k = 1000
    ids = rng.integers(0, k + 50, size=n).astype(np.uint32)
    ids[rng.random(n) < 0.05] = NO_ID
    score = _scores(rng, n, 61)
    dev = lambda a: torch.from_numpy(a.view(np.int32)).cuda()
    for sc, kk in ((score, k), (None, k), (score, -1)):
        host = rg.cluster_best_rows(ids, sc, kk)
        got = rg.cluster_best_rows(dev(ids), None if sc is None else dev(sc), kk)
        assert got.n_clusters == host.n_clusters and got.n_kept == host.n_kept
        assert got.keep.device.type == "cuda" and got.keep.dtype == torch.int64
        words = np.frombuffer(host.keep.buffers()[1], dtype=np.uint64, count=(n + 63) // 64)
        assert np.array_equal(got.keep.cpu().numpy().view(np.uint64), words)
        assert np.array_equal(got.rows.cpu().numpy(), host.rows.to_numpy())
        assert np.array_equal(got.best["best_row"].cpu().numpy(), host.best.field("best_row").to_numpy())
        assert np.array_equal(got.best["best_score"].cpu().numpy().view(np.uint32),
                              host.best.field("best_score").to_numpy())
        assert np.array_equal(got.best["n_reads"].cpu().numpy().view(np.uint32), host.best.field("n_reads").to_numpy())
    # an unaligned view takes the loads' scalar path: the same answers
    shifted = rg.cluster_best_rows(dev(np.concatenate([[0], ids]).astype(np.uint32))[1:].contiguous(), None, k)
    off1 = dev(np.concatenate([[0], ids]).astype(np.uint32))[1:]
    assert off1.data_ptr() % 16 == 4 and off1.is_contiguous()
    got = rg.cluster_best_rows(off1, dev(np.concatenate([[0], score]).astype(np.uint32))[1:], k)
    want = S.best_lexsort(ids, score, k)
    assert np.array_equal(got.rows.cpu().numpy(), want.rows)
    assert np.array_equal(got.best["best_row"].cpu().numpy(), want.best_row)
    assert np.array_equal(shifted.rows.cpu().numpy(), S.best_lexsort(ids, None, k).rows)


@pytest.mark.parametrize("first_chunk", ["kept", "empty"])
def test_the_tile_scan_carries_across_its_chunks(rg, geo, first_chunk):
    """More keep tiles than the scan's one workgroup takes at once: the offsets of the second chunk
    are the first chunk's total plus their own. empty: the first chunk holds skipped rows only, so
    it sums to 0 and every kept row lies behind it."""
    from rogtk_amd import count

    scan_block, tile = count.geometry()["scan_block"], geo["keep_tile"]
    n = (scan_block + 1) * tile + 5
    k = (n + 2) // 3
    ids = (np.arange(n, dtype=np.int64) // 3).astype(np.uint32)  # every tile of every chunk has kept rows
    if first_chunk == "empty":
        ids[:scan_block * tile] = k + (ids[:scan_block * tile] & 1)  # k and k + 1: skipped
    score = (np.arange(n, dtype=np.int64) * 2654435761 >> 7 & 3).astype(np.uint32)
    want = S.best_lexsort(ids, score, k)
    first = 0 if first_chunk == "kept" else scan_block * tile
    assert want.n_kept == k - first // 3 and int(want.rows[0]) >= first and int(want.rows[-1]) >= n - 3
    run = Level1(n, k)  # a dirty temp
    got = run(ids, score)
    run.check(got, want)  # all six outputs, exactly
    m = int(got["n_kept"][0])
    assert m == want.n_kept and (np.diff(got["kept"][:m]) > 0).all()
