"""GPU: the local connected-components kernels (k_local_cc: the 7-position dense instance
local_cc_tile7 and the two 8-position instances of local_cc_tile) on code sets that are
dense AND fall into many clusters (tests/h3_families.py), against the oracle's union-find
and the independent grid reference.

Uniform random codes at these densities percolate into one cluster, an answer that a kernel
uniting too much also gives. Here every word holds several in-word components, or scattered
codes next to component words, or two boxes whose edges overflow the edge list, and a parity
rule keeps the clusters apart: a wrong representative, a wrong closure lead, a component
mask read from the wrong word or an edge-batch window off by one merges or splits clusters
that both references keep as they are. Each case also asserts which instance the data
calls for (stats slots S_P0 / S_LCAP), so all three ran on non-degenerate answers.
"""
from __future__ import annotations

import os

import numpy as np
import pyarrow as pa
import pytest

import h3_families as F

pytestmark = pytest.mark.gpu

S_P0, S_LCAP = 6, 7  # slots of the workspace's stats block (cluster_kernels.hip, StatSlot)
FAMILY = dict(F.FAMILIES)


@pytest.fixture(scope="module")
def rg():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import rogtk_amd

    assert rogtk_amd.device_count() >= 1
    return rogtk_amd


def P():
    from oracle import pyoracle

    return pyoracle


_REF = {}


def _reference(key, codes, L):
    """Oracle ids of the sorted distinct codes (computed once per key, never modified), checked
    against the grid reference where that is cheap (L <= 10)."""
    if key not in _REF:
        rc, rv, rk, _ = P().umi_cluster(P().StrCol.from_fixed(F.codes_to_ascii(codes, L)), L, 1,
                                        threads=min(16, os.cpu_count() or 1))
        assert rv.all()
        if L <= 10:
            gi, gk = F.grid_components(codes, L)
            assert gk == rk and np.array_equal(gi, rc), "oracle != grid reference"
        rc.setflags(write=False)
        _REF[key] = (rc, rk)
    return _REF[key]


def _rows(codes, seed):
    """Every code 1-3 times, shuffled: the assign kernel sees duplicates in any order."""
    rng = np.random.default_rng(seed)
    return rng.permutation(np.repeat(codes, rng.integers(1, 4, codes.size)))


def _expected_instance(codes, L):
    densest = F.densest_tile(codes, 8)
    return (8 if L >= 8 and densest <= 16384 else 7), (1 if densest > 8192 else 0)


def _mark_local(eng, batch, L):
    if 7 <= L <= 13:
        return eng.mark_bitmap(batch)
    eng.mark(batch)
    return eng.build_local_bitmap()


def _run(eng, L, rows):
    """mark -> local bitmap -> resolve -> assign on one engine; ids, stats, (S_P0, S_LCAP)."""
    import torch

    from rogtk_amd import device as D

    batch = D.PackedBatch(torch.from_numpy(rows.view(np.int32)).cuda(), L)
    cid = torch.full((rows.size,), -7, dtype=torch.int32, device="cuda")
    local = _mark_local(eng, batch, L)
    eng.resolve(local, 1, 1)
    eng.assign(batch, cid)
    stats = eng.stats()
    torch.cuda.synchronize()
    st = eng.ws[:64].cpu().numpy().view(np.int64)
    return cid.cpu().numpy().view(np.uint32), stats, (int(st[S_P0]), int(st[S_LCAP]))


def _check(eng, key, codes, L, seed=0, want_clusters=None):
    rc, rk = _reference(key, codes, L)
    rows = _rows(codes, seed)
    cid, stats, inst = _run(eng, L, rows)
    want = _expected_instance(codes, L)
    print(f"{key}: codes {codes.size} rows {rows.size} clusters {rk} got {stats} instance {inst} want {want}")
    assert stats["error"] == 0 and stats["overflow"] == 0, (key, stats)
    assert inst == want, (key, inst, want)
    assert stats["n_distinct"] == codes.size, key
    assert stats["n_clusters"] == rk, (key, stats["n_clusters"], rk)
    if want_clusters is not None:
        assert rk == want_clusters, (key, rk)
    bad = np.flatnonzero(cid != rc[np.searchsorted(codes, rows)])
    assert bad.size == 0, (key, bad.size, rows[bad[:5]], cid[bad[:5]])


def _engine(L, n_rows):
    from rogtk_amd import device as D

    return D.ClusterEngine(L, min(n_rows, 4 ** L), "cuda")


# ------------------------------------------------------------------ one tile, one workgroup
@pytest.mark.parametrize("family", list(FAMILY))
@pytest.mark.parametrize("L", [3, 4, 5, 6, 7])
def test_one_tile_every_family(rg, L, family):
    """L <= 7: the whole space is one tile of local_cc_tile7, one workgroup, no global round
    (L = 3..6: lpos = L, 0 / 1 / 4 / 16 word groups per position). 8 seeds per family through
    one engine, so the workspace also carries the previous answer into the next."""
    eng = _engine(L, 3 * 4 ** L)
    for seed in range(8):
        codes = FAMILY[family](L, seed)
        assert codes.size > 0
        _check(eng, ("tile", family, L, seed), codes, L, seed)


# ------------------------------------------------- 7-position tiling + global rounds 7..L-1
@pytest.mark.parametrize("keep", [1.0, 0.85, 0.6])
@pytest.mark.parametrize("L", [8, 10])
def test_parity_cubes_seven_positions_then_global(rg, L, keep):
    """parity_cubes(L, 8, keep): every 4^8 tile holds 32768 * keep codes, so the 7-position
    instance takes the space (every word four 8-code components) and the global rounds join
    the class cubes across position 7 only (and nothing across 8, 9)."""
    codes = F.parity_cubes(L, 8, keep, seed=1)
    structural = keep >= 0.85  # (seed 1: no class cube is cut by the thinning, test_family_floors)
    _check(_engine(L, 3 * codes.size), ("parity_cubes", L, keep), codes, L,
           want_clusters=(128 if L == 8 else 512) if structural else None)


@pytest.mark.parametrize("how", ["parity", "mod4"])
@pytest.mark.parametrize("family", ["mixed", "boxes", "boxes2", "twobox"])
def test_ballasted_word_families_seven_positions(rg, family, how):
    """L = 9 word families (every kind of word next to every other; one- and two-box words;
    the two-box mask) with a 32768-code ballast tile, so the 7-position instance runs over
    all of them and the global rounds follow at positions 7 and 8."""
    L = 9
    base = {"mixed": lambda: F.mixed(L), "boxes": lambda: F.boxes(L, 0.1),
            "boxes2": lambda: F.boxes(L, 0.1, two=True), "twobox": lambda: F.twobox(L, 1.0)}[family]()
    codes = F.with_ballast(F.masked(base, L, how), L)
    assert _expected_instance(codes, L) == (7, 1)
    _check(_engine(L, 3 * codes.size), ("ballast", family, how), codes, L)


@pytest.mark.parametrize("how", ["parity", "mod4"])
@pytest.mark.parametrize("family", ["mixed", "boxes2"])
def test_word_families_eight_positions(rg, family, how):
    """The same families without the ballast: tiles of a few thousand codes, the 8192-code
    8-position instance (one-component words as single vertices next to per-code words)."""
    L = 9
    base = F.mixed(L) if family == "mixed" else F.boxes(L, 0.1, two=True)
    codes = F.masked(base, L, how)
    assert _expected_instance(codes, L)[0] == 8
    _check(_engine(L, 3 * codes.size), ("plain", family, how), codes, L)


@pytest.mark.parametrize("ballast", [False, True])
@pytest.mark.parametrize("seed", range(6))
def test_chains_every_position(rg, seed, ballast):
    """chains(9, seed): groups of 4 one-component words linked in a path of random order along
    word position seed % 6 (code positions 3..8), every group one cluster of 6 codes: the
    4-word closure of the 7-position instance (ballast), the listed edges of the 8-position
    one, and the global rounds' own closure at positions 7 and 8 must find each path whole."""
    L = 9
    codes = F.chains(L, seed)
    if ballast:
        codes = F.with_ballast(codes, L)
    else:
        assert _reference(("chains9", seed, "plain"), codes, L)[1] == 4 ** 5 // 4
    _check(_engine(L, 3 * codes.size), ("chains9", seed, "ballast" if ballast else "plain"), codes, L, seed)


# ------------------------------------- 8-position instances: edge batches, capacity met exactly
@pytest.mark.parametrize("L", [8, 9, 10])
@pytest.mark.parametrize("how", ["mod4", "parity"])
def test_twobox_eight_positions_edge_batches(rg, how, L):
    """masked(twobox(L, 1), how): every present word is the two-box mask (32 codes, two
    components, 80 in-word edges, listed per code). mod4: 8192 codes per 4^8 tile = the small
    instance's capacity exactly, ~20k edges against an edge list of 8192 (three batches), every
    word two clusters of 16 on its own. parity: 16384 codes per tile = the big instance's
    capacity exactly, edges far past its list of 12288. L = 9, 10: the global rounds follow."""
    codes = F.masked(F.twobox(L, 1.0), L, how)
    assert F.densest_tile(codes, 8) == (8192 if how == "mod4" else 16384)
    assert _expected_instance(codes, L) == (8, 0 if how == "mod4" else 1)
    _check(_engine(L, 3 * codes.size), ("twobox", how, L), codes, L,
           want_clusters=2 * 4 ** (L - 3) // 4 if how == "mod4" else None)


@pytest.mark.parametrize("L", [8, 9])
@pytest.mark.parametrize("n_twobox,n_domino,ecap,lcap", [(102, 154, 8192, 0), (153, 40, 12288, 1)])
def test_edge_list_boundary_on_bridges(rg, n_twobox, n_domino, ecap, lcap, L):
    """bridge_overflow: per tile, two-box words whose 80 * n_twobox in-word edges (none a bridge)
    fill the edge list (ecap: the list sizes of the two 8-position instances, k_local_cc) up to
    just short of its end, then domino words whose edges are all bridges, across the end of the
    list and into the second batch. An edge lost, doubled into the wrong slot or left unread at
    the batch boundary splits a domino (the two-box words alone would hide it: their components
    stay connected without any one edge)."""
    assert 80 * n_twobox < ecap - 1 and 80 * n_twobox + 2 * n_domino > ecap + 1
    codes = F.bridge_overflow(L, n_twobox, n_domino)
    assert _expected_instance(codes, L) == (8, lcap)
    per_tile = 2 * n_twobox + 2 * n_domino + (256 - n_twobox - n_domino)
    _check(_engine(L, 3 * codes.size), ("bridges", L, n_twobox, n_domino), codes, L,
           want_clusters=per_tile * 4 ** (L - 8))


@pytest.mark.parametrize("extra", [0.0, 0.03])
@pytest.mark.parametrize("L", [8, 10])
def test_mod4_singletons_stay_singletons(rg, L, extra):
    """mod4(L, extra): per-code words only (16 scattered codes each). extra = 0: 16384 codes per
    tile (the big 8-position instance at capacity), no edge anywhere: 4^L / 4 singletons must stay
    singletons. extra = 0.03: ~17.9k codes per tile, the 7-position instance with per-code words
    only, the extra codes bridging some of the singletons."""
    codes = F.mod4(L, extra, seed=1)
    _check(_engine(L, 3 * codes.size), ("mod4", L, extra), codes, L,
           want_clusters=4 ** L // 4 if extra == 0.0 else None)


# ------------------------------------------------------------- the 8-rank operating point
def _operating_point():
    L = 12
    codes = F.parity_cubes(L, 8, 0.85, seed=1)
    return L, codes


def test_operating_point_single_engine(rg):
    """parity_cubes(12, 8, .85): 1.78M codes, every 4^7 tile 43% dense (the density of the
    8-rank union bitmap) and 8192 clusters instead of one."""
    L, codes = _operating_point()
    _check(_engine(L, 3 * codes.size), ("parity_cubes", 12, 0.85), codes, L, want_clusters=8192)


def test_operating_point_eight_ranks(rg):
    """The same rows split over 8 emulated ranks: per-rank mark and local bitmap, the
    concatenation as the all-gather, resolve over the 8 bitmaps and assign on every rank."""
    import torch

    from rogtk_amd import device as D

    L, codes = _operating_point()
    rc, rk = _reference(("parity_cubes", 12, 0.85), codes, L)
    assert rk == 8192
    rows = _rows(codes, 8)
    n, shards = rows.size, 8
    dev_rows = torch.from_numpy(rows.view(np.int32)).cuda()
    cid = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    bounds = (np.linspace(0, n, shards + 1).astype(np.int64) // 4) * 4  # 16-byte aligned slices
    bounds[-1] = n
    engs, bats = [], []
    for r in range(shards):
        a, b = int(bounds[r]), int(bounds[r + 1])
        e = D.ClusterEngine(L, min(n, 4 ** L), "cuda")
        bt = D.PackedBatch(dev_rows[a:b], L)
        e.mark(bt)
        engs.append(e)
        bats.append((a, b, bt))
    gathered = torch.cat([e.build_local_bitmap().clone() for e in engs])
    for e, (a, b, bt) in zip(engs, bats):
        e.resolve(gathered, shards, 1)
        e.assign(bt, cid[a:b])
    torch.cuda.synchronize()
    for e in engs:
        stats = e.stats()
        st = e.ws[:64].cpu().numpy().view(np.int64)
        assert stats["error"] == 0 and stats["overflow"] == 0
        assert stats["n_distinct"] == codes.size and stats["n_clusters"] == rk
        assert (int(st[S_P0]), int(st[S_LCAP])) == (7, 1)
    got = cid.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, rc[np.searchsorted(codes, rows)])


# ------------------------------------------------------------------------- the host ABI
@pytest.mark.parametrize("name", ["parity_cubes7", "mod4_8", "mixed9_mod4"])
def test_host_abi_dense_families(rg, name):
    """rg.umi_cluster on strings of the dense families, with a null row and a row holding an N
    (one Hamming-1 step from a present code) appended; valid rows against the oracle."""
    L, codes = {"parity_cubes7": lambda: (7, F.parity_cubes(7, 8, 0.85, seed=1)),
                "mod4_8": lambda: (8, F.mod4(8, 0.03, seed=1)),
                "mixed9_mod4": lambda: (9, F.masked(F.mixed(9), 9, "mod4"))}[name]()
    rows = _rows(codes, 3)
    umis = [bytes(r) for r in F.codes_to_ascii(rows, L)]
    with_n = bytearray(umis[0])
    with_n[L // 2] = ord("N")
    umis += [None, bytes(with_n)]
    rc, rv, rk, _ = P().umi_cluster(P().StrCol.from_list(umis), L, 1)
    got, k, rl = rg.umi_cluster(pa.array(umis, type=pa.large_binary()), L, 1)
    assert rl == L and k == rk
    assert got.null_count == 1 and not got[len(umis) - 2].is_valid
    g = np.asarray(got.fill_null(0).to_numpy(zero_copy_only=False)).astype(np.uint32)
    assert np.array_equal(g[rv], rc[rv])
    # the regular rows alone are the family's clusters (the N row joins, never splits, them)
    assert rk >= 16
