"""CPU: the H3 oracle (a union-find over an edge search) against an independent reference,
label propagation over the 4^L grid (h3_families.grid_components), on dense code sets that
fall into many clusters; and the floors that keep those code sets non-degenerate (the GPU
tests of the local-CC kernels, test_gpu_dense_cc.py, rest on them)."""
from __future__ import annotations

import os

import numpy as np
import pytest

import h3_families as F
from oracle import pyoracle as P


def _oracle(codes, L):
    rc, rv, rk, rl = P.umi_cluster(P.StrCol.from_fixed(F.codes_to_ascii(codes, L)), L, 1,
                                   threads=min(8, os.cpu_count() or 1) if codes.size > 100_000 else 1)
    assert rv.all() and rl == L
    return rc, rk


@pytest.mark.parametrize("L", range(3, 11))
@pytest.mark.parametrize("family", [name for name, _ in F.FAMILIES])
def test_oracle_equals_grid_reference(family, L):
    """Every family, L = 3..10, three seeds: the oracle's ids and cluster count equal the
    grid reference's, and (L <= 5) the O(n^2) brute force's."""
    make = dict(F.FAMILIES)[family]
    for seed in range(3):
        codes = make(L, seed)
        assert codes.size > 0 and codes.dtype == np.uint32
        assert np.array_equal(codes, np.unique(codes)), "sorted distinct codes"
        rc, rk = _oracle(codes, L)
        gi, gk = F.grid_components(codes, L)
        assert gk == rk, (seed, gk, rk)
        assert np.array_equal(gi, rc), seed
        if L <= 5:
            bf, bk = P.py_cluster_bruteforce([bytes(r) for r in F.codes_to_ascii(codes, L)], L, 1)
            assert bk == rk and np.array_equal(np.asarray(bf, dtype=np.uint32), rc), seed


def test_grid_reference_handles_rows_not_codes():
    """Duplicated, shuffled rows get the ids of their codes."""
    codes = F.masked(F.mixed(7, seed=5), 7, "parity")
    rng = np.random.default_rng(0)
    rows = rng.permutation(np.repeat(codes, rng.integers(1, 4, codes.size)))
    gi, gk = F.grid_components(rows, 7)
    ci, ck = F.grid_components(codes, 7)
    assert gk == ck and np.array_equal(gi, ci[np.searchsorted(codes, rows)])


# name -> (L, codes builder, exact codes, exact densest 4^7 tile, exact densest 4^8 tile,
# exact clusters, floor rule); None = not pinned exactly. The exact values are structural
# (see the generators); the cluster counts of the thinned parity cubes are exact for these
# seeds because no class cube of theirs is cut in two by the thinning (at keep 0.85 a code
# loses all 8 in-cube neighbours with probability 2.6e-7; other seeds do split one).
FLOORS = {
    "parity_cubes(7,8,1.0)": (7, lambda: F.parity_cubes(7, 8, 1.0), 8192, 8192, None, 64, "half"),
    "parity_cubes(7,8,.85)": (7, lambda: F.parity_cubes(7, 8, 0.85, seed=1), None, None, None, 64, "half"),
    "parity_cubes(8,8,.85)": (8, lambda: F.parity_cubes(8, 8, 0.85, seed=1), None, None, None, 128, "half"),
    "parity_cubes(10,8,.85)": (10, lambda: F.parity_cubes(10, 8, 0.85, seed=1), None, None, None, 512, "half"),
    "parity_cubes(12,8,.85)": (12, lambda: F.parity_cubes(12, 8, 0.85, seed=1), None, None, None, 8192, "half"),
    "mod4(8,0)": (8, lambda: F.mod4(8, 0.0), 16384, None, 16384, 16384, "half"),
    "mod4(8,.03)": (8, lambda: F.mod4(8, 0.03, seed=1), None, None, None, None, "quarter"),
    "mod4(10,.03)": (10, lambda: F.mod4(10, 0.03, seed=1), None, None, None, None, "quarter"),
    "masked(twobox(8,1),mod4)": (8, lambda: F.masked(F.twobox(8, 1.0), 8, "mod4"), 8192, 2048, 8192, 512, "exact"),
    "masked(twobox(8,1),parity)": (8, lambda: F.masked(F.twobox(8, 1.0), 8, "parity"), 16384, 4096, 16384, 32,
                                   "half"),
    "masked(mixed(9),mod4)": (9, lambda: F.masked(F.mixed(9), 9, "mod4"), None, None, None, None, "half"),
    "masked(boxes(9,.1),parity)": (9, lambda: F.masked(F.boxes(9, 0.1), 9, "parity"), None, None, None, None,
                                   "half"),
}


@pytest.mark.parametrize("name", list(FLOORS))
def test_family_floors(name):
    """The inputs of the dense GPU cases are dense and many-cluster by the references alone:
    exact counts where the construction fixes them; otherwise at least 16 clusters and no
    cluster with more than half the codes (mod4 with extras: a giant component of ~60% of
    the codes forms, the bound there is n_clusters >= n_codes / 4). Oracle == grid reference
    on each of them too (L = 12 included)."""
    L, make, n_exact, d7_exact, d8_exact, k_exact, rule = FLOORS[name]
    codes = make()
    rc, rk = _oracle(codes, L)
    gi, gk = F.grid_components(codes, L)
    assert gk == rk and np.array_equal(gi, rc)
    sizes = F.cluster_sizes(rc)
    print(f"{name}: codes {codes.size} densest 4^7 {F.densest_tile(codes, 7)} 4^8 {F.densest_tile(codes, 8)} "
          f"clusters {rk} largest {sizes.max()}")
    if n_exact is not None:
        assert codes.size == n_exact
    if d7_exact is not None:
        assert F.densest_tile(codes, 7) == d7_exact
    if d8_exact is not None:
        assert F.densest_tile(codes, 8) == d8_exact
    if k_exact is not None:
        assert rk == k_exact
    if rule == "half":
        assert rk >= 16 and sizes.max() <= codes.size // 2
    elif rule == "quarter":
        assert rk >= 16 and rk >= codes.size / 4


def test_word_kinds_present():
    """The families put every kind of word in front of the 7-position kernel: 1, 2, 3, 4 in-word
    components, more than 4 (one vertex per code), and the pure families their single kind."""
    def kinds(codes):
        out = set()
        for w in np.unique(codes >> 6):
            bits = (codes[(codes >> 6) == w] & 63).astype(np.uint32)
            _, k = F.grid_components(bits, 3)
            out.add(min(k, 5))
        return out

    assert kinds(F.parity_cubes(7, 8, 1.0)) == {4}
    assert kinds(F.mod4(7, 0.0)) == {5}
    assert kinds(F.masked(F.twobox(7, 1.0), 7, "mod4")) == {2}
    assert kinds(F.masked(F.boxes(7, 0.1), 7, "parity")) == {1}
    assert kinds(F.masked(F.boxes(7, 0.1, two=True), 7, "parity")) == {1, 2}
    assert kinds(F.masked(F.mixed(7), 7, "parity")) >= {1, 2, 3, 4, 5}


def test_ballast_forces_seven_positions():
    codes = F.with_ballast(F.masked(F.mixed(9), 9, "mod4"), 9)
    assert np.array_equal(codes, np.unique(codes))
    assert F.densest_tile(codes, 8) == 32768
    rc, rk = _oracle(codes, 9)
    gi, gk = F.grid_components(codes, 9)
    assert gk == rk and np.array_equal(gi, rc)
    # the ballast's class cubes link to the codes below them through the top digit, and
    # still leave many clusters
    assert rk >= 16 and F.cluster_sizes(rc).max() <= codes.size // 2


@pytest.mark.parametrize("n_twobox,n_domino", [(102, 154), (153, 40)])
def test_bridge_overflow_counts(n_twobox, n_domino):
    """Every word of bridge_overflow is on its own: 2 clusters per two-box or domino word, 1 per
    full word, by both references."""
    codes = F.bridge_overflow(8, n_twobox, n_domino)
    assert codes.size == 32 * n_twobox + 4 * n_domino + 64 * (256 - n_twobox - n_domino)
    rc, rk = _oracle(codes, 8)
    gi, gk = F.grid_components(codes, 8)
    assert gk == rk and np.array_equal(gi, rc)
    assert rk == 2 * n_twobox + 2 * n_domino + (256 - n_twobox - n_domino)
