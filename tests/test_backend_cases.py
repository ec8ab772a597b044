"""The preconditions of the cases in tests/backend_cases.py, checked on the CPU: each case enters
the branch of the device code it is aimed at. These are conditions on the inputs, worked out from
the order in which the kernels visit them; nothing here runs the library.

Vote table (correct.hip): a workgroup votes for the run heads of 4096 consecutive sorted rows
into 1024 LDS slots. A tile that votes for more than 1024 distinct cluster ids cannot hold them
all, so at least (ids - 1024) of its votes take the fallback to the global tables."""
from __future__ import annotations

import numpy as np
import pytest

import backend_cases as B


def _packed_tiles(name, all_regular):
    case = B.vote_case(name)
    votes = B.packed_votes(case, all_regular)
    rows = case.n if all_regular else int(case.reg.sum())
    return case, votes, B.tiles_of_votes(votes), rows


@pytest.mark.parametrize("all_regular", [True, False])
@pytest.mark.parametrize("name", ["own_id", "interleaved"])
def test_packed_tiles_hold_more_ids_than_slots(name, all_regular):
    case, votes, tiles, rows = _packed_tiles(name, all_regular)
    profile = B.tile_profile(tiles, rows)
    print(name, "all regular" if all_regular else "bits off", "(rows, ids) per tile:", profile)
    # a tile of at most 1024 rows (the tail of the column) cannot overflow; every other one must
    assert any(r > B.VOTE_SLOTS for r, _ in profile)
    assert all(ids > B.VOTE_SLOTS for r, ids in profile if r > B.VOTE_SLOTS)
    assert sum(1 for r, _ in profile if r == B.VOTE_TILE) >= (1 if all_regular else 0)
    # the count-table method votes per present code, a tile being 4096 codes of the code space
    space = B.tiles_of_votes(votes, position=lambda v: v[1])
    table = B.tile_profile(space, 4 ** case.L)
    print(name, "count table (codes, ids) per tile:", table)
    assert all(ids > B.VOTE_SLOTS for _, ids in table)
    # the caller's ids are dense and the column's rows use them as the case says
    assert case.ids.max() < case.k and 4 ** case.L > case.codes.max()


def test_own_id_shape():
    case = B.vote_case("own_id")
    assert (case.n, case.k, case.L) == (4097, 4096, 6)
    assert sorted(case.codes.tolist()) == [0] + list(range(4096))
    assert np.array_equal(case.ids, case.codes)
    assert 0.04 < 1 - case.reg.mean() < 0.08


@pytest.mark.parametrize("all_regular", [True, False])
def test_interleaved_clusters_span_tiles_and_tie_across_them(all_regular):
    case, votes, tiles, rows = _packed_tiles("interleaved", all_regular)
    assert 2.5 * B.VOTE_TILE < rows <= 3 * B.VOTE_TILE and len(tiles) == 3
    wide = B.clusters_over_tiles(tiles, 3)
    ties = B.cross_tile_ties(tiles)
    print("interleaved", "all regular" if all_regular else "bits off", "rows", rows, "clusters voted for from 3 tiles:",
          len(wide), "top-count ties across tiles:", len(ties))
    assert len(wide) >= 20
    assert len(ties) >= 10
    # the tie is decided by the code: the winner is not the vote of the last tile
    by_id = {}
    for v in votes:
        by_id.setdefault(v[2], []).append(v)
    for c in ties:
        top = max(v[3] for v in by_id[c])
        assert len({v[1] for v in by_id[c] if v[3] == top}) >= 2
    if all_regular:
        assert len(ties) == 40 and len(wide) == 40


def test_same_home_ids_share_one_probe_window():
    case = B.vote_case("same_home")
    ids = B.same_home_ids()
    assert len(ids) == 12 and len({B.vote_home(i) for i in ids}) == 1
    assert case.n <= 64 and sorted(set(case.ids.tolist())) == ids and case.k > max(ids)
    # 12 ids, 8 probes from one home slot: at least 4 ids find no slot, and each has 3 votes
    votes = B.packed_votes(case, True)
    assert len(votes) == 36 and len(ids) - B.VOTE_PROBES >= 4
    assert len(B.tiles_of_votes(votes)) == 1
    assert len(B.tiles_of_votes(votes, position=lambda v: v[1])) == 1  # the count-table method's tile


@pytest.mark.parametrize("name", ["own_id", "interleaved"])
def test_general_tiles_hold_more_ids_than_slots(name):
    rows, ids, k, L = B.vote_strings(name)
    votes, live = B.general_votes(rows, ids)
    profile = B.tile_profile(B.tiles_of_votes(votes), live)
    irregular = {x for x in rows if x is not None and not (len(x) == L and all(c in b"ACGT" for c in x))}
    print(name, "general path (rows, ids) per tile:", profile, "irregular strings:", len(irregular), "nulls:",
          sum(x is None for x in rows))
    assert any(r == B.VOTE_TILE for r, _ in profile)
    assert all(i > B.VOTE_SLOTS for r, i in profile if r > B.VOTE_SLOTS)
    assert any(b"N" in x for x in irregular) and any(len(x) == L - 1 for x in irregular) and None in rows
    assert max(i for x, i in zip(rows, ids) if x is not None) < k


def test_hostile_column_holds_what_it_claims():
    distinct, rows = B.hostile_distinct(), B.hostile_rows()
    assert len(set(distinct)) == len(distinct) and 900 < len(distinct) < 1200
    assert 5000 < len(rows) < 7000 and sum(x is None for x in rows) == 100
    assert set(x for x in rows if x is not None) == set(distinct)
    lens = {len(x) for x in distinct}
    assert {0, 7, 8, 9, 15, 16, 17, 23, 24, 25, 63, 64, 65, 130, 257} <= lens
    assert any(b"\0" in x for x in distinct) and any(b >= 0x80 and b not in (0xC3, 0xA9) for x in distinct for b in x)
    assert all(b"A" + b"\0" * z in distinct for z in range(12))
    # equal strings are not neighbours in the input
    live = [x for x in rows if x is not None]
    assert sum(a == b for a, b in zip(live, live[1:])) < len(live) // 100
    regular = [x for x in distinct if len(x) == 8 and all(c in b"ACGT" for c in x)]
    assert len(regular) > 100
    print("hostile column:", len(rows), "rows,", len(distinct), "distinct strings,", len(regular), "regular")


def test_cc_graphs_have_the_sizes_they_claim():
    nv, E = B.cc_path()
    assert nv == 100_000 and len(E) == nv - 1 and not np.array_equal(E[:, 0], np.sort(E[:, 0]))
    nv, E = B.cc_star()
    assert (E == nv - 1).any(axis=1).all() and len(E) == nv - 1
    nv, E, labels, k = B.cc_small_components()
    assert nv == 70_001 and nv % 64 and len(E) % 64 and len(E) % 256 and 0 <= E.min() and E.max() < nv
    sizes = np.bincount(labels)
    assert len(sizes) == k and sizes.min() == 1 and sizes.max() == 5
    assert (E[:, 0] == E[:, 1]).sum() == 1501
