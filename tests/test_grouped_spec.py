"""The restatement of clustering within groups (tests/grouped_spec.py) against
its known answer and against the ungrouped restatement. No GPU."""
import numpy as np
import pytest

import directional_spec as D
import grouped_spec as G


@pytest.mark.parametrize("roots_fn", [D.roots_bfs, D.roots_fixed_point])
def test_known_table(roots_fn):
    ids, k, table, corrected = G.restate(D.KNOWN_ROWS, G.KNOWN_KEYS, 4, 1, roots_fn)
    assert k == 11 and table == G.KNOWN_TABLE
    assert sum(t[1] for t in table) == 268 == sum(x is not None for x in D.KNOWN_ROWS)
    assert [i for i, x in zip(ids, D.KNOWN_ROWS) if x is None] == [None]
    # the two edges that cross the named groups in the ungrouped column are gone
    at = {(x, key): i for x, key, i in zip(D.KNOWN_ROWS, G.KNOWN_KEYS, ids)}
    assert at[(b"GAAA", 0xFFFFFFFF)] == 7 != at[(b"AAAA", 7)]
    assert at[(b"TTGG", 1)] == 2 != at[(b"TCGG", 0)]
    assert at[(b"ACGN", 1)] == 9 and at[(b"ACGN", 7)] == 10
    for x, c in zip(D.KNOWN_ROWS, corrected):
        assert (x is None) == (c is None)


@pytest.mark.parametrize("roots_fn", [D.roots_bfs, D.roots_fixed_point])
@pytest.mark.parametrize("key", [0, 9, 0xFFFFFFFF])
def test_one_key_is_the_ungrouped_answer(roots_fn, key):
    ids, k, table, corrected = G.restate(D.KNOWN_ROWS, [key] * len(D.KNOWN_ROWS), 4, 1, roots_fn)
    want = D.restate(D.KNOWN_ROWS, 4, roots_fn)
    assert (ids, k, corrected) == (want[0], want[1], want[3])
    assert [t[:3] for t in table] == D.KNOWN_TABLE == want[2] and {t[3] for t in table} == {key}


def test_order_preserving_relabelling_changes_nothing():
    base = G.restate(D.KNOWN_ROWS, G.KNOWN_KEYS, 4)
    for f in (lambda k: min(2 * k, 0xFFFFFFFF), lambda k: sorted(set(G.KNOWN_KEYS)).index(k),
              lambda k: k // 2 + 5 * (k > 0)):
        keys = [f(k) for k in G.KNOWN_KEYS]
        ids, k, table, corrected = G.restate(D.KNOWN_ROWS, keys, 4)
        assert (ids, k, corrected) == (base[0], base[1], base[3])
        assert [t[:3] for t in table] == [t[:3] for t in base[2]]
        assert [t[3] for t in table] == [f(t[3]) for t in base[2]]
    # a map that reverses the order of the keys reorders the ids, not the clusters
    ids, k, table, _ = G.restate(D.KNOWN_ROWS, [0xFFFFFFFF - k for k in G.KNOWN_KEYS], 4)
    assert k == base[1] and sorted(t[:3] for t in table) == sorted(t[:3] for t in base[2]) and ids != base[0]


def test_max_distance_0_is_the_distinct_pairs():
    rows = D.random_families(seed=3, L=6, parents=40, mean=6.0)
    rows[5], rows[17] = None, rows[16][:-1] + b"N"
    keys = list(np.random.default_rng(1).integers(0, 4, len(rows)))
    ids, k, table, corrected = G.restate(rows, keys, 6, 0)
    pairs = {(int(g), x) for g, x in zip(keys, rows) if x is not None}
    assert k == len(pairs) and {(t[3], t[0]) for t in table} == pairs
    assert corrected == rows and all(t[2] == 1 for t in table)
    regular = [(t[3], t[0]) for t in table if len(t[0]) == 6 and b"N" not in t[0]]
    assert regular == sorted(regular, key=lambda p: (p[0], D.code(p[1]))) and table[-1][0].endswith(b"N")


def test_every_row_in_its_own_key():
    rows = D.KNOWN_ROWS
    ids, k, table, corrected = G.restate(rows, list(range(len(rows))), 4)
    assert k == sum(x is not None for x in rows) and corrected == rows
    assert sorted(i for i in ids if i is not None) == list(range(k))
