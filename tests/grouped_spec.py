"""The spec of UMI clustering within groups restated in pure Python on top of
directional_spec.py and correct_spec.py, shared by tests/test_grouped_spec.py and
tests/test_gpu_grouped.py (not a test module).

Every row carries an unsigned 32-bit key. The rows are split by key; each key's rows alone go
through the ungrouped rule (max_distance 1: the directional rule of §4c, max_distance 0: exact
strings); a cluster is regular when its representative is a regular string. Global ids: the
regular clusters in ascending (key, root code), then the irregular ones in ascending
(key, bytes); None for a null row whatever its key.
"""
from correct_spec import is_regular, resolve_len, summarize
from directional_spec import KNOWN_ROWS, ids_of, regular_counts, roots_fixed_point

# The known answer: directional_spec.KNOWN_ROWS, umi_len 4, max_distance 1, with these keys
# (chain 7, blocked pair 3, plateau 0xFFFFFFFF, contested 1, "through" 0, the null row 5, the
# two ACGN rows 1 and 7, ACGTA 0). The two edges that cross the named groups in the ungrouped
# column (AAAA -> GAAA, TCGG -> TTGG) are gone.
KNOWN_KEYS = [7] * 18 + [3] * 12 + [0xFFFFFFFF] * 3 + [1] * 17 + [0] * 215 + [5] + [1, 7] + [0]
assert len(KNOWN_KEYS) == len(KNOWN_ROWS)
# (representative, n_reads, n_distinct, group) in id order
KNOWN_TABLE = [(b"ACAC", 155, 3, 0), (b"TCGG", 60, 1, 0), (b"TTGG", 9, 2, 1), (b"TTTT", 8, 1, 1),
               (b"CCCC", 6, 1, 3), (b"CCCG", 6, 1, 3), (b"AAAA", 18, 4, 7), (b"GAAA", 3, 3, 0xFFFFFFFF),
               (b"ACGTA", 1, 1, 0), (b"ACGN", 1, 1, 1), (b"ACGN", 1, 1, 7)]


def identity_roots(counts) -> dict:
    """max_distance 0: no edges, every distinct string is its own root."""
    return {v: v for v in counts}


def restate(items, keys, umi_len: int, max_distance: int = 1, roots_fn=roots_fixed_point):
    """(ids with None for nulls, n_clusters, table, corrected); table[c] = (representative,
    n_reads, n_distinct, group)."""
    assert len(items) == len(keys) and all(0 <= int(k) <= 0xFFFFFFFF for k in keys)
    assert max_distance in (0, 1)
    L = resolve_len(items, umi_len)  # of the whole column, as the ungrouped call
    rows_of = {}
    for i, k in enumerate(keys):
        rows_of.setdefault(int(k), []).append(i)
    regular, irregular = [], []  # (key, local id) in the global order of each class
    local = {}
    for k in sorted(rows_of):
        sub = [items[i] for i in rows_of[k]]
        counts = regular_counts(sub, L)
        ids, n = ids_of(sub, L, (roots_fn if max_distance == 1 else identity_roots)(counts))
        table, _ = summarize(sub, ids, n, L)
        for c in range(n):  # ascending root code, then ascending bytes: ids_of's own order
            (regular if is_regular(table[c][0], L) else irregular).append((k, c))
        for i, c in zip(rows_of[k], ids):
            local[i] = c
    label = {kc: j for j, kc in enumerate(regular + irregular)}
    ids = [None if local[i] is None else label[(int(keys[i]), local[i])] for i in range(len(items))]
    table, corrected = summarize(items, ids, len(label), L)
    group = [k for k, _ in regular + irregular]
    return ids, len(label), [t + (g,) for t, g in zip(table, group)], corrected
