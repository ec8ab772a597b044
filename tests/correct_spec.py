"""The UMI-correction spec restated in pure Python, shared by
tests/test_correct.py and tests/test_gpu_correct.py (not a test module itself).

Clusters come from the oracle (oracle.pyoracle); per cluster a Counter of its rows' byte
strings and min(key=(-count, not regular, bytes)) name the representative.
"""
from collections import Counter

# the known answer of the spec: umi_len 4, max_distance 1
KNOWN_ROWS = ([b"AAAA"] * 3 + [b"AAAT"] * 3 + [b"AATT"] + [b"CCCC"] * 2 + [b"CCCG"] * 3 + [None]
              + [b"GGGN"] * 2 + [b"GGGT"] * 2 + [b"TTTT"] * 2 + [b"TTTN"] * 3 + [b"NNNN"]
              + [b"AAAAA"] * 2 + [b"AAAAC"] * 2 + [b"ACGa", b"ACGT"])
KNOWN_TABLE = [(b"AAAA", 7, 3), (b"ACGT", 2, 2), (b"CCCG", 5, 2), (b"GGGT", 4, 2), (b"TTTN", 5, 2),
               (b"AAAAA", 4, 2), (b"NNNN", 1, 1)]


def is_regular(s: bytes, L: int) -> bool:
    return 1 <= L <= 32 and len(s) == L and all(c in b"ACGT" for c in s)


def resolve_len(items, umi_len: int) -> int:
    if umi_len > 0:
        return umi_len
    return next((len(x) for x in items if x is not None), 0)


def summarize(items, ids, n_clusters: int, L: int):
    """(table, corrected): table[c] = (representative, n_reads, n_distinct); an id without
    rows gives (b"", 0, 0)."""
    per = [Counter() for _ in range(n_clusters)]
    for x, c in zip(items, ids):
        if x is not None:
            per[c][bytes(x)] += 1
    table = []
    for cnt in per:
        if not cnt:
            table.append((b"", 0, 0))
            continue
        rep = min(cnt, key=lambda s: (-cnt[s], not is_regular(s, L), s))
        table.append((rep, sum(cnt.values()), len(cnt)))
    corrected = [None if x is None else table[c][0] for x, c in zip(items, ids)]
    return table, corrected


def restate(items, umi_len: int, max_distance: int, brute: bool = True):
    """(ids with None for nulls, n_clusters, table, corrected) of the spec."""
    from oracle import pyoracle as P

    L = resolve_len(items, umi_len)
    if brute:
        ids, k = P.py_cluster_bruteforce(items, L, max_distance)
    else:
        cid, valid, k, _ = P.umi_cluster(P.StrCol.from_list(items), L, max_distance)
        ids = [int(c) if v else None for c, v in zip(cid, valid)]
    table, corrected = summarize(items, ids, k, L)
    return ids, k, table, corrected


def table_of(clusters):
    """A rogtk_amd `clusters` StructArray as the restatement's list of tuples."""
    reps = clusters.field("representative").to_pylist()
    reps = [r.encode() if isinstance(r, str) else bytes(r) for r in reps]
    return list(zip(reps, clusters.field("n_reads").to_pylist(), clusters.field("n_distinct").to_pylist()))


def as_bytes(arr):
    return [None if x is None else (x.encode() if isinstance(x, str) else bytes(x)) for x in arr.to_pylist()]
