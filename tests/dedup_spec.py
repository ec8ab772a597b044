"""Two independent restatements of the UMI deduplication spec and a random-case
generator. Neither touches the library.

  (a) best_dict     a Python loop over the rows with one dict entry per cluster id
  (b) best_lexsort  numpy: a lexsort on (id, -score, row), the head of each run of equal ids

Both return a Dedup of plain numpy arrays:
  best_row int64 [k] (-1: no row), best_score u32 [k] (0 where -1), n_reads u32 [k],
  keep bool [n], keep_words u64 [(n + 63) // 64] (LSB first, padding zero), rows int64 ascending,
  n_kept.
A row whose id is >= k (0xFFFFFFFF among them) is skipped."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

NO_ID = 0xFFFFFFFF


@dataclass
class Dedup:
    best_row: np.ndarray
    best_score: np.ndarray
    n_reads: np.ndarray
    keep: np.ndarray
    keep_words: np.ndarray
    rows: np.ndarray
    n_kept: int


def pack_words(keep: np.ndarray) -> np.ndarray:
    """bool [n] -> u64 [(n + 63) // 64], bit i % 64 of word i // 64, padding zero."""
    n = keep.size
    bits = np.zeros((n + 63) // 64 * 64, dtype=np.uint8)
    bits[:n] = keep
    return np.packbits(bits, bitorder="little").view("<u8").astype(np.uint64)


def unpack_words(words: np.ndarray, n: int) -> np.ndarray:
    """Every bit of the words (padding included) as bool [64 * len(words)]."""
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u8").view(np.uint8), bitorder="little").astype(bool)


def _finish(best_row, best_score, n_reads, n) -> Dedup:
    keep = np.zeros(n, dtype=bool)
    keep[best_row[best_row >= 0]] = True
    rows = np.flatnonzero(keep).astype(np.int64)
    return Dedup(best_row, best_score, n_reads, keep, pack_words(keep), rows, int(rows.size))


def best_dict(ids, score, k: int) -> Dedup:
    ids = [int(x) for x in ids]
    n = len(ids)
    sc = [0] * n if score is None else [int(x) for x in score]
    best = {}
    reads = {}
    for i in range(n):
        c = ids[i]
        if c >= k:
            continue
        reads[c] = reads.get(c, 0) + 1
        if c not in best or sc[i] > sc[best[c]]:  # rows ascend, so a tie keeps the earlier row
            best[c] = i
    best_row = np.full(k, -1, dtype=np.int64)
    best_score = np.zeros(k, dtype=np.uint32)
    n_reads = np.zeros(k, dtype=np.uint32)
    for c, i in best.items():
        best_row[c] = i
        best_score[c] = sc[i]
        n_reads[c] = reads[c]
    return _finish(best_row, best_score, n_reads, n)


def best_lexsort(ids, score, k: int) -> Dedup:
    ids = np.asarray(ids, dtype=np.int64)
    n = ids.size
    sc = np.zeros(n, dtype=np.int64) if score is None else np.asarray(score, dtype=np.int64)
    rows = np.arange(n, dtype=np.int64)
    live = ids < k
    i, s, r = ids[live], sc[live], rows[live]
    order = np.lexsort((r, -s, i))
    i, s, r = i[order], s[order], r[order]
    head = np.ones(i.size, dtype=bool)
    head[1:] = i[1:] != i[:-1]
    best_row = np.full(k, -1, dtype=np.int64)
    best_score = np.zeros(k, dtype=np.uint32)
    best_row[i[head]] = r[head]
    best_score[i[head]] = s[head].astype(np.uint32)
    n_reads = np.bincount(i, minlength=k).astype(np.uint32) if k else np.zeros(0, np.uint32)
    return _finish(best_row, best_score, n_reads, n)


def same(a: Dedup, b: Dedup) -> bool:
    return (np.array_equal(a.best_row, b.best_row) and np.array_equal(a.best_score, b.best_score)
            and np.array_equal(a.n_reads, b.n_reads) and np.array_equal(a.keep, b.keep)
            and np.array_equal(a.keep_words, b.keep_words) and np.array_equal(a.rows, b.rows)
            and a.n_kept == b.n_kept)


def random_case(seed: int):
    """(ids u32, score u32 or None, k): small cases with score ties, ids without rows, skipped
    ids (>= k and 0xFFFFFFFF), and now and then no rows, no clusters or no scores."""
    rng = np.random.default_rng(seed)
    n = int(rng.choice([0, 1, 2, 63, 64, 65, int(rng.integers(3, 400))]))
    k = int(rng.choice([0, 1, 2, int(rng.integers(3, 120))]))
    span = max(1, int(k * rng.choice([0.5, 1.0, 1.5])))  # some ids never drawn, some >= k
    ids = rng.integers(0, span + 1, size=n).astype(np.uint32)
    ids[rng.random(n) < 0.1] = NO_ID
    kind = int(rng.integers(0, 4))
    if kind == 0:
        score = None
    elif kind == 1:
        score = rng.integers(0, 3, size=n).astype(np.uint32)  # many ties
    elif kind == 2:
        score = rng.choice(np.array([0, 1, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint32), size=n)
    else:
        score = rng.integers(0, 61, size=n).astype(np.uint32)
    return ids, score, k
