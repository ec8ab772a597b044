"""Two independent restatements of the UMI count matrix spec and a random-case
generator. Neither touches the library.

  (a) count_dict     a Python loop over the rows with one set of molecules per (cell, feature)
  (b) count_lexsort  numpy: a lexsort on (cell, feature, molecule), run heads by comparing neighbours

Both return a Counts of plain numpy arrays, entries ascending in (cell, feature) and cut at
`capacity` (None: all of them):
  cell, feature, n_umis, n_reads u32 [min(entries, capacity)],
  totals int64 [3] = (entries: the true count, live rows, sum of n_umis over ALL entries),
  indptr int64 [n_cells + 1]: the first written entry whose cell is >= c (None when not asked for).
A row is live when cell < n_cells, feature < n_features and molecule < n_molecules."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

NO_ID = 0xFFFFFFFF


@dataclass
class Counts:
    cell: np.ndarray
    feature: np.ndarray
    n_umis: np.ndarray
    n_reads: np.ndarray
    totals: np.ndarray
    indptr: np.ndarray


def bit_width(v: int) -> int:
    return int(v).bit_length() if v > 0 else 0


def key_bits(n_cells: int, n_features: int, n_molecules: int) -> int:
    """cb + fb + mb of the library's sort key."""
    return bit_width(n_cells) + bit_width(n_features - 1) + bit_width(n_molecules - 1)


def count_dict(cell, feature, molecule, n_cells: int, n_features: int, n_molecules: int, capacity=None,
               indptr: bool = True) -> Counts:
    mols, reads = {}, {}
    live = 0
    for c, f, m in zip((int(x) for x in cell), (int(x) for x in feature), (int(x) for x in molecule)):
        if c >= n_cells or f >= n_features or m >= n_molecules:
            continue
        live += 1
        mols.setdefault((c, f), set()).add(m)
        reads[(c, f)] = reads.get((c, f), 0) + 1
    pairs = sorted(mols)
    entries = len(pairs)
    total_umis = sum(len(mols[p]) for p in pairs)
    m = entries if capacity is None else min(entries, capacity)
    pairs = pairs[:m]
    ptr = None
    if indptr:
        per_cell = [0] * (n_cells + 1)
        for c, _ in pairs:
            per_cell[c + 1] += 1
        ptr = np.cumsum(np.array(per_cell, dtype=np.int64))
    u32 = lambda v: np.array(v, dtype=np.uint32)
    return Counts(u32([p[0] for p in pairs]), u32([p[1] for p in pairs]), u32([len(mols[p]) for p in pairs]),
                  u32([reads[p] for p in pairs]), np.array([entries, live, total_umis], dtype=np.int64), ptr)


def count_lexsort(cell, feature, molecule, n_cells: int, n_features: int, n_molecules: int, capacity=None,
                  indptr: bool = True) -> Counts:
    c = np.asarray(cell, dtype=np.int64)
    f = np.asarray(feature, dtype=np.int64)
    m = np.asarray(molecule, dtype=np.int64)
    live = (c < n_cells) & (f < n_features) & (m < n_molecules)
    c, f, m = c[live], f[live], m[live]
    order = np.lexsort((m, f, c))
    c, f, m = c[order], f[order], m[order]
    n = c.size
    new_entry = np.ones(n, dtype=bool)
    new_entry[1:] = (c[1:] != c[:-1]) | (f[1:] != f[:-1])
    new_mol = new_entry.copy()
    new_mol[1:] |= m[1:] != m[:-1]
    entry_of_row = np.cumsum(new_entry) - 1
    entries = int(new_entry.sum())
    n_reads = np.bincount(entry_of_row, minlength=entries).astype(np.uint32)
    n_umis = np.bincount(entry_of_row[new_mol], minlength=entries).astype(np.uint32)
    keep = entries if capacity is None else min(entries, capacity)
    ec, ef = c[new_entry][:keep], f[new_entry][:keep]
    ptr = np.searchsorted(ec, np.arange(n_cells + 1), side="left").astype(np.int64) if indptr else None
    return Counts(ec.astype(np.uint32), ef.astype(np.uint32), n_umis[:keep], n_reads[:keep],
                  np.array([entries, n, int(n_umis.sum())], dtype=np.int64), ptr)


def same(a: Counts, b: Counts) -> bool:
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("cell", "feature", "n_umis", "n_reads",
                                                                      "totals", "indptr"))


def bad_u32_tensors(host_column):
    """Tensors that are no u32 column beside a first int32 tensor of 4 rows on the CPU, each with
    the words the refusal has to name after the column's name."""
    import torch

    return [
        (torch.zeros(3, dtype=torch.int32), "has 3 rows"),                            # another length
        (torch.zeros(4, dtype=torch.float32), "must be a contiguous int32 / uint32"),  # float
        (torch.zeros(4, dtype=torch.int64), "must be a contiguous int32 / uint32"),    # not the u32 bits
        (torch.zeros((4, 1), dtype=torch.int32), "must be 1-D"),                       # not 1-D
        (torch.zeros(8, dtype=torch.int32)[::2], "must be a contiguous int32 / uint32"),  # not contiguous
        (torch.zeros(4, dtype=torch.int32, device="meta"), "is on meta"),              # another device
        (host_column, "must be a torch tensor"),                                       # not a tensor beside tensors
    ]


def random_case(seed: int, n=None):
    """(cell, feature, molecule u32, n_cells, n_features, n_molecules): small id spaces, so triples
    repeat and a molecule id turns up under several features and cells; rows skipped for each of
    the three causes (an id at or past its size, 0xFFFFFFFF); now and then no rows, a size of 0
    or 1, or empty cells at the front, inside and at the end."""
    rng = np.random.default_rng(seed)
    if n is None:
        n = int(rng.choice([0, 1, 2, 63, 64, 65, int(rng.integers(3, 500))]))
    sizes = [int(rng.choice([0, 1, 2, int(rng.integers(3, 40))], p=[0.04, 0.1, 0.16, 0.7])) for _ in range(3)]
    cols = []
    for k in sizes:
        lo = int(rng.integers(0, 3)) if k > 4 else 0           # empty leading ids
        hi = max(lo + 1, k - int(rng.integers(0, 3)))          # empty trailing ids
        v = rng.integers(lo, hi + 2, size=n).astype(np.uint32)  # hi, hi + 1 may be >= k: skipped
        if k > 6:
            v[v == k // 2] = k // 2 + 1                        # an empty interior id
        v[rng.random(n) < 0.06] = NO_ID
        v[rng.random(n) < 0.03] = np.uint32(k)                 # exactly the size
        cols.append(v)
    return cols[0], cols[1], cols[2], sizes[0], sizes[1], sizes[2]
