"""The UMI count matrix: molecules and reads per (cell, feature).

The table that barcode correction, UMI clustering and deduplication lead to, on the GPU
(rogtk_amd/csrc/count_matrix.hip): for every (cell, feature) pair with at least one live row
the number of distinct molecule ids and the number of rows, entries ascending in (cell,
feature), with the CSR row pointer over the cells. A row is live when each of its three ids is
below its size; every other row (0xFFFFFFFF, which a rejected barcode, a null gene and a null
UMI row's cluster id use, among them) is counted nowhere. The reference has no counterpart: its
callers group on the host.

    cells = whitelist.correct(cbcs).keys
    m = rg.umi_count(umis, 12, cells, genes, n_cells, n_genes)   # cluster per (cell, gene), count
    m.cell, m.feature, m.n_umis, m.n_reads     # pa.UInt32Array, entries ascending in (cell, feature)
    m.indptr                                   # pa.Int64Array [n_cells + 1]: the CSR row pointer
    m.shape, m.nnz, m.n_live, m.n_molecules_counted
    m.to_scipy()                               # scipy.sparse.csr_matrix of n_umis
    rg.count_matrix(cell, feature, molecule)   # the same for the caller's own molecule ids
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Any, Tuple

import numpy as np
import pyarrow as pa

from . import _lib
from .columns import NO_ID, as_u32, current_stream, dev_ptr, device_temp, is_tensor, largest_plus_one, u32_tensor

SIZES = ("n_cells", "n_features", "n_molecules")


@dataclass
class CountMatrix:
    cell: Any
    feature: Any
    n_umis: Any
    n_reads: Any
    indptr: Any
    shape: Tuple[int, int]
    nnz: int
    n_live: int
    n_molecules_counted: int
    cluster_id: Any = None
    n_clusters: int = 0

    def _host(self, x, dtype) -> np.ndarray:
        """A field as a numpy array, whichever kind of call made it."""
        if isinstance(x, pa.Array):
            return np.asarray(x.to_numpy(zero_copy_only=False), dtype=dtype)
        return x.cpu().numpy().view(dtype)

    def to_scipy(self):
        """The matrix of n_umis as a scipy.sparse.csr_matrix of shape (n_cells, n_features)."""
        try:
            from scipy.sparse import csr_matrix
        except ImportError as e:
            raise ImportError("CountMatrix.to_scipy() needs scipy, which is not installed") from e
        data, col = self._host(self.n_umis, np.uint32), self._host(self.feature, np.uint32).astype(np.int64)
        if self.indptr is None:
            return csr_matrix((data, (self._host(self.cell, np.uint32).astype(np.int64), col)), shape=self.shape)
        return csr_matrix((data, col, self._host(self.indptr, np.int64)), shape=self.shape)

    def umis_per_cell(self) -> np.ndarray:
        """int64 [n_cells]: the molecules of every cell, summed over its features."""
        cell = self._host(self.cell, np.uint32).astype(np.int64)
        w = self._host(self.n_umis, np.uint32).astype(np.int64)
        out = np.zeros(self.shape[0], dtype=np.int64)
        np.add.at(out, cell, w)
        return out

    def features_per_cell(self) -> np.ndarray:
        """int64 [n_cells]: the features with at least one molecule in every cell."""
        cell = self._host(self.cell, np.uint32).astype(np.int64)
        return np.bincount(cell, minlength=self.shape[0]).astype(np.int64)


def geometry() -> dict:
    """The kernels' constants: sorted positions per flag / emit tile and the scan's workgroup."""
    out = (ctypes.c_int64 * 2)()
    _lib.call("rogtk_count_matrix_geometry", out)
    return {"tile": int(out[0]), "scan_block": int(out[1])}


def _check_sizes(sizes) -> None:
    for name, v in zip(SIZES, sizes):
        if not 0 <= v <= NO_ID:
            raise ValueError(f"{name} {v} outside 0..2^32-1")


def _capacity(n: int, sizes) -> int:
    return min(n, sizes[0] * sizes[1])


def _count_host(cols, sizes, want_indptr: bool) -> CountMatrix:
    n = cols[0].size
    nc = sizes[0]
    cap = _capacity(n, sizes)
    out = [np.empty(cap, np.uint32) for _ in range(4)]
    indptr = np.empty(nc + 1, np.int64) if want_indptr else None
    totals = np.zeros(3, np.int64)
    p = lambda a: _lib.ptr(a, null_if_empty=True)
    _lib.call("rogtk_count_matrix_host", p(cols[0]), p(cols[1]), p(cols[2]), n, *sizes, *(p(a) for a in out), cap,
              _lib.ptr(indptr), _lib.ptr(totals))
    nnz = min(int(totals[0]), cap)
    arrays = [pa.array(a[:nnz], type=pa.uint32()) for a in out]
    return CountMatrix(*arrays, None if indptr is None else pa.array(indptr, type=pa.int64()), (nc, sizes[1]), nnz,
                       int(totals[1]), int(totals[2]))


def _count_device(cols, sizes, want_indptr: bool) -> CountMatrix:
    """torch tensors in and out, on the columns' device and the current stream (synchronised once,
    for totals). The u32 columns are int32 (or uint32) tensors holding the u32 bits."""
    import torch

    for name, t in zip(("cell", "feature", "molecule"), cols):
        u32_tensor(t, name, cols[0], "cell")
    dev, n = cols[0].device, cols[0].numel()
    sizes = [s if s >= 0 else largest_plus_one(t) for s, t in zip(sizes, cols)]
    _check_sizes(sizes)
    nc = sizes[0]
    cap = _capacity(n, sizes)
    with torch.cuda.device(dev):
        temp = device_temp("rogtk_count_matrix_temp_bytes", n, *sizes, cap, device=dev)
        out = [torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(4)]
        indptr = torch.empty(nc + 1, dtype=torch.int64, device=dev) if want_indptr else None
        totals = torch.empty(3, dtype=torch.int64, device=dev)
        _lib.call("rogtk_count_matrix", *map(dev_ptr, cols), n, *sizes, *map(dev_ptr, out), cap,
                  *map(dev_ptr, (indptr, totals, temp)), temp.numel(), current_stream())
        tot = totals.cpu().tolist()
    nnz = min(int(tot[0]), cap)
    return CountMatrix(*(t[:nnz] for t in out), indptr, (nc, sizes[1]), nnz, int(tot[1]), int(tot[2]))


def count_matrix(cell, feature, molecule, n_cells: int = -1, n_features: int = -1, n_molecules: int = -1,
                 indptr: bool = True) -> CountMatrix:
    """Molecules and reads per (cell, feature). The three columns hold u32 ids;
    a row with an id at or past its size (0xFFFFFFFF, which an Arrow null becomes, among them)
    is skipped. A negative size: 1 + the column's largest value other than 0xFFFFFFFF (0 if
    none). Host arrays (numpy / Arrow) give Arrow out; torch device tensors give torch tensors
    out on the same device. indptr=False leaves the CSR row pointer out."""
    sizes = [int(n_cells), int(n_features), int(n_molecules)]
    if is_tensor(cell):
        return _count_device((cell, feature, molecule), sizes, bool(indptr))
    cols = [as_u32(cell, "cell", nulls_to=NO_ID)]
    cols.append(as_u32(feature, "feature", rows=cols[0].size, nulls_to=NO_ID))
    cols.append(as_u32(molecule, "molecule", rows=cols[0].size, nulls_to=NO_ID))
    sizes = [s if s >= 0 else largest_plus_one(c) for s, c in zip(sizes, cols)]
    _check_sizes(sizes)
    return _count_host(cols, sizes, bool(indptr))


def umi_count(umis, umi_len: int, cells, features, n_cells: int, n_features: int, max_distance: int = 1,
              method: str = "directional") -> CountMatrix:
    """``umi_cluster(umis, umi_len, max_distance, method, groups=key)`` with one key per (cell,
    feature) pair, cell * n_features + feature (0xFFFFFFFF for a row whose cell or feature is
    out of range), followed by ``count_matrix(cells, features, ids, n_cells, n_features,
    n_clusters)``. Every method / max_distance rule and refusal is the clustering call's. The
    result also carries cluster_id and n_clusters."""
    from .api import umi_cluster

    n_cells, n_features = int(n_cells), int(n_features)
    _check_sizes((n_cells, n_features, 0))
    if n_cells * n_features > NO_ID:
        raise ValueError(f"n_cells {n_cells} x n_features {n_features} pairs do not fit a u32 group key: rank the "
                         "(cell, feature) pairs that occur yourself and pass the ranks to umi_cluster(groups=) and "
                         "the cluster ids to count_matrix")
    c = as_u32(cells, "cells", rows=len(umis), nulls_to=NO_ID)
    f = as_u32(features, "features", rows=len(umis), nulls_to=NO_ID)
    ok = (c < n_cells) & (f < n_features)
    key = np.where(ok, c.astype(np.uint64) * np.uint64(n_features) + f, NO_ID).astype(np.uint32)
    ids, k, _ = umi_cluster(umis, umi_len, max_distance, method, key)
    res = count_matrix(c, f, ids, n_cells, n_features, k)
    res.cluster_id, res.n_clusters = ids, k
    return res
