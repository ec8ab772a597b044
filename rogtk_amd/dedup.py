"""UMI deduplication: the read to keep per cluster, the keep mask and the kept rows.

The step after ``umi_cluster`` that UMI-tools calls ``dedup``, on the GPU
(rogtk_amd/csrc/dedup.hip): per cluster id the row with the largest score (on a tie the
smallest row index), its score and the cluster's row count; per row whether it is that row.
A row whose id is >= n_clusters (0xFFFFFFFF, a null row, among them) is never kept and never
counted. The reference has no counterpart: its callers sort or group on the host.

    res = rg.umi_dedup(umis, 12, score=mapq, method="directional", groups=cell_ids)
    res.keep            # pa.BooleanArray, no nulls: table.filter(res.keep)
    res.rows            # pa.Int64Array, the kept rows ascending
    res.best            # StructArray{best_row, best_score, n_reads}, cluster-id order
    res.n_kept          # clusters with at least one row
    res.cluster_id, res.n_clusters, res.umi_len        # as rg.umi_cluster returns them
    rg.cluster_best_rows(my_ids, score=mapq)           # the same for the caller's ids
    rg.col(umis).umi.dedup(12, score=mapq)             # the keep mask alone
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Any, Optional

import numpy as np
import pyarrow as pa

from . import _lib
from .columns import NO_ID, as_u32, current_stream, dev_ptr, device_temp, is_tensor, largest_plus_one, u32_tensor

BEST_FIELDS = ("best_row", "best_score", "n_reads")


@dataclass
class DedupResult:
    keep: Any
    rows: Any
    best: Any
    n_kept: int
    cluster_id: Any = None
    n_clusters: int = 0
    umi_len: int = 0


def geometry() -> dict:
    """The kernels' constants: rows per select tile, rows per keep / compaction tile, the LDS
    slots of the select table and the probes per row."""
    out = (ctypes.c_int64 * 4)()
    _lib.call("rogtk_cluster_best_geometry", out)
    return {"select_tile": int(out[0]), "keep_tile": int(out[1]), "slots": int(out[2]), "probes": int(out[3])}


def _best_rows_host(cid: np.ndarray, sc: Optional[np.ndarray], k: int) -> DedupResult:
    n = cid.size
    if not 0 <= k < NO_ID:
        raise ValueError(f"n_clusters {k} outside 0..2^32-2")
    best_row = np.empty(k, np.int64)
    best_score = np.empty(k, np.uint32)
    n_reads = np.empty(k, np.uint32)
    words = np.empty((n + 63) // 64, np.uint64)
    kept = np.empty(min(n, k), np.int64)
    n_kept = ctypes.c_int64(0)
    p = lambda a: _lib.ptr(a, null_if_empty=True)
    _lib.call("rogtk_cluster_best_rows_host", p(cid), p(sc), n, k, p(best_row), p(best_score), p(n_reads), p(words),
              p(kept), ctypes.byref(n_kept))
    keep = pa.Array.from_buffers(pa.bool_(), n, [None, pa.py_buffer(words)], null_count=0)
    best = pa.StructArray.from_arrays(
        [pa.array(best_row, type=pa.int64()), pa.array(best_score, type=pa.uint32()),
         pa.array(n_reads, type=pa.uint32())], names=list(BEST_FIELDS))
    return DedupResult(keep, pa.array(kept[:n_kept.value], type=pa.int64()), best, int(n_kept.value), None, k)


def _best_rows_device(cid, score, k: int) -> DedupResult:
    """torch tensors in and out, on cluster_id's device and the current stream (synchronised
    once, for n_kept). The u32 columns are int32 (or uint32) tensors holding the u32 bits;
    keep is the bitmap as int64 words."""
    import torch

    u32_tensor(cid, "cluster_id")
    if score is not None:
        u32_tensor(score, "score", cid, "cluster_id")
    n, dev = cid.numel(), cid.device
    if k < 0:
        k = largest_plus_one(cid)
    if not 0 <= k < NO_ID:
        raise ValueError(f"n_clusters {k} outside 0..2^32-2")
    with torch.cuda.device(dev):
        temp = device_temp("rogtk_cluster_best_temp_bytes", n, k, device=dev)
        best_row = torch.empty(k, dtype=torch.int64, device=dev)
        best_score = torch.empty(k, dtype=torch.int32, device=dev)
        n_reads = torch.empty(k, dtype=torch.int32, device=dev)
        words = torch.empty((n + 63) // 64, dtype=torch.int64, device=dev)
        kept = torch.empty(min(n, k), dtype=torch.int64, device=dev)
        n_kept = torch.empty(1, dtype=torch.int64, device=dev)
        _lib.call("rogtk_cluster_best_rows", *map(dev_ptr, (cid, score)), n, k,
                  *map(dev_ptr, (best_row, best_score, n_reads, words, kept, n_kept, temp)), temp.numel(),
                  current_stream())
        m = int(n_kept.item())
    best = {"best_row": best_row, "best_score": best_score, "n_reads": n_reads}
    return DedupResult(words, kept[:m], best, m, None, k)


def cluster_best_rows(cluster_id, score=None, n_clusters: int = -1) -> DedupResult:
    """The kept row of every cluster id. cluster_id: u32 ids, dense
    0..n_clusters-1; an id >= n_clusters (0xFFFFFFFF, which an Arrow null becomes, among them)
    is skipped. score: one u32 per row, absent = all 0. n_clusters < 0: 1 + the largest id other
    than 0xFFFFFFFF (0 if none). Host arrays (numpy / Arrow) give Arrow out; torch device
    tensors give torch tensors out (keep as int64 bitmap words, best as a dict of tensors)."""
    if is_tensor(cluster_id):
        return _best_rows_device(cluster_id, score, int(n_clusters))
    cid = as_u32(cluster_id, "cluster_id", nulls_to=NO_ID)
    sc = None if score is None else as_u32(score, "score", rows=cid.size)
    k = int(n_clusters)
    if k < 0:
        k = largest_plus_one(cid)
    return _best_rows_host(cid, sc, k)


def umi_dedup(column, umi_len: int = 0, score=None, max_distance: int = 1, method: str = "cluster",
              groups=None) -> DedupResult:
    """``umi_cluster(column, umi_len, max_distance, method, groups)`` followed by the selection:
    every method / groups rule and refusal is that call's. Null UMI rows are never kept."""
    from .api import umi_cluster

    sc = None if score is None else as_u32(score, "score", rows=len(column))
    ids, k, rl = umi_cluster(column, umi_len, max_distance, method, groups)
    res = cluster_best_rows(ids, sc, k)
    res.cluster_id, res.n_clusters, res.umi_len = ids, k, rl
    return res
