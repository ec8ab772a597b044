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
from .columns import as_u32

NO_ID = 0xFFFFFFFF
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


def _is_tensor(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


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

    u32 = (torch.int32, torch.uint32)
    if cid.dim() != 1:
        raise ValueError(f"cluster_id must be 1-D, got shape {tuple(cid.shape)}")
    if cid.dtype not in u32 or not cid.is_contiguous():
        raise ValueError("cluster_id must be a contiguous int32 / uint32 device tensor (the u32 bits)")
    n = cid.numel()
    if score is not None:
        if not _is_tensor(score) or score.device != cid.device:
            raise ValueError("score must be a tensor on cluster_id's device")
        if score.dtype not in u32 or not score.is_contiguous():
            raise ValueError("score must be a contiguous int32 / uint32 device tensor (the u32 bits)")
        if tuple(score.shape) != (n,):
            raise ValueError(f"score has shape {tuple(score.shape)}, cluster_id has {n} rows")
    dev = cid.device
    if k < 0:
        ids = cid.view(torch.int32).to(torch.int64) & NO_ID
        ids = ids[ids != NO_ID]
        k = int(ids.max().item()) + 1 if ids.numel() else 0
    if not 0 <= k < NO_ID:
        raise ValueError(f"n_clusters {k} outside 0..2^32-2")
    with torch.cuda.device(dev):
        tb = ctypes.c_int64(0)
        _lib.call("rogtk_cluster_best_temp_bytes", n, k, ctypes.byref(tb))
        temp = torch.empty(tb.value, dtype=torch.uint8, device=dev)
        best_row = torch.empty(k, dtype=torch.int64, device=dev)
        best_score = torch.empty(k, dtype=torch.int32, device=dev)
        n_reads = torch.empty(k, dtype=torch.int32, device=dev)
        words = torch.empty((n + 63) // 64, dtype=torch.int64, device=dev)
        kept = torch.empty(min(n, k), dtype=torch.int64, device=dev)
        n_kept = torch.empty(1, dtype=torch.int64, device=dev)
        p = lambda t: None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())
        _lib.call("rogtk_cluster_best_rows", p(cid), p(score), n, k, p(best_row), p(best_score), p(n_reads), p(words),
                  p(kept), p(n_kept), p(temp), tb.value, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        m = int(n_kept.item())
    best = {"best_row": best_row, "best_score": best_score, "n_reads": n_reads}
    return DedupResult(words, kept[:m], best, m, None, k)


def cluster_best_rows(cluster_id, score=None, n_clusters: int = -1) -> DedupResult:
    """The kept row of every cluster id. cluster_id: u32 ids, dense
    0..n_clusters-1; an id >= n_clusters (0xFFFFFFFF, which an Arrow null becomes, among them)
    is skipped. score: one u32 per row, absent = all 0. n_clusters < 0: 1 + the largest id other
    than 0xFFFFFFFF (0 if none). Host arrays (numpy / Arrow) give Arrow out; torch device
    tensors give torch tensors out (keep as int64 bitmap words, best as a dict of tensors)."""
    if _is_tensor(cluster_id):
        return _best_rows_device(cluster_id, score, int(n_clusters))
    cid = as_u32(cluster_id, "cluster_id", nulls_to=NO_ID)
    sc = None if score is None else as_u32(score, "score", rows=cid.size)
    k = int(n_clusters)
    if k < 0:
        real = cid[cid != NO_ID]
        k = int(real.max()) + 1 if real.size else 0
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
