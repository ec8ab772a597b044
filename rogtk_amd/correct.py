"""UMI correction: cluster representatives, sizes and corrected UMIs.

The step after ``umi_cluster`` that every consumer of UMI clusters takes next, on the GPU
(rogtk_amd/csrc/correct.hip): per cluster the representative UMI (the distinct string
with the most rows; ties go to regular strings, then to the byte-lexicographically
smallest), its read count and its distinct-UMI count, and per row the representative of
its cluster. The reference has no counterpart: its callers ``group_by('umi')`` on the
host (rogtk/__init__.py:206-214).

    res = rg.umi_correct(umis, max_distance=1)
    res.corrected       # string array, nulls as the input's
    res.cluster_id      # pa.UInt32Array
    res.n_clusters      # int
    res.clusters        # StructArray{representative, n_reads, n_distinct}, cluster-id order
    rg.umi_cluster_summary(umis, my_ids)          # the same table for the caller's ids
    rg.col(umis).umi.correct(max_distance=1)      # the corrected column alone
    rg.umi_correct(umis, method="directional")    # count-aware clusters
    rg.umi_correct(umis, 12, method="directional", groups=cell_ids)   # within each key (§4d);
                                                  # clusters then has a fourth field, group
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import pyarrow as pa

from . import _lib
from .columns import ColumnLike, as_u32, one_chunk, text_type, validity_buffer

CLUSTER_FIELDS = ("representative", "n_reads", "n_distinct")


@dataclass
class UmiCorrection:
    corrected: pa.Array
    cluster_id: pa.Array
    n_clusters: int
    clusters: pa.StructArray
    umi_len: int = 0


def _clusters(tables) -> pa.StructArray:
    """representative, n_reads, n_distinct and, from a grouped call, group."""
    return pa.StructArray.from_arrays(tables, names=(list(CLUSTER_FIELDS) + ["group"])[:len(tables)])


def umi_correct(column: ColumnLike, umi_len: int = 0, max_distance: int = 1,
                method: str = "cluster", groups=None) -> UmiCorrection:
    """Clusters of the column (as ``umi_cluster``: method="cluster" the H3 components,
    "directional" the count-aware rule of DESIGN.md §4c), their summary and the corrected
    UMI of every row. A multi-chunk column is one batch. groups (one unsigned 32-bit key per
    row): clusters form within each key, and ``clusters`` gains a fourth field
    ``group``, the key of every cluster."""
    from .api import grouped_method, umi_method_entry

    grouped = groups is not None
    if grouped:
        entry, m = "rogtk_umi_correct_grouped_host", grouped_method(method, max_distance)
    else:
        entry = umi_method_entry(method, max_distance, "rogtk_umi_correct_host", "rogtk_umi_correct_directional_host")
    ch = one_chunk(column)
    n = ch.n
    cid = np.zeros(max(n, 1), dtype=np.uint32)
    results = [_lib.StrResult(), _lib.StrResult(), _lib.U32Result(), _lib.U32Result()]  # corrected, then the tables
    nclu, rl = ctypes.c_int64(0), ctypes.c_int(0)
    rule = [int(umi_len), int(max_distance)]
    if grouped:  # the keys before the rule, the method in it, the clusters' keys after the tables
        keys = as_u32(groups, "groups", rows=n)
        rule = [_lib.ptr(keys, null_if_empty=True), rule[0], m, rule[1]]
        results.append(_lib.U32Result())
    desc = ch.desc()
    _lib.call(entry, ctypes.byref(desc), *rule, _lib.ptr(cid), *[ctypes.byref(r) for r in results],
              ctypes.byref(nclu), ctypes.byref(rl))
    out, *tables = _lib.take_all(results, text_type(ch))
    ids = pa.Array.from_buffers(pa.uint32(), n, [validity_buffer(ch), pa.py_buffer(cid[:n])])
    return UmiCorrection(out, ids, int(nclu.value), _clusters(tables), int(rl.value))


def umi_cluster_summary(column: ColumnLike, cluster_id, n_clusters: int = -1, umi_len: int = 0) -> pa.StructArray:
    """The ``clusters`` table for caller-supplied ids (dense 0..n_clusters-1; ids of null rows
    are ignored). n_clusters < 0: 1 + the largest id of a non-null row. umi_len (0: the
    length of the first non-null row) decides which strings are regular in a count tie."""
    ch = one_chunk(column)
    n = ch.n
    cid = as_u32(cluster_id, "cluster_id", rows=n, nulls_to=0xFFFFFFFF)
    if n_clusters < 0:
        valid = np.asarray(ch.arrow.is_valid().to_numpy(zero_copy_only=False), dtype=bool) if n else np.zeros(0, bool)
        n_clusters = int(cid[valid].max()) + 1 if valid.any() else 0
    if cid.size == 0:
        cid = np.zeros(1, dtype=np.uint32)
    results = [_lib.StrResult(), _lib.U32Result(), _lib.U32Result()]
    desc = ch.desc()
    _lib.call("rogtk_cluster_summary_host", ctypes.byref(desc), int(umi_len), _lib.ptr(cid), int(n_clusters),
              *[ctypes.byref(r) for r in results])
    return _clusters(_lib.take_all(results, text_type(ch)))
