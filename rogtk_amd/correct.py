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
from .columns import ColumnLike, _one_chunk, validity_buffer

CLUSTER_FIELDS = ("representative", "n_reads", "n_distinct")


@dataclass
class UmiCorrection:
    corrected: pa.Array
    cluster_id: pa.Array
    n_clusters: int
    clusters: pa.StructArray
    umi_len: int = 0


def _desc(ch) -> _lib.StrCol:
    o, v, val = ch.ptrs()
    return _lib.StrCol(o, ch.offset_width, v, ch.values.size, val, ch.validity_offset, ch.n)


def _text_type(ch):
    t = ch.arrow.type
    return pa.large_binary() if pa.types.is_binary(t) or pa.types.is_large_binary(t) else pa.large_string()


def _take_str(res: _lib.StrResult, typ) -> pa.Array:
    """Copies of a rogtk_str_result's buffers as an Arrow array (the caller frees the result)."""
    n = int(res.n)
    offs = np.ctypeslib.as_array(ctypes.cast(res.offsets, ctypes.POINTER(ctypes.c_int64)), (n + 1,)).copy()
    nv = int(res.values_len)
    vals = np.ctypeslib.as_array(ctypes.cast(res.values, ctypes.POINTER(ctypes.c_uint8)), (max(nv, 1),))[:nv].copy()
    nulls = int(res.null_count)
    vb = None
    if nulls:
        nbytes = max((n + 63) // 64 * 8, 8)
        vb = pa.py_buffer(np.ctypeslib.as_array(ctypes.cast(res.validity, ctypes.POINTER(ctypes.c_uint8)),
                                                (nbytes,)).copy())
    return pa.Array.from_buffers(typ, n, [vb, pa.py_buffer(offs), pa.py_buffer(vals)], null_count=nulls)


def _take_u32(res: _lib.U32Result) -> pa.Array:
    n = int(res.n)
    a = np.ctypeslib.as_array(ctypes.cast(res.data, ctypes.POINTER(ctypes.c_uint32)), (max(n, 1),))[:n].copy()
    return pa.array(a, type=pa.uint32())


def _clusters(reps, n_reads, n_distinct, typ) -> pa.StructArray:
    return pa.StructArray.from_arrays([_take_str(reps, typ), _take_u32(n_reads), _take_u32(n_distinct)],
                                      names=list(CLUSTER_FIELDS))


def umi_correct(column: ColumnLike, umi_len: int = 0, max_distance: int = 1,
                method: str = "cluster", groups=None) -> UmiCorrection:
    """Clusters of the column (as ``umi_cluster``: method="cluster" the H3 components,
    "directional" the count-aware rule of DESIGN.md §4c), their summary and the corrected
    UMI of every row. A multi-chunk column is one batch. groups (one unsigned 32-bit key per
    row): clusters form within each key, and ``clusters`` gains a fourth field
    ``group``, the key of every cluster."""
    from .api import group_keys, grouped_method, umi_method_entry

    grouped = groups is not None
    if grouped:
        entry, m = "rogtk_umi_correct_grouped_host", grouped_method(method, max_distance)
    else:
        entry = umi_method_entry(method, max_distance, "rogtk_umi_correct_host", "rogtk_umi_correct_directional_host")
    ch = _one_chunk(column)
    n = ch.n
    cid = np.zeros(max(n, 1), dtype=np.uint32)
    corrected, reps = _lib.StrResult(), _lib.StrResult()
    n_reads, n_distinct, cgroup = _lib.U32Result(), _lib.U32Result(), _lib.U32Result()
    nclu, rl = ctypes.c_int64(0), ctypes.c_int(0)
    rule = [int(umi_len), int(max_distance)]
    outs = [ctypes.byref(r) for r in (corrected, reps, n_reads, n_distinct)]
    if grouped:  # the keys before the rule, the method in it, the clusters' keys after the tables
        keys = group_keys(groups, n)
        rule = [ctypes.c_void_p(keys.ctypes.data) if n else None, rule[0], m, rule[1]]
        outs.append(ctypes.byref(cgroup))
    desc = _desc(ch)
    lib = _lib.hip()
    _lib.check(getattr(lib, entry)(ctypes.byref(desc), *rule, ctypes.c_void_p(cid.ctypes.data), *outs,
                                   ctypes.byref(nclu), ctypes.byref(rl)))
    try:
        typ = _text_type(ch)
        out = _take_str(corrected, typ)
        clusters = _clusters(reps, n_reads, n_distinct, typ)
        if grouped:
            clusters = pa.StructArray.from_arrays(clusters.flatten() + [_take_u32(cgroup)],
                                                  names=list(CLUSTER_FIELDS) + ["group"])
    finally:
        lib.rogtk_str_result_free(ctypes.byref(corrected))
        lib.rogtk_str_result_free(ctypes.byref(reps))
        for r in (n_reads, n_distinct, cgroup):
            lib.rogtk_u32_result_free(ctypes.byref(r))
    ids = pa.Array.from_buffers(pa.uint32(), n, [validity_buffer(ch), pa.py_buffer(cid[:n])])
    return UmiCorrection(out, ids, int(nclu.value), clusters, int(rl.value))


def umi_cluster_summary(column: ColumnLike, cluster_id, n_clusters: int = -1, umi_len: int = 0) -> pa.StructArray:
    """The ``clusters`` table for caller-supplied ids (dense 0..n_clusters-1; ids of null rows
    are ignored). n_clusters < 0: 1 + the largest id of a non-null row. umi_len (0: the
    length of the first non-null row) decides which strings are regular in a count tie."""
    ch = _one_chunk(column)
    n = ch.n
    if isinstance(cluster_id, (pa.Array, pa.ChunkedArray)):
        cluster_id = cluster_id.fill_null(0xFFFFFFFF).to_numpy(zero_copy_only=False)
    cid = np.ascontiguousarray(cluster_id, dtype=np.uint32)
    if cid.shape != (n,):
        raise ValueError(f"cluster_id has shape {cid.shape}, the column has {n} rows")
    if n_clusters < 0:
        valid = np.asarray(ch.arrow.is_valid().to_numpy(zero_copy_only=False), dtype=bool) if n else np.zeros(0, bool)
        n_clusters = int(cid[valid].max()) + 1 if valid.any() else 0
    if cid.size == 0:
        cid = np.zeros(1, dtype=np.uint32)
    reps = _lib.StrResult()
    n_reads, n_distinct = _lib.U32Result(), _lib.U32Result()
    desc = _desc(ch)
    lib = _lib.hip()
    _lib.check(lib.rogtk_cluster_summary_host(ctypes.byref(desc), int(umi_len), ctypes.c_void_p(cid.ctypes.data),
                                              int(n_clusters), ctypes.byref(reps), ctypes.byref(n_reads),
                                              ctypes.byref(n_distinct)))
    try:
        return _clusters(reps, n_reads, n_distinct, _text_type(ch))
    finally:
        lib.rogtk_str_result_free(ctypes.byref(reps))
        lib.rogtk_u32_result_free(ctypes.byref(n_reads))
        lib.rogtk_u32_result_free(ctypes.byref(n_distinct))
