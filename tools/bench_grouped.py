#!/usr/bin/env python
"""Throughput of UMI clustering and correction within groups (rogtk_amd/csrc/grouped.hip,
DESIGN.md §4d).

Workload: the C2 shape, N synth-v1 UMIs of length 12 (default 10 M) resident in HBM as a string
column (int64 offsets, values), with one u32 key per row that keeps molecules together: the
ungrouped directional call runs once with root_code, and key = multiplicative hash of the row's
root code mod G, for G = 2^10 and 2^17. Timed with device events on one stream after a warm-up,
median of the timed steps, the operations alternating in this one process and build:

  directional_ids / directional_correct   the ungrouped calls on the same column: the yardstick
  grouped_ids_g10 / grouped_ids_g17       rogtk_umi_cluster_grouped_dev, directional, distance 1
  grouped_correct_g10 / _g17              rogtk_umi_correct_grouped_dev: ids + summary + gather
  grouped_ids_g17_value / _table          the same ids with the edge search bounded by value
                                          distance alone / clamped by a table of the key heads
                                          (the default, a galloped range, is grouped_ids_g17);
                                          also for g10

Reported besides: cluster counts, relaxation rounds, and one core of numpy + Python running the
per-key loop (the best-ancestor fixed point of tools/bench_directional.py once per key) over a
200 k-row sample, with the GPU's ids and root codes for the sample compared with it.

Not measured here: other umi_len, the host entries' transfer share, max_distance 0, irregular
strings at scale, keys that split molecules.

    python tools/bench_grouped.py [--rows 10000000] [--steps 10] [--warmup 3] [--out FILE]
    rocprofv3 --kernel-trace --stats ... -- python tools/bench_grouped.py --ops grouped_correct_g17

Prints one JSON line; --out also writes it to a file.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if path not in sys.path:
        sys.path.insert(0, path)

UMI_LEN = 12
GROUPS = {"g10": 1 << 10, "g17": 1 << 17}
WINDOWS = {"value": 0, "table": 1, "gallop": 2}
DEFAULT_WINDOW = "gallop"


def keys_of(root_codes: np.ndarray, n_groups: int) -> np.ndarray:
    """multiplicative hash of the root code mod n_groups: the rows of a molecule share a key"""
    h = (root_codes.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(32)
    return (h % np.uint64(n_groups)).astype(np.uint32)


def python_reference(codes: np.ndarray, keys: np.ndarray, L: int):
    """The per-key loop on one core. Returns (root code per row, cluster id per row, n_clusters)."""
    from bench_directional import python_reference as one_group

    order = np.argsort(keys, kind="stable")
    cuts = np.flatnonzero(np.diff(keys[order])) + 1
    root = np.empty(len(codes), dtype=np.uint64)
    for rows in np.split(order, cuts):
        root[rows] = one_group(codes[rows], L)[0]
    pairs = (keys.astype(np.uint64) << np.uint64(2 * L)) | root  # ids: ascending (key, root code)
    uniq, ids = np.unique(pairs, return_inverse=True)
    return root, ids.astype(np.uint32), len(uniq)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample", type=int, default=200_000, help="rows of the Python baseline (0: skip it)")
    ap.add_argument("--ops", default=None, help="comma-separated subset of the operations (for a profiler run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("bench_grouped needs a GPU (there is no CPU path to time)", file=sys.stderr)
        return 2
    from rogtk_amd import _lib, synth

    n, L = a.rows, UMI_LEN
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    s = ctypes.c_void_p(stream.cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    class Column:
        def __init__(self, codes_h):
            self.n = m = len(codes_h)
            self.off = (torch.arange(m + 1, dtype=torch.int64, device=dev) * L).contiguous()
            self.val = torch.from_numpy(np.ascontiguousarray(synth.codes_to_ascii(codes_h, L)).reshape(-1)).to(dev)
            self.cid = torch.empty(m, dtype=torch.int32, device=dev)
            self.root = torch.empty(m, dtype=torch.int64, device=dev)
            self.cgroup = torch.empty(m, dtype=torch.int32, device=dev)
            self.out = torch.empty(m * L, dtype=torch.uint8, device=dev)
            self.nk = ctypes.c_int64(0)
            self.keys = {}

        def make_keys(self):
            with torch.cuda.stream(stream):
                self.directional_ids(root=True)
                stream.synchronize()
            roots = self.root.cpu().numpy().view(np.uint64)
            for name, g in GROUPS.items():
                self.keys[name] = torch.from_numpy(keys_of(roots, g).view(np.int32)).to(dev)

        def directional_ids(self, root=False):
            _lib.call("rogtk_umi_cluster_directional_dev", p(self.off), p(self.val), None, self.n, L, p(self.cid),
                      ctypes.byref(self.nk), p(self.root) if root else None, s)

        def directional_correct(self):
            _lib.call("rogtk_umi_correct_directional_dev", p(self.off), p(self.val), None, self.n, L, p(self.cid),
                      ctypes.byref(self.nk), p(self.out), s)

        def grouped_ids(self, g, window=DEFAULT_WINDOW, root=False):
            _lib.call("rogtk_grouped_set_window", WINDOWS[window])
            try:
                _lib.call("rogtk_umi_cluster_grouped_dev", p(self.off), p(self.val), None, self.n, p(self.keys[g]), L,
                          1, 1, p(self.cid), ctypes.byref(self.nk), p(self.root) if root else None, p(self.cgroup), s)
            finally:
                _lib.call("rogtk_grouped_set_window", WINDOWS[DEFAULT_WINDOW])

        def grouped_correct(self, g):
            _lib.call("rogtk_umi_correct_grouped_dev", p(self.off), p(self.val), None, self.n, p(self.keys[g]), L, 1,
                      1, p(self.cid), ctypes.byref(self.nk), p(self.out), p(self.cgroup), s)

    codes_h = synth.umi_codes(n, L)
    col = Column(codes_h)
    col.make_keys()
    ops = {"directional_ids": col.directional_ids, "directional_correct": col.directional_correct}
    for g in GROUPS:
        ops[f"grouped_ids_{g}"] = lambda g=g: col.grouped_ids(g)
        ops[f"grouped_correct_{g}"] = lambda g=g: col.grouped_correct(g)
        for w in ("value", "table"):
            ops[f"grouped_ids_{g}_{w}"] = lambda g=g, w=w: col.grouped_ids(g, w)
    if a.ops:
        ops = {name: ops[name] for name in a.ops.split(",")}
    ms = {name: [] for name in ops}
    counts, rounds = {}, {}
    with torch.cuda.stream(stream):
        for _ in range(a.warmup):
            for fn in ops.values():
                fn()
        stream.synchronize()
        for _ in range(a.steps):  # the operations alternate, so drift hits them alike
            for name, fn in ops.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1))
        r = ctypes.c_int64(0)
        for name, fn in [("ungrouped", col.directional_ids)] + [(g, lambda g=g: col.grouped_ids(g)) for g in GROUPS]:
            fn()
            stream.synchronize()
            _lib.call("rogtk_directional_last_rounds", ctypes.byref(r))
            counts[name], rounds[name] = int(col.nk.value), int(r.value)

    result = {"kind": "bench_grouped", "device": torch.cuda.get_device_name(0), "rows": n, "umi_len": L,
              "steps": a.steps, "warmup": a.warmup, "groups": GROUPS, "default_window": DEFAULT_WINDOW,
              "distinct_keys": {g: int(len(torch.unique(k))) for g, k in col.keys.items()},
              "n_clusters": counts, "relaxation_rounds": rounds, "ops": {}}
    for name, v in ms.items():
        med = float(np.median(v))
        result["ops"][name] = {"kind": "gpu-events", "ms_median": med, "ms_min": float(min(v)),
                               "ms_max": float(max(v)), "rows_per_s": n / (med * 1e-3)}
    if a.ops or not a.sample:  # a profiler run: the timings of the chosen operations alone
        print(json.dumps(result))
        return 0
    med = {name: result["ops"][name]["ms_median"] for name in ops}
    result["ratios"] = {}
    for g in GROUPS:
        result["ratios"][f"grouped_ids_{g}_over_directional_ids"] = med[f"grouped_ids_{g}"] / med["directional_ids"]
        result["ratios"][f"grouped_correct_{g}_over_directional_correct"] = (
            med[f"grouped_correct_{g}"] / med["directional_correct"])
        for w in ("value", "table"):
            result["ratios"][f"grouped_ids_{g}_{w}_over_default"] = med[f"grouped_ids_{g}_{w}"] / med[f"grouped_ids_{g}"]

    # one core of numpy + Python on a sample (its own keys), and the GPU's answers for the same rows
    m = min(a.sample, n)
    sm = Column(codes_h[:m])
    sm.make_keys()
    result["python"], result["mismatches"] = {}, {}
    for g in GROUPS:
        with torch.cuda.stream(stream):
            sm.grouped_ids(g, root=True)
            stream.synchronize()
        g_ids = sm.cid.cpu().numpy().view(np.uint32)
        g_root = sm.root.cpu().numpy().view(np.uint64)
        g_k = int(sm.nk.value)
        keys_h = sm.keys[g].cpu().numpy().view(np.uint32)
        g_cgroup = sm.cgroup.cpu().numpy().view(np.uint32)[:g_k]
        t0 = time.perf_counter()
        r_root, r_ids, r_k = python_reference(codes_h[:m].astype(np.uint64), keys_h, L)
        t1 = time.perf_counter()
        result["python"][g] = {"kind": "python", "rows": m, "cores": 1, "seconds": t1 - t0,
                               "rows_per_s": m / (t1 - t0), "n_clusters": r_k}
        result["mismatches"][g] = {"cluster_id": int(np.count_nonzero(g_ids != r_ids)),
                                   "root_code": int(np.count_nonzero(g_root != r_root)), "n_clusters": int(g_k != r_k),
                                   "cluster_group": int(np.count_nonzero(g_cgroup[g_ids] != keys_h))}
    result["checked_rows"] = m
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if not any(v for mm in result["mismatches"].values() for v in mm.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
