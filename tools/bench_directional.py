#!/usr/bin/env python
"""Throughput of directional UMI clustering and correction (rogtk_amd/csrc/directional.hip,
DESIGN.md §4c).

Workload: the C2 shape, N synth-v1 UMIs of length 12 (default 10 M) resident in HBM as a string
column (int64 offsets, values). Timed with device events on one stream after a warm-up, median
of the timed steps, all in this one process and build:

  directional_ids      rogtk_umi_cluster_directional_dev (count -> edges -> relax -> label -> rows)
  directional_correct  rogtk_umi_correct_directional_dev: the same ids + summary + gather
  transitive_ids       rogtk_umi_cluster_dev, max_distance 1
  transitive_correct   rogtk_umi_correct_dev, max_distance 1: its ids + summary + gather
  c2_cluster           the C2 cluster step on the packed codes (cluster engine, max_distance 1)

The yardstick is the transitive summary + gather of the same run, transitive_correct -
transitive_ids; the JSON records the directional ids and the whole directional correction as
ratios to it. n_clusters under both methods and the relaxation rounds are reported. One core
of numpy + Python runs the best-ancestor fixed point (restatement (b) of the spec) on a 200 k-row
sample, and the GPU's ids and root codes for that sample are compared with it.

Not measured here: other umi_len, the host entries' transfer share, irregular strings at scale.

    python tools/bench_directional.py [--rows 10000000] [--steps 10] [--warmup 3] [--out FILE]
    rocprofv3 --kernel-trace --stats ... -- python tools/bench_directional.py --ops directional_correct

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
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

UMI_LEN = 12


def python_reference(codes: np.ndarray, L: int):
    """Restatement (b) on one core: distinct codes and counts (numpy), in-edges by dict lookups
    of the 3 L neighbours, best[v] = max over in-neighbours to the fixed point. Returns
    (root code per row, cluster id per row, n_clusters, rounds)."""
    D, inv, C = np.unique(codes, return_inverse=True, return_counts=True)
    at = {int(c): j for j, c in enumerate(D.tolist())}
    cnt = C.tolist()
    into = []
    for j, c in enumerate(D.tolist()):
        need = 2 * cnt[j] - 1
        us = []
        for p in range(L):
            for x in (1, 2, 3):
                u = at.get(c ^ (x << (2 * p)))
                if u is not None and cnt[u] >= need:
                    us.append(u)
        into.append(us)
    best = [(cnt[j], -j) for j in range(len(cnt))]
    rounds, changed = 0, True
    while changed:
        changed = False
        rounds += 1
        for v, us in enumerate(into):
            b = best[v]
            for u in us:
                if best[u] > b:
                    b = best[u]
            if b != best[v]:
                best[v] = b
                changed = True
    root = np.array([-b[1] for b in best], dtype=np.int64)
    is_root = root == np.arange(len(root))
    rank = np.cumsum(is_root) - 1
    return D[root][inv], rank[root][inv].astype(np.uint32), int(is_root.sum()), rounds


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
        print("bench_directional needs a GPU (there is no CPU path to time)", file=sys.stderr)
        return 2
    from rogtk_amd import _lib, synth
    from rogtk_amd import device as D

    n, L = a.rows, UMI_LEN
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    s = ctypes.c_void_p(stream.cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    class Column:
        """m rows of the synth-v1 column on the device, as strings and as packed codes."""

        def __init__(self, codes_h):
            self.n = m = len(codes_h)
            self.codes = torch.from_numpy(codes_h.view(np.int32).copy()).to(dev)
            self.off = (torch.arange(m + 1, dtype=torch.int64, device=dev) * L).contiguous()
            self.val = torch.from_numpy(np.ascontiguousarray(synth.codes_to_ascii(codes_h, L)).reshape(-1)).to(dev)
            self.cid = torch.empty(m, dtype=torch.int32, device=dev)
            self.root = torch.empty(m, dtype=torch.int64, device=dev)
            self.out = torch.empty(m * L, dtype=torch.uint8, device=dev)
            self.nk = ctypes.c_int64(0)
            self.engine = D.ClusterEngine(L, min(m, 4 ** L), dev)

        def directional_ids(self, root=False):
            _lib.call("rogtk_umi_cluster_directional_dev", p(self.off), p(self.val), None, self.n, L, p(self.cid),
                      ctypes.byref(self.nk), p(self.root) if root else None, s)

        def directional_correct(self):
            _lib.call("rogtk_umi_correct_directional_dev", p(self.off), p(self.val), None, self.n, L, p(self.cid),
                      ctypes.byref(self.nk), p(self.out), s)

        def transitive_ids(self):
            _lib.call("rogtk_umi_cluster_dev", p(self.off), p(self.val), None, self.n, L, 1, p(self.cid),
                      ctypes.byref(self.nk), s)

        def transitive_correct(self):
            _lib.call("rogtk_umi_correct_dev", p(self.off), p(self.val), None, self.n, L, 1, p(self.cid),
                      ctypes.byref(self.nk), p(self.out), s)

        def c2_cluster(self):
            D.cluster_batch(self.engine, D.PackedBatch(self.codes, L), self.cid, 1)

    codes_h = synth.umi_codes(n, L)
    col = Column(codes_h)
    ops = {"directional_ids": col.directional_ids, "directional_correct": col.directional_correct,
           "transitive_ids": col.transitive_ids, "transitive_correct": col.transitive_correct,
           "c2_cluster": col.c2_cluster}
    if a.ops:
        ops = {name: ops[name] for name in a.ops.split(",")}
    ms = {name: [] for name in ops}
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
        col.directional_ids()
        stream.synchronize()
        k_dir = int(col.nk.value)
        rounds = ctypes.c_int64(0)
        _lib.call("rogtk_directional_last_rounds", ctypes.byref(rounds))
        col.transitive_ids()
        stream.synchronize()
        k_tra = int(col.nk.value)

    result = {"kind": "bench_directional", "device": torch.cuda.get_device_name(0), "rows": n, "umi_len": L,
              "steps": a.steps, "warmup": a.warmup, "n_distinct_codes": int(len(np.unique(codes_h))),
              "n_clusters": {"directional": k_dir, "transitive": k_tra}, "relaxation_rounds": int(rounds.value),
              "ops": {}}
    for name, v in ms.items():
        med = float(np.median(v))
        result["ops"][name] = {"kind": "gpu-events", "ms_median": med, "ms_min": float(min(v)),
                               "ms_max": float(max(v)), "rows_per_s": n / (med * 1e-3)}
    if a.ops or not a.sample:  # a profiler run: the timings of the chosen operations alone
        print(json.dumps(result))
        return 0
    med = {name: result["ops"][name]["ms_median"] for name in ops}
    yard = med["transitive_correct"] - med["transitive_ids"]
    result["yardstick"] = {"what": "transitive summary + gather = transitive_correct - transitive_ids", "ms": yard}
    result["ratios"] = {"directional_ids_over_yardstick": med["directional_ids"] / yard,
                        "directional_correct_over_yardstick": med["directional_correct"] / yard,
                        "directional_correct_over_transitive_correct":
                            med["directional_correct"] / med["transitive_correct"],
                        "directional_ids_over_c2_cluster": med["directional_ids"] / med["c2_cluster"]}

    # one core of numpy + Python on a sample, and the GPU's answers for the same rows
    m = min(a.sample, n)
    sm = Column(codes_h[:m])
    with torch.cuda.stream(stream):
        sm.directional_ids(root=True)
        stream.synchronize()
    g_ids = sm.cid.cpu().numpy().view(np.uint32)
    g_root = sm.root.cpu().numpy().view(np.uint64)
    g_k = int(sm.nk.value)
    t0 = time.perf_counter()
    r_root, r_ids, r_k, r_rounds = python_reference(codes_h[:m].astype(np.uint64), L)
    t1 = time.perf_counter()
    result["python"] = {"kind": "python", "rows": m, "cores": 1, "seconds": t1 - t0, "rows_per_s": m / (t1 - t0),
                        "n_clusters": r_k, "sweeps": r_rounds}
    result["checked_rows"] = m
    result["mismatches"] = {"cluster_id": int(np.count_nonzero(g_ids != r_ids)),
                            "root_code": int(np.count_nonzero(g_root != r_root)), "n_clusters": int(g_k != r_k)}
    result["speedup_vs_python"] = result["ops"]["directional_ids"]["rows_per_s"] / result["python"]["rows_per_s"]
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if not any(result["mismatches"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
