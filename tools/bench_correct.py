#!/usr/bin/env python
"""Throughput of the packed UMI-correction step (rogtk_amd/csrc/correct.hip).

Workload: the C2 shape, N synth-v1 UMIs of length 12 (default 10 M) resident in HBM as the
packed SoA, cluster ids from the cluster engine (max_distance 1). Timed with device events on
one stream after a warm-up, median of the timed steps:

  summary        rogtk_cluster_summary_packed, the kept counting design (radix sort + runs)
  summary_table  the same with the count-table design (one scattered atomic per row)
  summary_regular_bits  the kept design with a regular-bits mask (adds the pass that packs
                 the regular rows to the front; all bits set here)
  correct        rogtk_cluster_correct_packed
  both           summary + correct

The two counting designs are timed alternately in the same process. Per operation: ms, rows/s,
the algorithmic 12 B/row (8 in, 4 out) as a rate and as a fraction of the 6.29 TB/s measured
copy ceiling, and the ratio to the C2 step's ms_per_step of the same build (--c2-ms, or
--c2-json with a bench.py result line). A 1-core numpy / Counter rate on a 200 k-row sample
(kind: python) is printed next to them; the GPU's tables and corrected codes for that sample
are checked against it, and the two designs' tables for the full column against each other.

    python tools/bench_correct.py [--rows 10000000] [--steps 10] [--warmup 3] [--out FILE]

Prints one JSON line; --out also writes it to a file.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

UMI_LEN = 12
COPY_CEILING = 6.29e12  # B/s, measured float4 copy
BYTES_PER_ROW = 12      # codes + ids in, corrected codes out


def python_reference(codes: np.ndarray, ids: np.ndarray, k: int):
    """The spec on one core: Counter per distinct code, the vote per cluster, the gather."""
    cnt = Counter(zip(ids.tolist(), codes.tolist()))
    best = {}
    n_reads = np.zeros(k, np.uint32)
    n_distinct = np.zeros(k, np.uint32)
    for (c, code), m in cnt.items():
        n_reads[c] += m
        n_distinct[c] += 1
        key = (-m, code)
        if c not in best or key < best[c]:
            best[c] = key
    rep = np.full(k, 0xFFFFFFFF, np.uint32)
    for c, (_, code) in best.items():
        rep[c] = code
    return rep, n_reads, n_distinct, rep[ids]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample", type=int, default=200_000)
    ap.add_argument("--c2-ms", type=float, default=None, help="ms_per_step of bench.py's C2 step, same build")
    ap.add_argument("--c2-json", default=None, help="file holding bench.py's JSON result line")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    c2_ms = a.c2_ms
    if c2_ms is None and a.c2_json:
        with open(a.c2_json) as f:
            for ln in f:
                ln = ln.strip()
                if ln.startswith("{") and "ms_per_step" in ln:
                    c2_ms = float(json.loads(ln)["ms_per_step"])

    import torch

    if not torch.cuda.is_available():
        print("bench_correct needs a GPU (there is no CPU path to time)", file=sys.stderr)
        return 2
    from rogtk_amd import _lib, synth
    from rogtk_amd import device as D

    n, L = a.rows, UMI_LEN
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    s = ctypes.c_void_p(stream.cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def cluster(codes_h):
        m = len(codes_h)
        codes = torch.from_numpy(codes_h.view(np.int32).copy()).to(dev)
        cid = torch.empty(m, dtype=torch.int32, device=dev)
        eng = D.ClusterEngine(L, min(m, 4 ** L), dev)
        D.cluster_batch(eng, D.PackedBatch(codes, L), cid, 1)
        k = int(eng.stats()["n_clusters"])
        torch.cuda.synchronize()
        return codes, cid, k

    class Run:
        def __init__(self, codes, cid, k):
            self.codes, self.cid, self.k, self.n = codes, cid, k, codes.numel()
            tb = ctypes.c_int64(0)
            _lib.call("rogtk_cluster_summary_temp_bytes", self.n, L, k, ctypes.byref(tb))
            self.tb = tb.value
            self.temp = torch.empty(self.tb, dtype=torch.uint8, device=dev)
            self.rep = torch.empty(k, dtype=torch.int32, device=dev)
            self.n_reads = torch.empty(k, dtype=torch.int32, device=dev)
            self.n_distinct = torch.empty(k, dtype=torch.int32, device=dev)
            self.out = torch.empty(self.n, dtype=torch.int32, device=dev)
            self.bits = torch.full(((self.n + 63) // 64,), -1, dtype=torch.int64, device=dev)

        def summary(self, method=0, bits=False):
            _lib.call("rogtk_cluster_summary_set_method", method)
            _lib.call("rogtk_cluster_summary_packed", p(self.codes), p(self.bits) if bits else None, self.n, L,
                      p(self.cid), self.k,
                      p(self.rep), p(self.n_reads), p(self.n_distinct), p(self.temp), self.tb, s)
            _lib.call("rogtk_cluster_summary_set_method", 0)

        def correct(self):
            _lib.call("rogtk_cluster_correct_packed", p(self.cid), None, self.n, p(self.rep), self.k, p(self.out), s)

        def tables(self):
            stream.synchronize()
            return [t.cpu().numpy().view(np.uint32).copy() for t in (self.rep, self.n_reads, self.n_distinct)]

    codes_h = synth.umi_codes(n, L)
    run = Run(*cluster(codes_h))

    ops = {"summary": lambda: run.summary(0), "summary_table": lambda: run.summary(1),
           "summary_regular_bits": lambda: run.summary(0, True), "correct": run.correct,
           "both": lambda: (run.summary(0), run.correct())}
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

    result = {"kind": "bench_correct", "device": torch.cuda.get_device_name(0), "rows": n, "umi_len": L,
              "n_clusters": run.k, "steps": a.steps, "warmup": a.warmup, "bytes_per_row": BYTES_PER_ROW,
              "copy_ceiling_GBps": COPY_CEILING / 1e9, "temp_bytes": run.tb, "c2_ms_per_step": c2_ms, "ops": {}}
    for name, v in ms.items():
        med = float(np.median(v))
        rate = BYTES_PER_ROW * n / (med * 1e-3)
        result["ops"][name] = {"kind": "gpu-events", "ms_median": med, "ms_min": float(min(v)), "ms_max": float(max(v)),
                               "rows_per_s": n / (med * 1e-3), "algorithmic_GBps": rate / 1e9,
                               "fraction_of_copy_ceiling": rate / COPY_CEILING,
                               "ratio_to_c2_step": None if not c2_ms else med / c2_ms}
    result["kept_design"] = "sort"
    result["table_over_sort"] = result["ops"]["summary_table"]["ms_median"] / result["ops"]["summary"]["ms_median"]

    # the two designs agree on the full column
    with torch.cuda.stream(stream):
        run.summary(0)
        t_sort = run.tables()
        run.summary(1)
        t_tab = run.tables()
        run.summary(0)
    design_bad = int(sum(np.count_nonzero(x != y) for x, y in zip(t_sort, t_tab)))
    result["n_distinct_codes"] = int(t_sort[2].sum())

    # one core of Python on a sample, and the GPU's answers for the same rows
    m = min(a.sample, n)
    sm = Run(*cluster(codes_h[:m]))
    with torch.cuda.stream(stream):
        sm.summary(0)
        sm.correct()
    g_rep, g_reads, g_distinct = sm.tables()
    g_out = sm.out.cpu().numpy().view(np.uint32)
    ids_h = sm.cid.cpu().numpy().view(np.uint32)
    t0 = time.perf_counter()
    r_rep, r_reads, r_distinct, r_out = python_reference(codes_h[:m], ids_h, sm.k)
    t1 = time.perf_counter()
    result["python"] = {"kind": "python", "rows": m, "cores": 1, "rows_per_s": m / (t1 - t0)}
    result["checked_rows"] = m
    result["mismatches"] = {"rep_code": int(np.count_nonzero(g_rep != r_rep)),
                            "n_reads": int(np.count_nonzero(g_reads != r_reads)),
                            "n_distinct": int(np.count_nonzero(g_distinct != r_distinct)),
                            "corrected": int(np.count_nonzero(g_out != r_out)), "sort_vs_table_full": design_bad}
    result["speedup_vs_python"] = result["ops"]["both"]["rows_per_s"] / result["python"]["rows_per_s"]
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if not any(result["mismatches"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
