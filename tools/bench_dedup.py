#!/usr/bin/env python
"""Throughput of UMI deduplication on the device (rogtk_amd/csrc/dedup.hip).

Workload: N rows (default 10 M) resident in HBM, scores uniform in 0..60, and three id columns:

  c2_clusters  the ids of the C2 cluster step on synth-v1 UMIs of length 12 (max_distance 1:
               one giant cluster and many small ones, rows in random order)
  one_cluster  every row in cluster 0
  own_cluster  row i in cluster i

Per id column, timed with device events on one stream after a warm-up, median of the timed
steps, the operations alternating:

  select            votes and row counts (the tables' memsets included)
  select_no_combine the same without the LDS combine: one global atomic pair per row
  keep              the keep words, the tile popcounts and the decode of the tables
  compact           scan of the tile popcounts + scatter of the kept rows
  all               one full rogtk_cluster_best_rows call

Per operation: ms and rows/s; for `all` also the algorithmic bytes (8 B/row in, n/8 + 8 n_kept +
16 n_clusters out) as a rate and as a fraction of the 6.29 TB/s measured copy ceiling. The full
call's answers with and without the combine are compared; numpy's lexsort on one core is timed
on the same data (kind: numpy), and the GPU's answers for the first 200 k rows are checked
against it.

    python tools/bench_dedup.py [--rows 10000000] [--steps 10] [--warmup 3] [--out FILE]

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
COPY_CEILING = 6.29e12  # B/s, measured float4 copy
NO_ID = 0xFFFFFFFF


def numpy_reference(ids: np.ndarray, score: np.ndarray, k: int):
    """The spec by one lexsort on (id, -score, row): best_row, best_score, n_reads, kept rows."""
    i = ids.astype(np.int64)
    rows = np.arange(i.size, dtype=np.int64)
    live = i < k
    i, s, r = i[live], score.astype(np.int64)[live], rows[live]
    order = np.lexsort((r, -s, i))
    i, s, r = i[order], s[order], r[order]
    head = np.ones(i.size, dtype=bool)
    head[1:] = i[1:] != i[:-1]
    best_row = np.full(k, -1, dtype=np.int64)
    best_score = np.zeros(k, dtype=np.uint32)
    best_row[i[head]] = r[head]
    best_score[i[head]] = s[head].astype(np.uint32)
    n_reads = np.bincount(i, minlength=k).astype(np.uint32)
    return best_row, best_score, n_reads, np.sort(r[head])


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample", type=int, default=200_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("bench_dedup needs a GPU (there is no CPU path to time)", file=sys.stderr)
        return 2
    from rogtk_amd import _lib, dedup, synth
    from rogtk_amd import device as D

    n, L = a.rows, UMI_LEN
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    s = ctypes.c_void_p(stream.cuda_stream)
    p = lambda t: None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())

    def c2_ids():
        codes = torch.from_numpy(synth.umi_codes(n, L).view(np.int32).copy()).to(dev)
        cid = torch.empty(n, dtype=torch.int32, device=dev)
        eng = D.ClusterEngine(L, min(n, 4 ** L), dev)
        D.cluster_batch(eng, D.PackedBatch(codes, L), cid, 1)
        k = int(eng.stats()["n_clusters"])
        torch.cuda.synchronize()
        return cid.cpu().numpy().view(np.uint32).copy(), k

    class Run:
        def __init__(self, ids_h, score_h, k):
            self.n, self.k = ids_h.size, k
            self.ids = torch.from_numpy(ids_h.view(np.int32)).to(dev)
            self.score = torch.from_numpy(score_h.view(np.int32)).to(dev)
            tb = ctypes.c_int64(0)
            _lib.call("rogtk_cluster_best_temp_bytes", self.n, k, ctypes.byref(tb))
            self.tb = tb.value
            self.temp = torch.empty(self.tb, dtype=torch.uint8, device=dev)
            self.best_row = torch.empty(k, dtype=torch.int64, device=dev)
            self.best_score = torch.empty(k, dtype=torch.int32, device=dev)
            self.n_reads = torch.empty(k, dtype=torch.int32, device=dev)
            self.keep = torch.empty((self.n + 63) // 64, dtype=torch.int64, device=dev)
            self.kept = torch.empty(min(self.n, k), dtype=torch.int64, device=dev)
            self.n_kept = torch.zeros(1, dtype=torch.int64, device=dev)

        def call(self, combine=1, phases=7):
            _lib.call("rogtk_cluster_best_set_knobs", combine, phases)
            try:
                _lib.call("rogtk_cluster_best_rows", p(self.ids), p(self.score), self.n, self.k, p(self.best_row),
                          p(self.best_score), p(self.n_reads), p(self.keep), p(self.kept), p(self.n_kept),
                          p(self.temp), self.tb, s)
            finally:
                _lib.call("rogtk_cluster_best_set_knobs", 1, 7)

        def answers(self):
            stream.synchronize()
            m = int(self.n_kept.item())
            return (self.best_row.cpu().numpy(), self.best_score.cpu().numpy().view(np.uint32),
                    self.n_reads.cpu().numpy().view(np.uint32), self.kept[:m].cpu().numpy(),
                    self.keep.cpu().numpy().view(np.uint64))

    rng = np.random.default_rng(0)
    score_h = rng.integers(0, 61, size=n).astype(np.uint32)
    c2, c2_k = c2_ids()
    columns = {"c2_clusters": (c2, c2_k), "one_cluster": (np.zeros(n, np.uint32), 1),
               "own_cluster": (np.arange(n, dtype=np.uint32), n)}
    ops = {"select": (1, 1), "select_no_combine": (0, 1), "keep": (1, 2), "compact": (1, 4), "all": (1, 7)}

    result = {"kind": "bench_dedup", "device": torch.cuda.get_device_name(0), "rows": n, "steps": a.steps,
              "warmup": a.warmup, "score_range": [0, 60], "copy_ceiling_GBps": COPY_CEILING / 1e9,
              "geometry": dedup.geometry(), "columns": {}}
    bad_total = 0
    for name, (ids_h, k) in columns.items():
        run = Run(ids_h, score_h, k)
        ms = {op: [] for op in ops}
        with torch.cuda.stream(stream):
            for _ in range(a.warmup):
                run.call()
                for knobs in ops.values():
                    run.call(*knobs)
            stream.synchronize()
            for _ in range(a.steps):  # the operations alternate, so drift hits them alike
                for op, knobs in ops.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    run.call(*knobs)
                    e1.record(stream)
                    e1.synchronize()
                    ms[op].append(e0.elapsed_time(e1))
            run.call(0, 7)
            plain = run.answers()
            run.call(1, 7)
            combined = run.answers()
        n_kept = int(combined[3].size)
        nbytes = 8 * n + n // 8 + 8 * n_kept + 16 * k
        col = {"n_clusters": k, "n_kept": n_kept, "largest_cluster": int(combined[2].max()), "temp_bytes": run.tb,
               "algorithmic_bytes": nbytes, "ops": {}}
        for op, v in ms.items():
            med = float(np.median(v))
            col["ops"][op] = {"kind": "gpu-events", "ms_median": med, "ms_min": float(min(v)), "ms_max": float(max(v)),
                              "rows_per_s": n / (med * 1e-3)}
        med = col["ops"]["all"]["ms_median"]
        col["ops"]["all"]["algorithmic_GBps"] = nbytes / (med * 1e-3) / 1e9
        col["ops"]["all"]["fraction_of_copy_ceiling"] = nbytes / (med * 1e-3) / COPY_CEILING
        col["no_combine_over_combine"] = (col["ops"]["select_no_combine"]["ms_median"]
                                          / col["ops"]["select"]["ms_median"])
        combine_bad = int(sum(np.count_nonzero(x != y) if x.shape == y.shape else max(x.size, y.size)
                              for x, y in zip(plain, combined)))

        # numpy on one core on the same data
        t0 = time.perf_counter()
        r_full = numpy_reference(ids_h, score_h, k)
        t1 = time.perf_counter()
        col["numpy"] = {"kind": "numpy", "rows": n, "cores": 1, "seconds": t1 - t0, "rows_per_s": n / (t1 - t0)}
        col["speedup_vs_numpy"] = col["ops"]["all"]["rows_per_s"] / col["numpy"]["rows_per_s"]
        full_bad = int(sum(np.count_nonzero(x != y) if x.shape == y.shape else max(x.size, y.size)
                           for x, y in zip(r_full, combined[:4])))
        # ... and the GPU's answers for the first rows against it
        m = min(a.sample, n)
        ks = min(k, int(ids_h[:m].max()) + 1)
        sm = Run(ids_h[:m].copy(), score_h[:m].copy(), ks)
        with torch.cuda.stream(stream):
            sm.call()
            g = sm.answers()
        r = numpy_reference(ids_h[:m], score_h[:m], ks)
        keep = np.zeros((m + 63) // 64 * 64, dtype=np.uint8)
        keep[r[3]] = 1
        words = np.packbits(keep, bitorder="little").view("<u8")
        col["checked_rows"] = m
        col["mismatches"] = {"best_row": int(np.count_nonzero(g[0] != r[0])),
                             "best_score": int(np.count_nonzero(g[1] != r[1])),
                             "n_reads": int(np.count_nonzero(g[2] != r[2])),
                             "kept_rows": int(np.count_nonzero(g[3] != r[3])) if g[3].shape == r[3].shape else m,
                             "keep_words": int(np.count_nonzero(g[4] != words)),
                             "combine_vs_no_combine_full": combine_bad, "numpy_full": full_bad}
        bad_total += sum(col["mismatches"].values())
        result["columns"][name] = col
        del run, sm
        torch.cuda.empty_cache()

    worst = max(result["columns"], key=lambda c: result["columns"][c]["ops"]["all"]["ms_median"])
    result["worst_column"] = worst
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if bad_total == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
