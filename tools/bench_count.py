#!/usr/bin/env python
"""Throughput of the UMI count matrix on the device (rogtk_amd/csrc/count_matrix.hip).

Workload: N rows (default 10 M) resident in HBM, three cases:

  c2_clusters  molecule = the ids of the C2 cluster step on synth-v1 UMIs of length 12
               (max_distance 1), cell = one of 5,000 cells with a log-normal size distribution out
               of a 737,280-row whitelist (as tools/bench_barcode.py draws them), feature uniform
               in 0..32,767
  own_entry    every row its own (cell, feature) pair, rows shuffled
  one_triple   every row the same (cell, feature, molecule)

Per case, timed with device events on one stream after a warm-up, median of the timed steps, the
operations alternating:

  pack   the keys
  sort   the hipcub radix sort
  rest   flags + scan + emit + diff + indptr
  all    one full rogtk_count_matrix call

Per operation: ms and rows/s; for `all` also the algorithmic bytes (12 B/row in, 16 B per entry
and 8 B per cell of indptr out) as a rate and as a fraction of the 6.29 TB/s measured copy
ceiling, and the sort's share of the call. numpy (np.unique over the packed key, one core) is timed
on the same rows (kind: numpy) and every output of the GPU is compared with it.

    python tools/bench_count.py [--rows 10000000] [--steps 10] [--warmup 3] [--out FILE]

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
WHITELIST = 737_280
CELLS = 5_000
FEATURES = 32_768


def bit_width(v: int) -> int:
    return int(v).bit_length() if v > 0 else 0


def numpy_reference(c, f, m, sizes):
    """The spec by np.unique over the packed key: entry_cell, entry_feature, n_umis, n_reads, indptr, totals."""
    nc, nf, nm = sizes
    fb, mb = bit_width(nf - 1), bit_width(nm - 1)
    live = (c < nc) & (f < nf) & (m < nm)
    key = (c[live].astype(np.uint64) << np.uint64(fb + mb)) | (f[live].astype(np.uint64) << np.uint64(mb)) \
        | m[live].astype(np.uint64)
    uk, cnt = np.unique(key, return_counts=True)
    pair = uk >> np.uint64(mb)
    head = np.ones(uk.size, dtype=bool)
    head[1:] = pair[1:] != pair[:-1]
    start = np.flatnonzero(head)
    n_umis = np.diff(np.append(start, uk.size)).astype(np.uint32)
    n_reads = np.add.reduceat(cnt, start).astype(np.uint32) if start.size else np.zeros(0, np.uint32)
    ec = (pair[head] >> np.uint64(fb)).astype(np.uint32)
    ef = (pair[head] & np.uint64((1 << fb) - 1)).astype(np.uint32)
    indptr = np.searchsorted(ec, np.arange(nc + 1), side="left").astype(np.int64)
    return ec, ef, n_umis, n_reads, indptr, np.array([start.size, int(live.sum()), uk.size], dtype=np.int64)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("bench_count needs a GPU (there is no CPU path to time)", file=sys.stderr)
        return 2
    from rogtk_amd import _lib, count, synth
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
        def __init__(self, cols, sizes):
            self.n, self.sizes = cols[0].size, sizes
            self.cols = [torch.from_numpy(x.view(np.int32)).to(dev) for x in cols]
            self.cap = min(self.n, sizes[0] * sizes[1])
            tb = ctypes.c_int64(0)
            _lib.call("rogtk_count_matrix_temp_bytes", self.n, *sizes, self.cap, ctypes.byref(tb))
            self.tb = tb.value
            self.temp = torch.empty(self.tb, dtype=torch.uint8, device=dev)
            self.out = [torch.empty(self.cap, dtype=torch.int32, device=dev) for _ in range(4)]
            self.indptr = torch.empty(sizes[0] + 1, dtype=torch.int64, device=dev)
            self.totals = torch.zeros(3, dtype=torch.int64, device=dev)

        def call(self, phases=7):
            _lib.call("rogtk_count_matrix_set_phases", phases)
            try:
                _lib.call("rogtk_count_matrix", *(p(t) for t in self.cols), self.n, *self.sizes,
                          *(p(t) for t in self.out), self.cap, p(self.indptr), p(self.totals), p(self.temp), self.tb, s)
            finally:
                _lib.call("rogtk_count_matrix_set_phases", 7)

        def answers(self):
            stream.synchronize()
            tot = self.totals.cpu().numpy()
            w = min(int(tot[0]), self.cap)
            return [t[:w].cpu().numpy().view(np.uint32) for t in self.out] + [self.indptr.cpu().numpy(), tot]

    rng = np.random.default_rng(0)
    c2, c2_k = c2_ids()
    weight = rng.lognormal(0.0, 1.5, size=CELLS)
    cells = rng.choice(WHITELIST, size=CELLS, replace=False).astype(np.uint32)
    shuffled = rng.permutation(n)
    cases = {
        "c2_clusters": ([cells[rng.choice(CELLS, size=n, p=weight / weight.sum())],
                         rng.integers(0, FEATURES, size=n).astype(np.uint32), c2], (WHITELIST, FEATURES, c2_k)),
        "own_entry": ([(shuffled // FEATURES).astype(np.uint32), (shuffled % FEATURES).astype(np.uint32),
                       (shuffled % 1000).astype(np.uint32)], ((n + FEATURES - 1) // FEATURES, FEATURES, 1000)),
        "one_triple": ([np.full(n, 3, np.uint32), np.full(n, 5, np.uint32), np.full(n, 7, np.uint32)], (8, 8, 8)),
    }
    ops = {"pack": 1, "sort": 2, "rest": 4, "all": 7}

    result = {"kind": "bench_count", "device": torch.cuda.get_device_name(0), "rows": n, "steps": a.steps,
              "warmup": a.warmup, "copy_ceiling_GBps": COPY_CEILING / 1e9, "geometry": count.geometry(), "cases": {}}
    bad_total = 0
    for name, (cols, sizes) in cases.items():
        run = Run(cols, sizes)
        ms = {op: [] for op in ops}
        with torch.cuda.stream(stream):
            for _ in range(a.warmup):
                for ph in ops.values():
                    run.call(ph)
            run.call()
            stream.synchronize()
            for _ in range(a.steps):  # the operations alternate, so drift hits them alike
                for op, ph in ops.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    run.call(ph)
                    e1.record(stream)
                    e1.synchronize()
                    ms[op].append(e0.elapsed_time(e1))
            run.call()
            got = run.answers()
        entries = int(got[5][0])
        nbytes = 12 * n + 16 * entries + 8 * (sizes[0] + 1) + 24
        bits = bit_width(sizes[0]) + bit_width(sizes[1] - 1) + bit_width(sizes[2] - 1)
        case = {"sizes": list(sizes), "key_bits": bits, "entries": entries, "live_rows": int(got[5][1]),
                "molecules": int(got[5][2]), "temp_bytes": run.tb, "algorithmic_bytes": nbytes, "ops": {}}
        for op, v in ms.items():
            med = float(np.median(v))
            case["ops"][op] = {"kind": "gpu-events", "ms_median": med, "ms_min": float(min(v)), "ms_max": float(max(v)),
                               "rows_per_s": n / (med * 1e-3)}
        med = case["ops"]["all"]["ms_median"]
        case["ops"]["all"]["algorithmic_GBps"] = nbytes / (med * 1e-3) / 1e9
        case["ops"]["all"]["fraction_of_copy_ceiling"] = nbytes / (med * 1e-3) / COPY_CEILING
        case["sort_share_of_all"] = case["ops"]["sort"]["ms_median"] / med
        case["non_sort_over_sort"] = ((case["ops"]["pack"]["ms_median"] + case["ops"]["rest"]["ms_median"])
                                      / case["ops"]["sort"]["ms_median"])

        t0 = time.perf_counter()
        ref = numpy_reference(*cols, sizes)
        t1 = time.perf_counter()
        case["numpy"] = {"kind": "numpy", "rows": n, "cores": 1, "seconds": t1 - t0, "rows_per_s": n / (t1 - t0)}
        case["speedup_vs_numpy"] = case["ops"]["all"]["rows_per_s"] / case["numpy"]["rows_per_s"]
        names = ("entry_cell", "entry_feature", "n_umis", "n_reads", "indptr", "totals")
        case["mismatches"] = {k: int(np.count_nonzero(x != y)) if x.shape == y.shape else int(max(x.size, y.size))
                              for k, x, y in zip(names, got, ref)}
        bad_total += sum(case["mismatches"].values())
        result["cases"][name] = case
        del run
        torch.cuda.empty_cache()

    result["mismatches_total"] = bad_total
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if bad_total == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
