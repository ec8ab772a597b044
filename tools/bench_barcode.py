#!/usr/bin/env python
"""Throughput of cell-barcode correction against a whitelist (rogtk_amd/csrc/barcode.hip,
DESIGN.md §4e).

Workload: N barcodes of length 16 (default 10 M) resident in HBM as a string column (int64
offsets, values), synthesised with a fixed seed: 95 % drawn from about 5,000 "cells" of the
whitelist with a skewed (log-normal) size distribution, 4 % a cell's barcode with one
substitution, 0.5 % with one N, 0.5 % random. Whitelists of W = 737,280 and W = 6,794,880
random distinct codes. Timed with device events on one stream after a warm-up, median of the
timed steps, the operations alternating in this one process and build:

  correct_counts / correct_reject   rogtk_barcode_correct_dev in both modes
  count                             rogtk_barcode_count_dev: the exact pass alone
  correct_counts_wave               a wave per miss instead of a lane per miss (the default)
  correct_counts_plain, count_plain lookups by a binary search over the whole sorted whitelist
                                    instead of the prefix table
  sort_distinct                     the cheapest call that does comparable row work on the same
                                    column: rogtk_umi_cluster_grouped_dev, directional,
                                    max_distance 0, every key 0: pack + sort + distinct

Every variant's outputs are compared with the default's (they must be identical), and the
default's outputs on a 200 k-row sample with restatement (a) of tests/barcode_spec.py on one
core (a dict of the whitelist's strings), at the smaller W.

Not measured here: other L, the host entries' transfer share, the plugin's per-call handle
build, u32 codes (the library packs to u64 at every L).

    python tools/bench_barcode.py [--rows 10000000] [--steps 10] [--warmup 3] [--out FILE]
    rocprofv3 --kernel-trace --stats ... -- python tools/bench_barcode.py --ops correct_counts_w6794880

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
for path in (ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

L = 16
WHITELISTS = (737_280, 6_794_880)
CELLS = 5_000
PROBES = {"wave": 0, "lane": 1, "lane_plain": 3}
DEFAULT_PROBE = "lane"
COPY_CEILING = 6.29e12  # B/s, the README's copy ceiling


def to_ascii(codes: np.ndarray) -> np.ndarray:
    shifts = np.arange(L - 1, -1, -1, dtype=np.uint64) * np.uint64(2)
    return np.frombuffer(b"ACGT", dtype=np.uint8)[(codes.astype(np.uint64)[:, None] >> shifts[None, :]) & np.uint64(3)]


def synthesise(n: int, W: int, seed: int = 2024):
    """(whitelist codes [W], row bytes (n, L)); the kinds are interleaved at random."""
    rng = np.random.default_rng(seed + W)
    wl = np.unique(rng.integers(0, 1 << 32, size=int(W * 1.02) + 1000, dtype=np.uint64))
    wl = rng.permutation(wl)[:W]
    assert len(wl) == W
    cells = wl[rng.choice(W, size=CELLS, replace=False)]
    weight = rng.lognormal(0.0, 1.5, size=CELLS)
    codes = cells[rng.choice(CELLS, size=n, p=weight / weight.sum())]
    kind = rng.random(n)
    sub = kind < 0.04
    pos = rng.integers(0, L, size=n).astype(np.uint64)
    flip = rng.integers(1, 4, size=n).astype(np.uint64) << (np.uint64(2) * pos)
    codes = np.where(sub, codes ^ flip, codes)
    rnd = (kind >= 0.045) & (kind < 0.05)
    codes = np.where(rnd, rng.integers(0, 1 << 32, size=n, dtype=np.uint64), codes)
    rows = to_ascii(codes)
    with_n = np.flatnonzero((kind >= 0.04) & (kind < 0.045))
    rows[with_n, (L - 1 - pos[with_n]).astype(np.int64)] = ord("N")
    return wl, rows


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
        print("bench_barcode needs a GPU (there is no CPU path to time)", file=sys.stderr)
        return 2
    import rogtk_amd as rg
    from rogtk_amd import _lib

    n = a.rows
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    s = ctypes.c_void_p(stream.cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    class Case:
        def __init__(self, W):
            self.W = W
            self.wl_codes, self.rows_h = synthesise(n, W)
            t0 = time.perf_counter()
            self.wl = rg.BarcodeWhitelist(to_ascii(self.wl_codes).view(f"S{L}").reshape(-1))
            self.create_s = time.perf_counter() - t0  # Python checks + pack + upload + sort + table
            self.off = (torch.arange(n + 1, dtype=torch.int64, device=dev) * L).contiguous()
            self.val = torch.from_numpy(self.rows_h.reshape(-1)).to(dev)
            self.index = torch.empty(n, dtype=torch.int32, device=dev)
            self.status = torch.empty(n, dtype=torch.uint8, device=dev)
            self.exact = torch.empty(W, dtype=torch.int32, device=dev)
            self.counts = torch.empty(W, dtype=torch.int32, device=dev)
            self.zero_keys = torch.zeros(n, dtype=torch.int32, device=dev)
            self.cid = torch.empty(n, dtype=torch.int32, device=dev)
            self.totals = (ctypes.c_int64 * 5)()
            self.nk = ctypes.c_int64(0)

        def correct(self, ambiguous=0, probe=DEFAULT_PROBE):
            _lib.call("rogtk_barcode_set_probe", PROBES[probe])
            try:
                _lib.call("rogtk_barcode_correct_dev", self.wl.handle, p(self.off), p(self.val), None, n, ambiguous,
                          None, p(self.index), p(self.status), p(self.exact), p(self.counts), self.totals, s)
            finally:
                _lib.call("rogtk_barcode_set_probe", PROBES[DEFAULT_PROBE])

        def count(self, probe=DEFAULT_PROBE):
            _lib.call("rogtk_barcode_set_probe", PROBES[probe])
            try:
                _lib.call("rogtk_barcode_count_dev", self.wl.handle, p(self.off), p(self.val), None, n, p(self.exact),
                          self.totals, s)
            finally:
                _lib.call("rogtk_barcode_set_probe", PROBES[DEFAULT_PROBE])

        def sort_distinct(self):
            _lib.call("rogtk_umi_cluster_grouped_dev", p(self.off), p(self.val), None, n, p(self.zero_keys), L, 1, 0,
                      p(self.cid), ctypes.byref(self.nk), None, None, s)

        def outputs(self):
            stream.synchronize()
            return (self.index.cpu().numpy().copy(), self.status.cpu().numpy().copy(),
                    self.exact.cpu().numpy().copy(), self.counts.cpu().numpy().copy(), list(self.totals))

    cases = {W: Case(W) for W in WHITELISTS}
    ops = {}
    for W, c in cases.items():
        t = f"_w{W}"
        ops["correct_counts" + t] = lambda c=c: c.correct(0)
        ops["correct_reject" + t] = lambda c=c: c.correct(1)
        ops["count" + t] = lambda c=c: c.count()
        ops["correct_counts_wave" + t] = lambda c=c: c.correct(0, "wave")
        ops["correct_counts_plain" + t] = lambda c=c: c.correct(0, "lane_plain")
        ops["count_plain" + t] = lambda c=c: c.count("lane_plain")
        ops["sort_distinct" + t] = lambda c=c: c.sort_distinct()
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

    result = {"kind": "bench_barcode", "device": torch.cuda.get_device_name(0), "rows": n, "barcode_len": L,
              "steps": a.steps, "warmup": a.warmup, "cells": CELLS, "default_probe": DEFAULT_PROBE, "code_type": "u64",
              "whitelists": {str(W): dict(c.wl.info(), create_seconds=c.create_s) for W, c in cases.items()},
              "ops": {}}
    for name, v in ms.items():
        med = float(np.median(v))
        result["ops"][name] = {"kind": "gpu-events", "ms_median": med, "ms_min": float(min(v)),
                               "ms_max": float(max(v)), "rows_per_s": n / (med * 1e-3)}
    if a.ops or not a.sample:  # a profiler run: the timings of the chosen operations alone
        print(json.dumps(result))
        return 0
    med = {name: result["ops"][name]["ms_median"] for name in ops}
    result["ratios"], result["totals"], result["variant_mismatches"], result["exact_pass"] = {}, {}, {}, {}
    with torch.cuda.stream(stream):
        for W, c in cases.items():
            t = f"_w{W}"
            for name in ("correct_counts", "correct_reject", "count"):
                result["ratios"][name + t + "_over_sort_distinct"] = med[name + t] / med["sort_distinct" + t]
            result["ratios"]["wave_over_lane" + t] = med["correct_counts_wave" + t] / med["correct_counts" + t]
            result["ratios"]["plain_over_prefix_correct" + t] = med["correct_counts_plain" + t] / med["correct_counts" + t]
            result["ratios"]["plain_over_prefix_count" + t] = med["count_plain" + t] / med["count" + t]
            read = n * (8 + L)  # the row's int64 offset and its bytes
            result["exact_pass"][str(W)] = {"bytes_read": read, "bytes_per_s": read / (med["count" + t] * 1e-3),
                                            "fraction_of_copy_ceiling": read / (med["count" + t] * 1e-3) / COPY_CEILING}
            c.correct(0)
            base = c.outputs()
            result["totals"][str(W)] = dict(zip(("exact", "corrected", "ambiguous", "no_match", "null"), base[4]))
            bad = {}
            for probe in ("wave", "lane_plain"):
                c.correct(0, probe)
                got = c.outputs()
                bad[probe] = int(sum(np.count_nonzero(x != y) for x, y in zip(got[:4], base[:4])) + (got[4] != base[4]))
            result["variant_mismatches"][str(W)] = bad

    # restatement (a) on one core over a sample, and the GPU's answers for the same rows
    import barcode_spec as B

    W = WHITELISTS[0]
    c = cases[W]
    m = min(a.sample, n)
    sample = [bytes(r) for r in c.rows_h[:m]]
    wl_strings = [bytes(r) for r in to_ascii(c.wl_codes)]
    result["python"], result["mismatches"] = {}, {}
    for mode in ("counts", "reject"):
        t0 = time.perf_counter()
        want = B.correct_dict(sample, wl_strings, mode)
        t1 = time.perf_counter()
        got = c.wl.correct(np.asarray(sample, dtype=f"S{L}"), mode)
        result["python"][mode] = {"kind": "python", "rows": m, "cores": 1, "W": W, "seconds": t1 - t0,
                                  "rows_per_s": m / (t1 - t0)}
        result["mismatches"][mode] = {
            "index": int(np.count_nonzero(got.keys != np.asarray(want.index, dtype=np.uint32))),
            "status": int(np.count_nonzero(got.status != np.asarray(want.status, dtype=np.uint8))),
            "corrected": int(sum(x != y for x, y in zip(got.corrected.to_pylist(), want.corrected))),
            "exact_counts": int(np.count_nonzero(got.exact_counts != np.asarray(want.exact_counts, dtype=np.uint32))),
            "counts": int(np.count_nonzero(got.counts != np.asarray(want.counts, dtype=np.uint32))),
            "totals": int(list(got.totals.values()) != want.totals)}
    result["checked_rows"] = m
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    bad = any(v for mm in result["mismatches"].values() for v in mm.values()) or \
        any(v for mm in result["variant_mismatches"].values() for v in mm.values())
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
