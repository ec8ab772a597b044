#!/usr/bin/env python
"""Throughput of the fuzzy namespace's kernels on device-resident columns.

Workload: N synthetic 150-byte reads (default 10 M); a 20-base target planted with one edit
(a substitution or a deletion) in every second read. The column (int64 offsets + values)
lives on the device; `match` (k_fuzzy_contains) and `replace_target` (k_fuzzy_replace_measure,
the offsets scan, k_fuzzy_replace_fill) are driven through the Level-1 entry points and timed
with device events after a warm-up. Reported per operation: rows/s, input GB/s (offsets +
values read once) and that rate's fraction of the 6.29 TB/s measured copy ceiling of the
MI355X. A 1-core Python `re` rate on a 200 k-row sample is printed next to them
(kind: python-re) and the GPU answers for that sample are checked against it.

    python tools/bench_fuzzy.py [--rows 10000000] [--steps 10] [--warmup 3] [--out FILE]

Prints one JSON line; --out also writes it to a file.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TARGET = "GATTACAGATTACACCGTGA"
REPLACEMENT = "NNNNNNNNNNNNNNNNNNNN"
READ_LEN = 150
COPY_CEILING = 6.29e12  # B/s, measured float4 copy


def make_reads(n: int, seed: int) -> np.ndarray:
    """(n, 150) ASCII reads; odd rows carry the target with one substitution or one deletion."""
    from rogtk_amd import synth

    raw = np.ascontiguousarray(synth.reads(n, READ_LEN, seed=seed))
    rng = np.random.default_rng(seed)
    t = np.frombuffer(TARGET.encode(), np.uint8)
    rows = np.arange(1, n, 2)
    m = len(rows)
    pos = rng.integers(0, READ_LEN - len(t) + 1, m)
    edit = rng.integers(0, len(t), m)
    patch = np.broadcast_to(t, (m, len(t))).copy()
    sub = rng.random(m) < 0.5
    # substitution: another base at `edit`; deletion: the tail moves up and the last byte keeps the read's own
    other = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, m)]
    other = np.where(other == t[edit], np.uint8(ord("N")), other)
    k = np.arange(len(t))
    shifted = np.where(k[None, :] >= edit[:, None], np.take(np.append(t, 0), k[None, :] + 1), patch)
    cols = pos[:, None] + k[None, :]
    keep = raw[rows[:, None], cols]
    shifted[:, -1] = keep[:, -1]
    patch[np.arange(m), edit] = other
    raw[rows[:, None], cols] = np.where(sub[:, None], patch, shifted)
    return raw


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample", type=int, default=200_000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("bench_fuzzy needs a GPU (there is no CPU path to time)", file=sys.stderr)
        return 2
    from rogtk_amd import _lib
    from rogtk_amd.strings import FuzzyProgram

    n = a.rows
    raw = make_reads(n, a.seed)
    dev = torch.device("cuda:0")
    vals = torch.from_numpy(raw.reshape(-1)).to(dev)
    offs = (torch.arange(n + 1, dtype=torch.int64, device=dev) * READ_LEN)
    col = _lib.StrCol(offs.data_ptr(), 8, vals.data_ptr(), vals.numel(), None, 0, n)
    words = (n + 63) // 64
    bits = torch.zeros(words, dtype=torch.int64, device=dev)
    vbits = torch.zeros(words, dtype=torch.int64, device=dev)
    tb = ctypes.c_int64(0)
    _lib.call("rogtk_str_temp_bytes", n, ctypes.byref(tb))
    temp = torch.zeros(tb.value, dtype=torch.uint8, device=dev)
    out_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    # every match is replaced by as many bytes as the target has: the output is no longer than the input + 1 B/row
    out = torch.zeros(vals.numel() + n, dtype=torch.uint8, device=dev)
    prog = FuzzyProgram.native(TARGET).set_replacement(REPLACEMENT)
    stream = torch.cuda.Stream(device=dev)
    s = ctypes.c_void_p(stream.cuda_stream)

    def contains():
        _lib.call("rogtk_fuzzy_contains", prog.handle, ctypes.byref(col), bits.data_ptr(), vbits.data_ptr(), s)

    def measure():
        _lib.call("rogtk_fuzzy_replace_measure", prog.handle, ctypes.byref(col), 0, out_off.data_ptr(),
                  vbits.data_ptr(), temp.data_ptr(), tb.value, s)

    def fill():
        _lib.call("rogtk_fuzzy_replace_fill", prog.handle, ctypes.byref(col), 0, out_off.data_ptr(),
                  out.data_ptr(), s)

    def replace():
        measure()
        fill()

    def timed(fn):
        with torch.cuda.stream(stream):
            for _ in range(a.warmup):
                fn()
            stream.synchronize()
            ms = []
            for _ in range(a.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
        return ms

    in_bytes = vals.numel() + (n + 1) * 8
    result = {"kind": "bench_fuzzy", "device": torch.cuda.get_device_name(0), "rows": n, "read_len": READ_LEN,
              "target": TARGET, "program": prog.describe().count("|") + 1, "steps": a.steps, "warmup": a.warmup,
              "input_bytes": in_bytes, "copy_ceiling_GBps": COPY_CEILING / 1e9, "ops": {}}
    for name, fn in (("contains", contains), ("replace_target", replace), ("replace_measure", measure),
                     ("replace_fill", fill)):
        ms = timed(fn)
        med = float(np.median(ms))
        result["ops"][name] = {
            "kind": "gpu-events", "ms_median": med, "ms_min": float(min(ms)), "ms_max": float(max(ms)),
            "rows_per_s": n / (med * 1e-3), "input_GBps": in_bytes / (med * 1e-3) / 1e9,
            "fraction_of_copy_ceiling": in_bytes / (med * 1e-3) / COPY_CEILING,
        }
    torch.cuda.synchronize()
    total_out = int(out_off[n].item())
    result["ops"]["replace_target"]["output_bytes"] = total_out

    # 1-core python re on a sample, and the GPU's answers for the same rows
    m = min(a.sample, n)
    rx = re.compile("|".join([TARGET] + [TARGET[:i] + ".{0,1}" + TARGET[i + 1:] for i in range(len(TARGET))]
                             + [TARGET[:-1] + "."]))
    strs = [bytes(r).decode() for r in raw[:m]]
    t0 = time.perf_counter()
    hits = [rx.search(x) is not None for x in strs]
    t1 = time.perf_counter()
    subs = [rx.sub(lambda _m: REPLACEMENT, x, count=1) for x in strs]
    t2 = time.perf_counter()
    result["python_re"] = {"kind": "python-re", "rows": m, "cores": 1, "contains_rows_per_s": m / (t1 - t0),
                           "replace_rows_per_s": m / (t2 - t1)}
    got = np.unpackbits(bits.cpu().numpy().view(np.uint8), bitorder="little")[:m].astype(bool)
    o = out_off[: m + 1].cpu().numpy()
    data = out[: int(o[m])].cpu().numpy().tobytes()
    bad_c = int(np.count_nonzero(got != np.array(hits)))
    bad_r = sum(data[o[i]:o[i + 1]].decode() != subs[i] for i in range(m))
    result["checked_rows"] = m
    result["mismatches"] = {"contains": bad_c, "replace_target": int(bad_r)}
    result["match_fraction_sample"] = float(np.mean(hits))
    result["speedup_vs_python_re"] = {
        "contains": result["ops"]["contains"]["rows_per_s"] / result["python_re"]["contains_rows_per_s"],
        "replace_target": result["ops"]["replace_target"]["rows_per_s"] / result["python_re"]["replace_rows_per_s"],
    }
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if bad_c == 0 and bad_r == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
