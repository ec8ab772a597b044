#!/usr/bin/env python3
"""Level-2 (host Arrow buffers) rates, PCIe included: what a polars plugin sees.

Times the host entry points on 10M-row pyarrow columns: H2D copy of the column, the kernels
and the D2H copy of the results are all inside the timed region. The UMI entries run on
synth-v1 C2 UMIs as 12-byte strings; the string-out entries (reverse_complement,
fuzzy.replace_target, barcode.correct with its corrected column) on random 64-byte reads and
16-byte barcodes. `small_call_us` is the median of 1,000 reverse_complement calls on a 10-row
column: what a caller that goes group by group pays per call. Only the public Python API is
used. Never bench.py's `value`.
"""
import json
import os
import sys
import time

import numpy as np
import pyarrow as pa

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rogtk_amd as rg  # noqa: E402
from rogtk_amd import synth  # noqa: E402


def timed(fn, reps=3):
    fn()  # warm (allocations, LUT upload)
    best = 1e9
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t)
    return best


ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def as_column(rows):
    """A large_binary column over the rows of a 2-D uint8 array."""
    n, w = rows.shape
    offsets = np.arange(n + 1, dtype=np.int64) * w
    return pa.Array.from_buffers(pa.large_binary(), n, [None, pa.py_buffer(offsets), pa.py_buffer(rows.reshape(-1))])


def fixed_width(rng, n, w):
    return as_column(ACGT[rng.integers(0, 4, size=(n, w), dtype=np.uint8)])


def main():
    n = int(os.environ.get("N", "10000000"))
    L = 12
    umis = synth.umi_ascii(n, L)
    offsets = pa.py_buffer((np.arange(n + 1, dtype=np.int64) * L).tobytes())
    col = pa.Array.from_buffers(pa.large_binary(), n, [None, offsets, pa.py_buffer(umis.reshape(-1).tobytes())])
    out = {}
    out["umi_complexity_host"] = n / timed(lambda: rg.umi_complexity_scores(col))
    out["hamming_host"] = n / timed(lambda: rg.hamming_within(col, "ACGTACGTACGT", 1))
    out["umi_cluster_host"] = n / timed(lambda: rg.umi_cluster(col, L, 1))
    del col, umis
    from rogtk_amd import strings

    rng = np.random.default_rng(7)
    reads = fixed_width(rng, n, 64)
    out["reverse_complement_host"] = n / timed(lambda: strings.reverse_complement(reads))
    out["fuzzy_replace_target_host"] = n / timed(lambda: strings.FuzzyNamespace(reads).replace_target("ACGTACGT", "N"))
    small = reads.slice(0, 10)
    strings.reverse_complement(small)
    lat = []
    for _ in range(1000):
        t = time.perf_counter()
        strings.reverse_complement(small)
        lat.append(time.perf_counter() - t)
    del reads
    # 16-byte barcodes: 100k whitelist entries, 1 row in 5 with one substitution
    wl_codes = np.unique(rng.integers(0, 4, size=(100_000, 16), dtype=np.uint8), axis=0)
    rows = wl_codes[rng.integers(0, len(wl_codes), size=n)]
    hit = rng.random(n) < 0.2
    pos = rng.integers(0, 16, size=n)
    rows[hit, pos[hit]] = (rows[hit, pos[hit]] + rng.integers(1, 4, size=int(hit.sum()), dtype=np.uint8)) & 3
    wl = rg.BarcodeWhitelist(as_column(ACGT[wl_codes]))
    barcodes = as_column(ACGT[rows])
    del rows
    out["barcode_correct_host"] = n / timed(lambda: wl.correct(barcodes).corrected)
    print(json.dumps({"metric": "Level-2 host-buffer rate (PCIe H2D + kernels + D2H), rows/s", "rows": n,
                      "rates": {k: round(v, 1) for k, v in out.items()},
                      "small_call_us": round(float(np.median(lat)) * 1e6, 2),
                      "note": "pyarrow column in host memory; results copied back into Arrow buffers"}))


if __name__ == "__main__":
    main()
