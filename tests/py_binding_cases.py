"""The forms in which one list of rows reaches a Python wrapper (tests/test_py_bindings.py and
tests/test_gpu_py_bindings.py): every Arrow string type, empty, one row, nulls on both sides of
a 64-row validity word, no valid row at all, a slice whose bit offset is no multiple of 8, and
chunked arrays of 0, 1 and 3 chunks with an empty chunk among them."""
from __future__ import annotations

import numpy as np
import pyarrow as pa

TYPES = {"string": pa.string(), "large_string": pa.large_string(), "binary": pa.binary(),
         "string_view": pa.string_view()}
N_ROWS = 70  # the smallest column that crosses a validity word at a bit offset of 3


def typed(rows, kind):
    """rows (str or None) as the Python values of the Arrow type: bytes for binary."""
    return [None if r is None else r.encode() for r in rows] if kind == "binary" else list(rows)


def forms(rows, kind):
    """[(name, column, its rows)] over the first 70 of rows (str or None; row 1 is not null and
    some other row is)."""
    t = TYPES[kind]
    rows = typed(rows[:N_ROWS], kind)
    assert len(rows) == N_ROWS and rows[1] is not None and None in rows[3:]
    r65 = [None if i in (0, 63, 64) else r for i, r in enumerate(rows[:65])]
    parent = pa.array(rows, type=t)
    return [
        ("empty", pa.array([], type=t), []),
        ("one_row", pa.array(rows[1:2], type=t), rows[1:2]),
        ("nulls_0_63_64", pa.array(r65, type=t), r65),
        ("all_null", pa.array([None] * 5, type=t), [None] * 5),
        ("pa_nulls", pa.nulls(3, t), [None] * 3),
        ("slice_3_of_70", parent.slice(3), rows[3:]),
        ("chunked_0", pa.chunked_array([], type=t), []),
        ("chunked_1", pa.chunked_array([parent]), rows),
        ("chunked_3", pa.chunked_array([parent.slice(0, 30), pa.array([], type=t), parent.slice(30)]), rows),
    ]


def umi_rows():
    """70 UMIs of 12 bytes in small families (one substitution apart, so clusters form), with
    nulls and a few rows that are not 12 bytes of ACGT."""
    rng = np.random.default_rng(11)
    parents = ["".join(rng.choice(list("ACGT"), size=12)) for _ in range(9)]
    rows = []
    for i in range(N_ROWS):
        u = list(parents[int(rng.integers(0, len(parents)))])
        if rng.random() < 0.3:
            u[int(rng.integers(0, 12))] = str(rng.choice(list("ACGT")))
        rows.append("".join(u))
    for i in (0, 20, 44, 66):
        rows[i] = None
    rows[7], rows[8], rows[31], rows[50], rows[69] = "", rows[9][:11], rows[9] + "A", "ACGTNACGTACG", rows[9].lower()
    return rows


def cigar_rows():
    rng = np.random.default_rng(12)
    rows = ["".join(f"{int(rng.integers(1, 40))}{rng.choice(list('MIDNS'))}" for _ in range(int(rng.integers(1, 6))))
            for _ in range(N_ROWS)]
    for i in (4, 33, 65):
        rows[i] = None
    rows[10] = ""
    return rows
