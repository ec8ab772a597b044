"""The row functions of the string transforms (rogtk_amd/csrc/strings_rows.h, the code the
GPU kernels run) compiled for the host (oracle/str_rows_host.cpp) against the oracle
(oracle/pystrings.py), byte for byte, over every row of tests/strings_cases.py.

This is where the CIGAR rows that decide how far a kernel reads and writes (numbers near
2^64, rows over ROGTK_STR_MAX_ROW_BYTES) run before any GPU sees them. The same input files
go through the sanitized build (`make -C oracle sanitize`) by hand on a CPU-only machine;
no test runs that binary.
"""
from __future__ import annotations

import os

import pytest

import strings_cases as C
from oracle import pystrings as O

BINARY = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "str_rows_host")


def test_known_answers_pin_the_oracle():
    """The written answers of strings_cases.KNOWN are what the oracle computes."""
    for op, param, vals, want in C.KNOWN:
        got = O.column(op, [[v] for v in vals], param)[0]
        assert got == want, (op, param, vals, got, want)
    for c in C.known_cases():
        assert C.expected(c) == [None if w is None else C.row_bytes(w) for w in c["want"]]


@pytest.mark.parametrize("name", C.RANDOM_NAMES)
def test_host_rows_random(name, tmp_path):
    case = C.random_case(name)
    want = C.expected(case)
    assert len(want) == 2000 and any(w is None for w in want) and any(w for w in want)
    assert C.run_harness(BINARY, case, tmp_path) == want


def test_host_rows_known_answers(tmp_path):
    for case in C.known_cases():
        got = C.run_harness(BINARY, case, tmp_path)
        want = [None if w is None else C.row_bytes(w) for w in case["want"]]
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (case["name"], i, [c[i] for c in case["cols"]], g, w)
        assert len(got) == len(want)


@pytest.mark.parametrize("case", C.OVER_CAP, ids=[c["name"] for c in C.OVER_CAP])
def test_host_rows_over_cap(case, tmp_path):
    """Over-cap rows measure as cap + 1 in time proportional to their input (the harness
    run has a time limit), are not filled, and leave their neighbours' bytes as they are."""
    want = C.expected(case)
    assert [i for i, w in enumerate(want) if isinstance(w, int)] == case["over"]
    assert C.run_harness(BINARY, case, tmp_path) == want
