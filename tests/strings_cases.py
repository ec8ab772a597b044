"""Rows for the element-wise string transforms (rogtk_amd/csrc/strings.hip), shared by the
CPU test of the host harness (tests/test_strings_rows_host.py: the kernels' row functions
compiled for the host) and by the GPU tests (tests/test_strings.py through Level 2,
tests/test_gpu_strings_device.py through Level 1). Every consumer runs every row: nothing
here is filtered on either side.

Three groups:
  random_case(op)   2,000 rows per op from the generators below, with nulls and some
                    2-, 3- and 4-byte UTF-8 characters;
  KNOWN             hand-written known answers at the CIGAR number limits (2^64 - 1, 2^64,
                    leading zeros), the lossy cuts of 3- and 4-byte characters, and the
                    `parse::<usize>` corners of the allele enrichment;
  OVER_CAP          columns holding rows whose output exceeds ROGTK_STR_MAX_ROW_BYTES. They
                    are a list of their own and are never part of a column that is expected
                    to succeed: Level 2 rejects the column, Level 1 and the harness report
                    cap + 1 for the row.
The expected values come from oracle/pystrings.py; the known answers are also written out,
so the oracle is pinned by them as well.
"""
from __future__ import annotations

import struct
import subprocess
from typing import List, Optional

import numpy as np

from oracle import pystrings as O

OPS = {"revcomp": 1, "parse_cigar": 2, "aligned_ref": 3, "aligned_query": 4, "cigar_insertions": 5, "enrich": 6,
       "phred_str": 7, "phred_list": 8}
MAX_ROW_BYTES = 2147483647  # ROGTK_STR_MAX_ROW_BYTES (include/rogtk_hip.h)
U64 = 18446744073709551615


# ------------------------------------------------------------------ generators
def _rand_dna(rng, n, lo, hi, alphabet="ACGT"):
    al = np.frombuffer(alphabet.encode(), np.uint8)
    return [bytes(rng.choice(al, int(rng.integers(lo, hi + 1)))).decode() for _ in range(n)]


def _rand_cigar(rng, qlen, ops="MIDNSHP=X"):
    parts, used = [], 0
    while used < qlen:
        op = ops[int(rng.integers(len(ops)))]
        k = int(rng.integers(0, 12))
        parts.append(f"{k}{op}")
        used += k if op in "MIS=X" else 0
    return "".join(parts)


def _sprinkle(rng, rows, every=7):
    """Every `every`-th row gets a few chars replaced by 2-, 3- and 4-byte UTF-8 chars."""
    out = list(rows)
    for i in range(3, len(out), every):
        s = list(out[i])
        for _ in range(min(len(s), 3)):
            s[int(rng.integers(len(s)))] = "é€😀"[int(rng.integers(3))]
        out[i] = "".join(s)
    return out


def _nulls(rows, start, step):
    out = list(rows)
    for i in range(start, len(out), step):
        out[i] = None
    return out


def _alleles(rng, seq, cig):
    """Alleles that reference the rows' insertions (1-based and 0-based positions), plus junk."""
    alleles = []
    for s, c in zip(seq, cig):
        ins = O.extract_insertions(s, c) if s is not None and c is not None else {}
        parts = ["AC"]
        for p in list(ins)[:3]:
            parts.append(f"[{p + int(rng.integers(0, 2))}:{len(ins[p])}I]")
        parts += ["[5:3D]", "[None]", "[x:1I]", "TT"]
        if rng.random() < 0.05:
            parts.append("[12:")
        alleles.append("".join(parts))
    return alleles


def random_case(name: str, n: int = 2000) -> dict:
    """{"name", "op", "param", "cols"}: n rows of op `name` ("parse_cigar_block" and
    "phred_str64" are the second parameter values of their ops)."""
    rng = np.random.default_rng(1000 + RANDOM_NAMES.index(name))
    op, param = name, 0
    if name == "revcomp":
        cols = [_nulls(_sprinkle(rng, _rand_dna(rng, n, 0, 300, "ACGTNacgtn")), 5, 13)]
    elif name in ("parse_cigar", "parse_cigar_block"):
        op, param = "parse_cigar", int(name.endswith("block"))
        cols = [_nulls([_rand_cigar(rng, 150) for _ in range(n)], 4, 11)]
    elif name in ("aligned_ref", "aligned_query"):
        ref = _sprinkle(rng, _rand_dna(rng, n, 0, 200, "ACGTacgtN"))
        qry = _sprinkle(rng, _rand_dna(rng, n, 0, 200, "ACGTacgtN"), 9)
        cig = [_rand_cigar(rng, len(q.encode())) for q in qry]
        cols = [_nulls(ref, 2, 17), _nulls(qry, 6, 19), _nulls(cig, 8, 23)]
    elif name in ("cigar_insertions", "enrich"):
        seq = _sprinkle(rng, _rand_dna(rng, n, 0, 160), 5)
        cig = [_rand_cigar(rng, len(s.encode()), "MIDS") for s in seq]
        if name == "enrich":
            al = _sprinkle(rng, _alleles(rng, seq, cig), 29)
            cols = [_nulls(al, 5, 31), _nulls(seq, 3, 37), _nulls(cig, 6, 41)]
        else:
            cols = [_nulls(seq, 3, 17), _nulls(cig, 6, 19)]
    elif name in ("phred_str", "phred_str64", "phred_list"):
        op, param = name.replace("64", ""), 64 if name.endswith("64") else 33
        rows = [bytes(rng.integers(33, 127, int(rng.integers(0, 200)), dtype=np.uint8)).decode() for _ in range(n)]
        cols = [_nulls(_sprinkle(rng, rows, 11), 7, 13)]
    else:
        raise ValueError(name)
    return {"name": name, "op": op, "param": param, "cols": cols}


RANDOM_NAMES = ["revcomp", "parse_cigar", "parse_cigar_block", "aligned_ref", "aligned_query", "cigar_insertions",
                "enrich", "phred_str", "phred_str64", "phred_list"]

# ------------------------------------------------------------------ known answers
_SEQ = "A€C😀GT"  # bytes: A 0 | € 1-3 | C 4 | 😀 5-8 | G 9 | T 10
_FF = "�"
# (op, param, one value per input column, the expected output row)
KNOWN = [
    ("parse_cigar", 0, [f"{U64}M3D2I"], "I,2,2"),  # ref wraps: end < ref, no single deletions
    ("parse_cigar", 1, [f"{U64}M3D2I"], f"D,{U64},3|I,2,2"),
    ("parse_cigar", 1, [f"{U64 + 1}D1M2I"], "I,1,2"),  # 2^64 overflows usize: the op is skipped
    ("parse_cigar", 1, ["00000000000000000000005D1I"], "D,0,5|I,5,1"),
    ("cigar_insertions", 0, [_SEQ, "1M1I"], "1:" + _FF),
    ("cigar_insertions", 0, [_SEQ, "1M3I"], "1:€"),
    ("cigar_insertions", 0, [_SEQ, "2M2I"], "2:" + _FF * 2),
    ("cigar_insertions", 0, [_SEQ, "4M2I"], "4:C" + _FF),
    ("cigar_insertions", 0, [_SEQ, "4M4I"], "4:C" + _FF),
    ("cigar_insertions", 0, [_SEQ, "5M3I1M"], "5:" + _FF),
    ("cigar_insertions", 0, [_SEQ, "1S3I"], "0:€"),
    # seq_pos wraps: the reference panics on these two; here "past the end of seq"
    ("cigar_insertions", 0, [_SEQ, f"{U64}S2I"], ""),
    ("cigar_insertions", 0, [_SEQ, f"1M{U64}I1I"], "1:A"),
    ("cigar_insertions", 0, [_SEQ, f"1M{U64}I1D1I"], "2:A"),  # the huge insertion is dropped, not read
    ("revcomp", 0, [_SEQ], "AC😀G€T"),
    ("phred_str", 33, ["I€😀\x7f"], "40|139|223|94"),
    ("phred_str", 64, ["!\""], "225|226"),
    ("phred_list", 33, ["I€😀\x7f"], [40, 139, 223, 94]),
    ("enrich", 0, ["[0:1I]", "ACGT", "1M1I2M"], "[0:1I]"),
    ("enrich", 0, ["[1:1I]", "ACGT", "1M1I2M"], "[1:1I:C]"),
    ("enrich", 0, ["[+1:1I]", "ACGT", "1M1I2M"], "[+1:1I:C]"),
    ("enrich", 0, ["[1:I]", "ACGT", "1M1I2M"], "[1:I:C]"),
    ("enrich", 0, ["[1:1I]]", "ACGT", "1M1I2M"], "[1:1I:C]]"),
] + [("enrich", 0, [a, "ACGT", "1M1I2M"], a) for a in [
    "[-1:1I]", "[:1I]", "[1:]", "[1:1I:X]", "[[1:1I]", f"[{U64}:1I]", f"[{U64 + 1}:1I]", "[ 1:1I]", "[1:1Iб]",
    "[б:1I]"]] + [
    ("aligned_ref", 0, ["aé", "Éa", "1M1D1S1I1X1=9N"], "AÃ--©"),
    ("aligned_query", 0, ["aé", "Éa", "1M1D1S1I1X1=9N"], "Ã-\x89A---------"),
    # the largest passing neighbours of the over-cap rows, at a size a test can hold
    ("aligned_ref", 0, ["ACGT", "ACGT", "2M1000000I2M"], "AC" + "-" * 1000000 + "GT"),
    ("parse_cigar", 0, ["5M100000D"], "|".join(f"D,{p},1" for p in range(5, 100005))),
]


def known_cases() -> List[dict]:
    """The known answers as one column per (op, param), in KNOWN's order, each with a null
    row in the middle; "want" holds the written answers."""
    out: List[dict] = []
    for op, param, vals, want in KNOWN:
        c = next((c for c in out if c["op"] == op and c["param"] == param), None)
        if c is None:
            c = {"name": f"known_{op}_{param}", "op": op, "param": param, "cols": [[] for _ in vals], "want": []}
            out.append(c)
        for col, v in zip(c["cols"], vals):
            col.append(v)
        c["want"].append(want)
    for c in out:
        k = len(c["want"]) // 2
        for col in c["cols"]:
            col.insert(k, None)
        c["want"].insert(k, None)
    return out


# ------------------------------------------------------------------ over the cap
# {"cols", "over": rows whose output exceeds MAX_ROW_BYTES}. Why each is over:
#   aligned_ref writes len '-' for I and S, aligned_query for D and N: len > cap;
#   parse_cigar without block_dels writes len records of >= 5 bytes: 5 * len > cap.
OVER_CAP = [
    # (at most two over-cap rows per column: a Level 1 caller's buffer spans them)
    {"name": "over_aligned_ref", "op": "aligned_ref", "param": 0, "over": [1, 3],
     "cols": [["ACGT"], ["ACGT"] * 5, ["4M", "4294967296I", "2M3I", f"{1 << 63}I", "1000000I"]]},
    {"name": "over_aligned_ref_clip", "op": "aligned_ref", "param": 0, "over": [1],
     "cols": [["ACGT"] * 3, ["ACGT"] * 3, ["1M", f"{U64}S", "2M"]]},
    {"name": "over_aligned_query", "op": "aligned_query", "param": 0, "over": [1],
     "cols": [["ACGT"] * 3, ["ACGT"] * 3, ["2M1D2M", f"1M{1 << 63}D", "4M"]]},
    {"name": "over_parse_cigar", "op": "parse_cigar", "param": 0, "over": [1, 3],
     "cols": [["3D", "99999999999D", "1M2D1I", "2147483647D", "100000D", None, "2D"]]},
    # two rows whose unguarded int64 sum (2^63 + 2^63) would come back as 0
    {"name": "over_two_rows", "op": "aligned_ref", "param": 0, "over": [0, 2],
     "cols": [["ACGT"] * 4, ["ACGT"] * 4, [f"{1 << 63}I", "1M", f"{1 << 63}I", "3M"]]},
]


# ------------------------------------------------------------------ expected values
def row_bytes(v) -> bytes:
    """An output row as the bytes the kernels write (PHRED_LIST: the u8 values)."""
    return v.encode() if isinstance(v, str) else bytes(v)


def expected(case: dict) -> List[Optional[bytes]]:
    """The oracle's output rows as bytes (None = null). For an OVER_CAP case the rows
    listed in "over" are not computed (the oracle would build them) and come back as the
    int MAX_ROW_BYTES + 1, the length every implementation must report for them."""
    cols, over = case["cols"], set(case.get("over", ()))
    n = max(len(c) for c in cols)
    out: List[Optional[bytes]] = []
    for i in range(n):
        if i in over:
            out.append(MAX_ROW_BYTES + 1)
            continue
        row = [[c[0] if len(c) == 1 else c[i]] for c in cols]
        v = O.column(case["op"], row, case["param"])[0]
        out.append(None if v is None else row_bytes(v))
    return out


def expected_lengths(want) -> List[int]:
    return [0 if w is None else w if isinstance(w, int) else len(w) for w in want]


# ------------------------------------------------------------------ the host harness's files
def write_harness_input(path, case: dict) -> None:
    """oracle/str_rows_host.cpp's input format."""
    cols = case["cols"]
    n = max(len(c) for c in cols)
    with open(path, "wb") as f:
        f.write(b"RSTRIN01" + struct.pack("<4q", OPS[case["op"]], case["param"], n, len(cols)))
        for c in cols:
            data = [b"" if v is None else v.encode() for v in c]
            offs = np.zeros(len(c) + 1, dtype="<i8")
            np.cumsum([len(d) for d in data], out=offs[1:])
            f.write(struct.pack("<3q", len(c), int(offs[-1]), 1))
            f.write(offs.tobytes() + b"".join(data) + bytes(v is not None for v in c))


def read_harness_output(path):
    """(lengths, valid, values) of oracle/str_rows_host.cpp's output file."""
    raw = open(path, "rb").read()
    assert raw[:8] == b"RSTROUT1"
    n = struct.unpack_from("<q", raw, 8)[0]
    lengths = np.frombuffer(raw, "<i8", n, 16)
    valid = np.frombuffer(raw, np.uint8, n, 16 + 8 * n).astype(bool)
    return lengths, valid, raw[16 + 9 * n:]


def run_harness(binary, case: dict, tmpdir):
    """Runs the harness on one case; returns its output rows as expected() spells them."""
    fin, fout = f"{tmpdir}/{case['name']}.in", f"{tmpdir}/{case['name']}.out"
    write_harness_input(fin, case)
    r = subprocess.run([binary, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (case["name"], r.returncode, r.stderr[-2000:])
    lengths, valid, values = read_harness_output(fout)
    rows, at = [], 0
    for ln, ok in zip(lengths.tolist(), valid.tolist()):
        if not ok:
            assert ln == 0
            rows.append(None)
        elif ln > MAX_ROW_BYTES:
            rows.append(ln)
        else:
            rows.append(values[at:at + ln])
            at += ln
    assert at == len(values)
    return rows
