"""Level 1 of the string transforms (rogtk_str_temp_bytes -> rogtk_str_measure ->
rogtk_str_fill, include/rogtk_hip.h) on torch device tensors and a non-default stream,
against oracle/pystrings.py byte for byte.

Level 2 (rogtk_str_transform_host, tests/test_strings.py) rewrites every column to int64
offsets from 0 before a kernel sees it, so only these tests reach the kernels with int32
offsets, a first offset that is not 0, a validity bit offset, a broadcast null scalar and
the temp-size check. Rows: tests/strings_cases.py (shared with the host harness test).
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pyarrow as pa
import pytest

import strings_cases as C
from oracle import pybam
from oracle import pystrings as O
from rogtk_amd import _lib

pytestmark = pytest.mark.gpu

CANARY64 = 0x5A5A5A5A5A5A5A5A
CANARY8 = 0xA5
PRE, POST = b"\x82\xacPREFIX", b"\x80\x80POST"  # bytes around an embedded column (continuation bytes first)
VALIDITIES = ["absent", 0, 3, 69, "allnull"]
LAYOUTS = [(ow, embed, v) for ow in (4, 8) for embed in (False, True) for v in VALIDITIES]


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


@functools.lru_cache(maxsize=None)
def _case(name):
    return C.random_case(name)


def _effective(rows, validity):
    """The rows a kernel sees under a validity layout: no bitmap = every row valid (a null
    row's bytes are then its content), all-null = a bitmap of zeros over the same bytes."""
    if validity == "absent":
        return ["" if r is None else r for r in rows]
    if validity == "allnull":
        return [None] * len(rows)
    return list(rows)


@functools.lru_cache(maxsize=None)
def _expected(name, n, kind):
    """Expected rows of the first n rows of a random case (kind: "absent", "allnull" or
    "given"), computed once per module."""
    c = _case(name)
    cols = [_effective(col[:n], kind) for col in c["cols"]]
    return tuple(C.expected({"op": c["op"], "param": c["param"], "cols": cols}))


def _kind(validity):
    return validity if isinstance(validity, str) else "given"


def _dev_col(torch, rows, ow, embed, validity, keep):
    """A device column of `rows` in the given layout; the tensors go to `keep`."""
    n = len(rows)
    if validity == "absent":  # the bytes of a null row are content without a bitmap: none
        data = [b"" if r is None else r.encode() for r in rows]
    else:  # null rows may own bytes (Arrow allows it): the kernels must not show them
        data = [(b"zz" if i % 2 else b"") if r is None else r.encode() for i, r in enumerate(rows)]
    pre, post = (PRE, POST) if embed else (b"", b"")
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(d) for d in data], out=offs[1:])
    offs += len(pre)
    vals = np.frombuffer(pre + b"".join(data) + post + b"\x00", dtype=np.uint8)
    dev = torch.device("cuda:0")
    t_off = torch.from_numpy(offs.astype(np.int32 if ow == 4 else np.int64)).to(dev)
    t_val = torch.from_numpy(vals.copy()).to(dev)
    keep += [t_off, t_val]
    if validity == "absent":
        return _lib.StrCol(t_off.data_ptr(), ow, t_val.data_ptr(), t_val.numel(), None, 0, n)
    bit_off = 0 if validity == "allnull" else int(validity)
    bits = np.ones(bit_off + n + 29, dtype=np.uint8)  # bits outside the column's window: junk
    bits[:bit_off] = np.arange(bit_off) % 3 == 0
    bits[bit_off:bit_off + n] = [validity != "allnull" and r is not None for r in rows]
    t_bits = torch.from_numpy(np.packbits(bits, bitorder="little")).to(dev)
    keep.append(t_bits)
    return _lib.StrCol(t_off.data_ptr(), ow, t_val.data_ptr(), t_val.numel(), t_bits.data_ptr(), bit_off, n)


class Level1:
    """One measure (+ fill) through the device API on a stream of its own."""

    def __init__(self, torch):
        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.stream = torch.cuda.Stream(device=self.dev)
        self.s = ctypes.c_void_p(self.stream.cuda_stream)

    def temp_bytes(self, n):
        tb = ctypes.c_int64(0)
        _lib.call("rogtk_str_temp_bytes", n, ctypes.byref(tb))
        return tb.value

    def measure(self, op, param, cols, n):
        """(offsets[n + 1], valid bools[n]); checks the words past the outputs and the
        validity bits at or above n."""
        torch = self.torch
        arr = (_lib.StrCol * len(cols))(*cols)
        words = (n + 63) // 64
        tb = self.temp_bytes(n)
        torch.cuda.synchronize()
        with torch.cuda.stream(self.stream):
            temp = torch.empty(tb, dtype=torch.uint8, device=self.dev)
            self.out_off = torch.full((n + 2,), CANARY64, dtype=torch.int64, device=self.dev)
            vbits = torch.full((words + 1,), CANARY64, dtype=torch.int64, device=self.dev)
            _lib.call("rogtk_str_measure", C.OPS[op], arr, len(cols), n, param, self.out_off.data_ptr(),
                      vbits.data_ptr(), temp.data_ptr(), tb, self.s)
            self.stream.synchronize()
        o = self.out_off.cpu().numpy()
        v = vbits.cpu().numpy()
        assert o[n + 1] == CANARY64 and v[words] == CANARY64
        bits = np.unpackbits(v[:words].view(np.uint8), bitorder="little")
        assert not bits[n:].any(), "validity bits at or above n_rows are set"
        return o[:n + 1].copy(), bits[:n].astype(bool)

    def fill(self, op, param, cols, n, nbytes):
        """The output buffer (nbytes + 64 canary bytes) after rogtk_str_fill on the measured offsets."""
        torch = self.torch
        arr = (_lib.StrCol * len(cols))(*cols)
        with torch.cuda.stream(self.stream):
            out = torch.full((nbytes + 64,), CANARY8, dtype=torch.uint8, device=self.dev)
            _lib.call("rogtk_str_fill", C.OPS[op], arr, len(cols), n, param, self.out_off.data_ptr(),
                      out.data_ptr(), self.s)
            self.stream.synchronize()
        return out

    def run(self, op, param, cols, n):
        offs, valid = self.measure(op, param, cols, n)
        out = self.fill(op, param, cols, n, int(offs[n])).cpu().numpy()
        assert (out[int(offs[n]):] == CANARY8).all(), "bytes written past the total"
        return offs, valid, out[:int(offs[n])].tobytes()


def _check(got, want, what):
    """Offsets, total, bytes, null rows of length 0 and validity, all exact."""
    offs, valid, data = got
    lens = C.expected_lengths(want)
    exp_off = np.zeros(len(want) + 1, dtype=np.int64)
    np.cumsum(lens, out=exp_off[1:])
    assert valid.tolist() == [w is not None for w in want], what
    bad = np.nonzero(offs != exp_off)[0]
    assert bad.size == 0, (what, "first differing offset", int(bad[0]), int(offs[bad[0]]), int(exp_off[bad[0]]))
    assert all(offs[i] == offs[i + 1] for i, w in enumerate(want) if w is None), what
    assert int(offs[-1]) == len(data) == sum(lens), what
    assert data == b"".join(w or b"" for w in want), what


@pytest.mark.parametrize("name", C.RANDOM_NAMES)
def test_level1_layouts(gpu, name):
    """Every op under int32 / int64 offsets x offsets from 0 / inside a larger buffer x
    validity absent / at bit 0, 3, 69 / all-null; 257 rows (two blocks, a partial wave)."""
    c, n, run = _case(name), 257, Level1(gpu)
    for ow, embed, validity in LAYOUTS:
        keep: list = []
        cols = [_dev_col(gpu, col[:n], ow, embed, validity, keep) for col in c["cols"]]
        want = _expected(name, n, _kind(validity))
        _check(run.run(c["op"], c["param"], cols, n), want, (name, ow, embed, validity))
    assert any(w is None for w in _expected(name, n, "given")) and all(
        w is not None for w in _expected(name, n, "absent"))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_level1_row_counts(gpu, n):
    """Every op at the row counts around a wave and a block; the layout rotates with the op."""
    run = Level1(gpu)
    for k, name in enumerate(C.RANDOM_NAMES):
        c = _case(name)
        ow, embed, validity = LAYOUTS[(7 * k + n) % len(LAYOUTS)]
        keep: list = []
        cols = [_dev_col(gpu, col[:n], ow, embed, validity, keep) for col in c["cols"]]
        _check(run.run(c["op"], c["param"], cols, n), _expected(name, n, _kind(validity)), (name, n, ow, embed, validity))


@pytest.mark.parametrize("op", ["aligned_ref", "aligned_query"])
def test_level1_broadcast_reference(gpu, op):
    """A 1-row first column, valid and null, beside longer ones: row 0 for every row."""
    c, n, run = _case(op), 300, Level1(gpu)
    qry, cig = c["cols"][1][:n], c["cols"][2][:n]
    for ref in (["ACGTACGTAAccé"], [None]):
        for ow, embed, validity in ((4, True, 3), (8, False, 69), (8, True, 0)):
            keep: list = []
            cols = [_dev_col(gpu, r, ow, embed, validity, keep) for r in (ref, qry, cig)]
            want = [None if v is None else C.row_bytes(v) for v in O.column(op, [ref, qry, cig])]
            _check(run.run(op, 0, cols, n), want, (op, ref, ow, embed, validity))
            assert (ref[0] is None) == all(w is None for w in want)


@pytest.mark.parametrize("name", C.RANDOM_NAMES)
def test_level1_equals_level2(gpu, name):
    from rogtk_amd import strings

    c, n = _case(name), 1000
    keep: list = []
    cols = [_dev_col(gpu, col[:n], 4, True, 3, keep) for col in c["cols"]]
    offs, valid, data = Level1(gpu).run(c["op"], c["param"], cols, n)
    arrays = [pa.array(col[:n], type=pa.large_string()) for col in c["cols"]]
    n2, offs2, vals2, bits2, nulls2 = strings._transform(C.OPS[c["op"]], arrays, c["param"])
    assert n2 == n and np.array_equal(offs, offs2) and data == vals2.tobytes()
    assert np.array_equal(valid, np.unpackbits(bits2, bitorder="little")[:n].astype(bool))
    assert nulls2 == int((~valid).sum())


def test_level1_known_answers(gpu):
    """The known answers of strings_cases.KNOWN (CIGAR numbers at 2^64 - 1 and 2^64, lossy
    cuts of 3- and 4-byte chars, the parse::<usize> corners) through the device API."""
    run = Level1(gpu)
    for c in C.known_cases():
        want = [None if w is None else C.row_bytes(w) for w in c["want"]]
        for ow, embed, validity in ((4, True, 69), (8, False, 0)):
            keep: list = []
            cols = [_dev_col(gpu, col, ow, embed, validity, keep) for col in c["cols"]]
            _check(run.run(c["op"], c["param"], cols, len(want)), want, (c["name"], ow))


def test_level1_errors_launch_nothing(gpu):
    """temp_bytes one byte short, a wrong n_cols and a column of 2 rows beside 5 are
    ROGTK_E_INVALID, and the outputs keep their canaries."""
    torch, n = gpu, 5
    keep: list = []
    rows = ["ACGT", None, "A", "", "GGC"]
    col = _dev_col(torch, rows, 8, False, 0, keep)
    short = _dev_col(torch, rows[:2], 8, False, 0, keep)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    s = ctypes.c_void_p(stream.cuda_stream)
    tb = ctypes.c_int64(0)
    _lib.call("rogtk_str_temp_bytes", n, ctypes.byref(tb))
    temp = torch.zeros(tb.value, dtype=torch.uint8, device=dev)
    out_off = torch.full((n + 1,), CANARY64, dtype=torch.int64, device=dev)
    vbits = torch.full((1,), CANARY64, dtype=torch.int64, device=dev)
    out = torch.full((64,), CANARY8, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    lib = _lib.hip()

    def measure(op, cols, temp_bytes):
        arr = (_lib.StrCol * len(cols))(*cols)
        return lib.rogtk_str_measure(C.OPS[op], arr, len(cols), n, 0, out_off.data_ptr(), vbits.data_ptr(),
                                     temp.data_ptr(), temp_bytes, s)

    def fill(op, cols):
        arr = (_lib.StrCol * len(cols))(*cols)
        return lib.rogtk_str_fill(C.OPS[op], arr, len(cols), n, 0, out_off.data_ptr(), out.data_ptr(), s)

    assert measure("revcomp", [col], tb.value - 1) == _lib.ROGTK_E_INVALID
    assert "temp_bytes" in lib.rogtk_last_error().decode()
    assert measure("revcomp", [col, col], tb.value) == _lib.ROGTK_E_INVALID
    assert measure("cigar_insertions", [col], tb.value) == _lib.ROGTK_E_INVALID
    assert measure("cigar_insertions", [col, short], tb.value) == _lib.ROGTK_E_INVALID
    assert "2 rows" in lib.rogtk_last_error().decode()
    assert fill("revcomp", [col, col]) == _lib.ROGTK_E_INVALID
    assert fill("cigar_insertions", [short, col]) == _lib.ROGTK_E_INVALID
    torch.cuda.synchronize()
    assert (out_off.cpu().numpy() == CANARY64).all() and int(vbits.item()) == CANARY64
    assert (out.cpu().numpy() == CANARY8).all()
    # and the same buffers with the right arguments work
    assert measure("revcomp", [col], tb.value) == _lib.ROGTK_OK
    stream.synchronize()
    assert out_off.cpu().numpy().tolist() == [0, 4, 4, 5, 5, 8]


@pytest.mark.parametrize("case", C.OVER_CAP, ids=[c["name"] for c in C.OVER_CAP])
def test_over_cap_rows(gpu, case):
    """A row over ROGTK_STR_MAX_ROW_BYTES: Level 2 refuses the column naming the row; Level 1
    measures cap + 1 for it and the right lengths for its neighbours, and fill on those
    offsets writes the neighbours alone. (These rows ran through the host harness, plain
    and sanitized, before they ran here: tests/test_strings_rows_host.py.)"""
    from rogtk_amd import strings

    torch = gpu
    want = C.expected(case)
    n = len(want)
    arrays = [pa.array(col, type=pa.large_string()) for col in case["cols"]]
    with pytest.raises(_lib.RogtkError) as ei:
        strings._transform(C.OPS[case["op"]], arrays, case["param"])
    assert ei.value.code == _lib.ROGTK_E_UNSUPPORTED and f"row {case['over'][0]}:" in str(ei.value)

    run = Level1(torch)
    keep: list = []
    cols = [_dev_col(torch, col, 8, True, 3, keep) for col in case["cols"]]
    offs, valid = run.measure(case["op"], case["param"], cols, n)
    assert np.diff(offs).tolist() == C.expected_lengths(want)
    assert [int(x) for x in np.diff(offs)[case["over"]]] == [C.MAX_ROW_BYTES + 1] * len(case["over"])
    assert valid.tolist() == [w is not None for w in want]
    out = run.fill(case["op"], case["param"], cols, n, int(offs[n]))
    for i, w in enumerate(want):
        if isinstance(w, bytes):
            a = int(offs[i])
            assert out[a:a + len(w)].cpu().numpy().tobytes() == w, (case["name"], i)
            out[a:a + len(w)] = CANARY8
    assert bool((out == CANARY8).all()), "bytes written outside the neighbours' ranges"


def test_bam_sequence_column_composes_with_revcomp(gpu, tmp_path):
    """The sequence column of one rogtk_bam_next_dev batch (device pointers as they come:
    int64 offsets, validity words) into Level 1 reverse complement."""
    from rogtk_amd import bam, synth_bam

    torch = gpu
    rng = np.random.default_rng(11)
    seqs = ["".join(rng.choice(list("ACGTN"), int(rng.integers(1, 200)))) for _ in range(500)]
    seqs[17] = seqs[63] = seqs[499] = ""  # no sequence: a null row
    path = str(tmp_path / "rows.bam")
    synth_bam.write_bam(path, [(b"chr1", 100000)],
                        [synth_bam.record_bytes(name=f"r{i}".encode(), ref_id=0, pos=i, flag=0, seq=s)
                         for i, s in enumerate(seqs)], block=4099)
    rows = pybam.bam_rows(path, "htslib")
    want = [None if r["sequence"] is None else O.reverse_complement(r["sequence"]).encode() for r in rows]
    assert len(want) == 500 and sum(w is None for w in want) == 3

    run = Level1(torch)
    with bam.BamReader(path) as rd:
        n, b = bam._next_dev(rd, 1 << 20, "htslib", True, run.stream)
        assert n == 500
        col = _lib.StrCol(b.offsets[2], 8, b.values[2], -1, b.validity[2], 0, n)
        got = run.run("revcomp", 0, [col], n)
        rd.check(run.stream)
    _check(got, want, "bam sequence -> revcomp")
