"""The fuzzy kernels (rogtk_amd/csrc/fuzzy.hip) on programs and rows beyond the one-target
patterns of tests/test_fuzzy.py, against the plain matcher of tests/fuzzy_spec.py.

fuzzy.hip matches with three shortcuts over its atom-by-atom matcher: a 256-byte LDS window per
chunk of 64 starts, an 8-byte prefilter per alternative, and one measured agreement with the
program's longest literal run from which alternatives are skipped or declared dead. The
families here put each of them where it can go wrong: alternatives that share part of the
run, none of it, or whose order decides (general, order); matches that end past the window
(far window); code points of 3 and 4 bytes under a wildcard among the first 9 atoms (wide);
programs at the 512-alternative and 16,384-atom caps (caps). tests/test_fuzzy_spec.py checks
the spec against `re` and that the families hold what they are built to hold.

Every comparison is exact equality, on contains, replace-first and replace-all, with one null
row in each column.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pyarrow as pa
import pytest

import fuzzy_spec as S
from rogtk_amd import _lib
from rogtk_amd.strings import FuzzyNamespace, FuzzyProgram

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _with_null(values, at):
    return list(values[:at]) + [None] + list(values[at:])


def _bytes_of(arr: pa.Array):
    assert arr.type == pa.large_string()
    return arr.view(pa.large_binary()).to_pylist()


def _same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (what, i, a, b)


def check_case(case, exp, repl, what):
    """The three operations on the case's rows (one null among them) equal the spec's answers."""
    at = len(case.rows) // 2
    col = pa.array(_with_null(case.rows, at), type=pa.large_binary())
    ns = FuzzyNamespace(col)
    got = ns.contains(case.program, literal=case.is_literal)
    assert got.type == pa.bool_() and got.null_count == 1
    _same(got.to_pylist(), _with_null(exp.contains, at), (what, "contains"))
    got = ns.replace(case.program, repl, literal=case.is_literal)
    assert got.null_count == 1
    _same(_bytes_of(got), _with_null(exp.all, at), (what, "replace all"))
    prog = FuzzyProgram.pattern(case.program, literal=case.is_literal).set_replacement(repl)
    got = prog.replace(col, False)
    assert got.null_count == 1
    _same(_bytes_of(got), _with_null(exp.first, at), (what, "replace first"))
    # and the same program object answers contains and replace-all as the namespace did
    _same(prog.contains(col).to_pylist(), _with_null(exp.contains, at), (what, "program contains"))
    _same(_bytes_of(prog.replace(col, True)), _with_null(exp.all, at), (what, "program replace all"))


# ------------------------------------------------------------------ known answers
KNOWN = [  # program, row, replace-first, replace-all (replacement <R>), derived by hand
    ("A|AB", "xABAB", "x<R>BAB", "x<R>B<R>B"),
    ("AB|A", "xABAB", "x<R>AB", "x<R><R>"),
    ("AC.?|ACGT", "ACGTT", "<R>TT", "<R>TT"),
    ("ACGT|AC.?", "ACGTT", "<R>T", "<R>T"),
    ("A.C|A.?CG", "ACCGACG", "<R>GACG", "<R>G<R>"),
    ("A.?CG|A.C", "ACCGACG", "<R>ACG", "<R><R>"),
    # alternatives that share part of the longest literal run (ACGTACGT), and one that shares none
    ("ACGTACGT|ACGTTT|ACG.?ACC|TTG", "ACGTACC", "<R>", "<R>"),
    ("ACGTACGT|ACGTTT|ACG.?ACC|TTG", "ACGACCTTG", "<R>TTG", "<R><R>"),
    ("ACGTACGT|ACGTTT|ACG.?ACC|TTG", "ACG😀ACGACG€ACC", "ACG😀ACG<R>", "ACG😀ACG<R>"),
    ("ACGTACGT|ACGTTT|ACG.?ACC|TTG", "ACG\nACCACGTTTT", "ACG\nACC<R>T", "ACG\nACC<R>T"),
    ("ACGTACGT|ACGTTT|ACG.?ACC|TTG", "ACGTACGACGTACGT", "ACGTACG<R>", "ACGTACG<R>"),
    # after the optional T the row leaves the run at its sixth byte, which the prefilter sees
    ("ACGTACGT|ACGTTT|ACG.?ACC|TTG", "ACGTAGC", "ACGTAGC", "ACGTAGC"),
    ("ACGTACGT|ACGTTT|ACG.?ACC|TTG", "ACGTACCACGTAGCTTG", "<R>ACGTAGCTTG", "<R>ACGTAGC<R>"),
    # the same beyond the 8 bytes the prefilter sees: the optional C is taken, the row leaves
    # the run at byte 14 of 20, and the TT that ends the second alternative follows at byte 18
    ("ACGTTGCAAGCTTCGATCCG|ACGTTGCAAG.?TTCGATCTT|GGG", "ACGTTGCAAGCTTCAATCTT", "ACGTTGCAAGCTTCAATCTT", "ACGTTGCAAGCTTCAATCTT"),
    ("ACGTTGCAAGCTTCGATCCG|ACGTTGCAAG.?TTCGATCTT|GGG", "ACGTTGCAAGCTTCAATCTTGGG", "ACGTTGCAAGCTTCAATCTT<R>", "ACGTTGCAAGCTTCAATCTT<R>"),
    ("ACGTTGCAAGCTTCGATCCG|ACGTTGCAAG.?TTCGATCTT|GGG", "ACGTTGCAAGCTTCGATCTT", "<R>", "<R>"),
    ("ACGTTGCAAGCTTCGATCCG|ACGTTGCAAG.?TTCGATCTT|GGG", "ACGTTGCAAG€TTCGATCTT", "<R>", "<R>"),
    ("ACGTTGCAAGCTTCGATCCG|ACGTTGCAAG.?TTCGATCTT|GGG", "ACGTTGCAAGTTCGATCTTACGTTGCAAGCTTCGATCCG", "<R>ACGTTGCAAGCTTCGATCCG", "<R><R>"),
    # two wildcards of different widths in one alternative; a code point cut by "\n"
    ("A..T|GG", "A€😀TA\n€TGG", "<R>A\n€TGG", "<R>A\n€T<R>"),
]


def test_gpu_known_answers(gpu):
    for prog in sorted({k[0] for k in KNOWN}):
        rows = [k for k in KNOWN if k[0] == prog]
        case = S.Case(prog, False, [k[1].encode() for k in rows], [()] * len(rows))
        exp = S.expected_of(case)
        assert exp.first == [k[2].encode() for k in rows] and exp.all == [k[3].encode() for k in rows], prog
        check_case(case, exp, b"<R>", prog)


# ------------------------------------------------------------------ general
@pytest.mark.parametrize("part", range(4))
def test_gpu_general_programs(gpu, part):
    """Programs whose alternatives share all, part or none of the reference run, with several
    wildcards, on rows over code points of every width and "\\n"."""
    for seed in S.GENERAL_SEEDS[part::4]:
        check_case(S.case_of("general", seed), S.expected("general", seed), b"<R>", ("general", seed))


def test_gpu_order_decides(gpu):
    for k in range(len(S.ORDER_PAIRS)):
        for case in S.order(k):
            for repl in S.REPLACEMENTS:
                check_case(case, S.expected_of(case, repl), repl, ("order", case.program, repl))


# ------------------------------------------------------------------ far window
@pytest.mark.parametrize("kind", S.FAR_KINDS)
def test_gpu_far_window(gpu, kind):
    """Matches that end past byte c + 256 of their chunk, and near misses whose one wrong byte
    is the last one inside the window, one of the first two past it, or the match's last."""
    for repl in S.REPLACEMENTS:
        check_case(S.case_of("far", kind), S.expected("far", kind, repl=repl), repl, ("far", kind, repl))


def _level1(torch, prog, arr, replace_all):
    """contains, replace_measure and replace_fill on device tensors and an explicit stream:
    (hit bits, valid bits, the output rows as bytes or None)."""
    n = len(arr)
    bufs = arr.buffers()
    dev = torch.device("cuda:0")
    offs = torch.from_numpy(np.frombuffer(bufs[1], dtype=np.int64, count=n + 1).copy()).to(dev)
    vals = torch.from_numpy(np.frombuffer(bufs[2], dtype=np.uint8).copy()).to(dev)
    valid = torch.from_numpy(np.frombuffer(bufs[0], dtype=np.uint8).copy()).to(dev)
    col = _lib.StrCol(offs.data_ptr(), 8, vals.data_ptr(), vals.numel(), valid.data_ptr(), 0, n)
    words = (n + 63) // 64
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        bits = torch.zeros(words, dtype=torch.int64, device=dev)
        vbits = torch.zeros(words, dtype=torch.int64, device=dev)
        s = ctypes.c_void_p(stream.cuda_stream)
        _lib.call("rogtk_fuzzy_contains", prog.handle, ctypes.byref(col), bits.data_ptr(), vbits.data_ptr(), s)
        tb = ctypes.c_int64(0)
        _lib.call("rogtk_str_temp_bytes", n, ctypes.byref(tb))
        temp = torch.zeros(tb.value, dtype=torch.uint8, device=dev)
        out_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        rvbits = torch.zeros(words, dtype=torch.int64, device=dev)
        _lib.call("rogtk_fuzzy_replace_measure", prog.handle, ctypes.byref(col), int(replace_all),
                  out_off.data_ptr(), rvbits.data_ptr(), temp.data_ptr(), tb.value, s)
        stream.synchronize()
        total = int(out_off[n].item())
        out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device=dev)
        _lib.call("rogtk_fuzzy_replace_fill", prog.handle, ctypes.byref(col), int(replace_all),
                  out_off.data_ptr(), out.data_ptr(), s)
        stream.synchronize()

    def unpack(t):
        return np.unpackbits(t.cpu().numpy().view(np.uint8), bitorder="little")[:n].astype(bool)

    ok = unpack(vbits)
    assert np.array_equal(ok, unpack(rvbits))
    o = out_off.cpu().numpy()
    data = out.cpu().numpy()
    assert (data[total:] == 0xA5).all(), "replace_fill wrote past the measured length"
    raw = data.tobytes()
    rows = [raw[o[i]:o[i + 1]] if ok[i] else None for i in range(n)]
    return unpack(bits), ok, rows


@pytest.mark.parametrize("kind", S.FAR_KINDS)
def test_gpu_far_window_level1(gpu, kind):
    """The same family through rogtk_fuzzy_contains / replace_measure / replace_fill on device
    tensors: the bytes past a row's window are read from the caller's value buffer, not from
    the host path's staging buffer."""
    case, exp = S.case_of("far", kind), S.expected("far", kind)
    at = len(case.rows) // 2
    arr = pa.array(_with_null(case.rows, at), type=pa.large_binary())
    prog = FuzzyProgram.pattern(case.program, literal=case.is_literal).set_replacement(b"<R>")
    for replace_all, want in ((1, exp.all), (0, exp.first)):
        hit, ok, rows = _level1(gpu, prog, arr, replace_all)
        assert ok.tolist() == [r is not None for r in _with_null(case.rows, at)]
        _same([bool(h) if v else None for h, v in zip(hit, ok)], _with_null(exp.contains, at), (kind, "contains"))
        _same(rows, _with_null(want, at), (kind, "replace", replace_all))


# ------------------------------------------------------------------ wide code points
@pytest.mark.parametrize("kind", S.WIDE_KINDS)
def test_gpu_wide_code_points(gpu, kind):
    """A wildcard at atom 0..8 of a 16-atom alternative over code points of 1-4 bytes, at row
    start and at start offset 61: one program per (kind, atom)."""
    for j in S.WIDE_J:
        check_case(S.case_of("wide", kind, j), S.expected("wide", kind, j), b"<R>", ("wide", kind, j))


def test_gpu_wide_code_points_combined(gpu):
    """All 18 alternatives in one program, so every prefilter is tried at every start."""
    for repl in S.REPLACEMENTS:
        check_case(S.case_of("wide_combined"), S.expected("wide_combined", repl=repl), repl, ("wide combined", repl))


# ------------------------------------------------------------------ caps
def test_gpu_program_at_both_caps(gpu):
    """512 alternatives of 32 atoms: about 58 KB of dynamic LDS at launch; rows won by the
    first, a middle and the last alternative of the table, and by none."""
    check_case(S.case_of("caps_many"), S.expected("caps_many"), b"<R>", "caps many")


def test_gpu_program_at_the_atoms_cap(gpu):
    """4 alternatives of 4,096 atoms that share their first 3,000: the measured agreement with
    the reference run, and the winning alternative, run far past the window."""
    check_case(S.case_of("caps_long"), S.expected("caps_long"), b"<R>", "caps long")
