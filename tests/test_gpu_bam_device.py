"""The device BAM path (config C5) on the cases of tests/bam_device_cases.py: decode without a
host sync (rogtk_bam_next_dev on a real stream), the UMI column of a batch
(rogtk_bam_umi_dev), the appends at a device-side byte count (rogtk_bam_umi_append /
rogtk_bam_append_strings, _DevColumn), the range concatenation (rogtk_concat_strings_dev),
the deferred corrupt-record error (rogtk_bam_check) and bam_umi_cluster / bams_umi_cluster end
to end, against oracle/pybam.py, oracle/pyoracle.py and numpy. Every comparison is exact:
bytes, bits and ids. tests/test_bam_device_cases.py (CPU) holds the conditions that keep these
tests from passing vacuously (mixed validity words, empty UMIs, 762-byte names, ...).

Every call runs on a real torch.cuda.Stream: a NULL stream takes the synchronous path that
tests/test_bam.py covers. Output buffers carry canaries before and after what a call may
write, and validity words are pre-filled with ones, so a store out of range or a bit past the
last row shows.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import bam_device_cases as C
from oracle import pybam
from oracle import pyoracle as P

pytestmark = pytest.mark.gpu

G = 8  # canary elements on each side of an output
CAN8, CAN64 = 0xA5, -0x5A5A5A5A5A5A5A5B
SOURCES = ("sequence", "name")


@pytest.fixture(scope="module")
def torch():
    import torch as t

    return t


@pytest.fixture(scope="module")
def dev(torch):
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module")
def stream(torch):
    s = torch.cuda.Stream()
    assert s.cuda_stream  # a real stream, not the NULL one
    return s


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("bamdev")
    out = {"f": str(d / "device.bam"), "f2": str(d / "device2.bam"), "empty": str(d / "header_only.bam")}
    C.write_device_bam(out["f"], C.SEED)
    C.write_device_bam(out["f2"], C.SEED2)
    C.write_header_only_bam(out["empty"])
    return out


_ROWS = {}


def oracle_rows(path, mode):
    """pybam.bam_rows, computed once per (file, mode) and shared (never modified)."""
    if (path, mode) not in _ROWS:
        _ROWS[path, mode] = pybam.bam_rows(path, mode)
    return _ROWS[path, mode]


# ------------------------------------------------------------------ helpers
def _up(torch, dev, a):
    """A numpy array on the device (uint64 words as int64); never an empty allocation."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.size == 0:
        a = np.zeros(1, a.dtype)
    return torch.from_numpy(a.copy()).to(dev)


class Guarded:
    """n elements of device memory between two canary zones; `fill` is what the n elements
    hold before the call (the canary unless given)."""

    def __init__(self, torch, dev, n, dtype, fill=None):
        can = CAN8 if dtype == torch.uint8 else CAN64
        self.n, self.can, self.item = n, can, 1 if dtype == torch.uint8 else 8
        self.whole = torch.full((n + 2 * G,), can, dtype=dtype, device=dev)
        if fill is not None:
            self.whole[G:G + n] = fill
        self.ptr = ctypes.c_void_p(self.whole.data_ptr() + G * self.item)

    def get(self):
        """The n elements as numpy, after checking both canary zones."""
        w = self.whole.cpu().numpy()
        assert (w[:G] == self.can).all() and (w[G + self.n:] == self.can).all(), "canary overwritten"
        return w[G:G + self.n]


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _sp(stream):
    return ctypes.c_void_p(stream.cuda_stream)


def _batch(torch, dev, hb, with_valid=True):
    """A rogtk_bam_batch over a hand batch's name and sequence columns (+ the tensors)."""
    from rogtk_amd import _lib

    t = {k: _up(torch, dev, hb[k]) for k in ("name_off", "name_val", "seq_off", "seq_val", "seq_valid")}
    b = _lib.BamBatch()
    b.offsets[0], b.values[0] = t["name_off"].data_ptr(), t["name_val"].data_ptr()
    b.offsets[2], b.values[2] = t["seq_off"].data_ptr(), t["seq_val"].data_ptr()
    b.validity[2] = t["seq_valid"].data_ptr() if with_valid else None
    return b, t


# ------------------------------------------------------------------ a. concat
def _concat(torch, dev, stream, parts, cap=None):
    from rogtk_amd import _lib

    exp_off, exp_val, exp_words = C.expect_concat(parts)
    n, total = len(exp_off) - 1, int(exp_off[-1])
    cap = total if cap is None else cap
    k = len(parts)
    with torch.cuda.stream(stream):
        d = [(_up(torch, dev, o), _up(torch, dev, v), _up(torch, dev, w)) for o, v, w, _ in parts]
        off = Guarded(torch, dev, n + 1, torch.int64)
        val = Guarded(torch, dev, max(total, cap), torch.uint8)
        vw = Guarded(torch, dev, (n + 63) // 64, torch.int64, fill=-1)
        base = Guarded(torch, dev, 1, torch.int64)
        ovf = Guarded(torch, dev, 1, torch.int64)
        Pk = ctypes.c_void_p * k
        _lib.call("rogtk_concat_strings_dev", k, Pk(*[x[0].data_ptr() for x in d]) if k else None,
                  Pk(*[x[1].data_ptr() for x in d]) if k else None, Pk(*[x[2].data_ptr() for x in d]) if k else None,
                  (ctypes.c_int64 * k)(*[c for _, _, _, c in parts]) if k else None, off.ptr, val.ptr, cap, vw.ptr,
                  base.ptr, ovf.ptr, _sp(stream))
        stream.synchronize()
        got = off.get(), val.get(), _u64(vw.get()), int(base.get()[0]), int(ovf.get()[0])
    return got, (exp_off, exp_val, exp_words, n, total)


@pytest.mark.parametrize("counts", [C.CONCAT_COUNTS, (130,), (), (0, 0, 0), (64, 64), (63, 1, 1, 63)])
def test_concat_strings_dev_matches_numpy(torch, dev, stream, counts):
    parts = C.concat_parts(1, counts)
    (off, val, words, base, ovf), (e_off, e_val, e_words, n, total) = _concat(torch, dev, stream, parts)
    assert np.array_equal(off, e_off)
    assert np.array_equal(val[:total], e_val) and (val[total:] == CAN8).all()
    assert np.array_equal(words, e_words), [hex(int(x) ^ int(y)) for x, y in zip(words, e_words)]
    if n % 64:
        assert int(words[-1]) >> (n % 64) == 0  # bits past n
    assert base == total and ovf == 0


def test_concat_strings_dev_overflow(torch, dev, stream):
    parts = C.concat_parts(1)
    e_off, e_val, _ = C.expect_concat(parts)
    total = int(e_off[-1])
    cap = total - 1
    (off, val, words, base, ovf), (_, _, e_words, n, _) = _concat(torch, dev, stream, parts, cap=cap)
    past = e_off[1:] > cap
    assert past.sum() >= 1 and ovf == int(past.sum())
    assert np.array_equal(off, e_off) and base == total  # still the true offsets
    assert np.array_equal(words, e_words)
    for i in np.flatnonzero(~past):
        assert np.array_equal(val[e_off[i]:e_off[i + 1]], e_val[e_off[i]:e_off[i + 1]])
    assert (val[cap:] == CAN8).all()  # nothing at or past the cap
    for i in np.flatnonzero(past):  # a row that does not fit is not written at all
        assert (val[e_off[i]:min(e_off[i + 1], cap)] == CAN8).all()


# ------------------------------------------------------------------ b. rogtk_bam_umi_dev
def _umi_dev(torch, dev, stream, b, n, source, umi_len, sep, exp, cap=None):
    from rogtk_amd import _lib

    e_off, e_val, e_words = C.column(exp)
    total = int(e_off[-1])
    with torch.cuda.stream(stream):
        off = Guarded(torch, dev, n + 1, torch.int64)
        val = Guarded(torch, dev, max(total, 1), torch.uint8)
        vw = Guarded(torch, dev, (n + 63) // 64, torch.int64, fill=-1)
        try:
            _lib.call("rogtk_bam_umi_dev", ctypes.byref(b), n, source, umi_len, ord(sep), off.ptr, val.ptr,
                      total if cap is None else cap, vw.ptr, _sp(stream))
        finally:
            stream.synchronize()
    return (off, val, vw), (e_off, e_val, e_words, total)


@pytest.mark.parametrize("with_valid", [True, False])
@pytest.mark.parametrize("source", [0, 1])
def test_bam_umi_dev_on_a_hand_batch(torch, dev, stream, source, with_valid):
    n = 200
    hb = C.hand_batch(3, n)
    with torch.cuda.stream(stream):
        b, keep = _batch(torch, dev, hb, with_valid)
    for sep in "_:":
        for umi_len in (1, 12, 40):
            exp = C.expect_umis(hb["names"], hb["seqs"], hb["valid"] if with_valid else None, source, umi_len, sep)
            (off, val, vw), (e_off, e_val, e_words, total) = _umi_dev(torch, dev, stream, b, n, source, umi_len, sep,
                                                                      exp)
            assert total > 0
            assert np.array_equal(off.get(), e_off), (sep, umi_len)
            assert np.array_equal(val.get()[:total], e_val), (sep, umi_len)
            words = _u64(vw.get())
            assert np.array_equal(words, e_words), (sep, umi_len)
            assert int(words[-1]) >> (n % 64) == 0
            assert C.column_items(off.get(), val.get(), words, n) == exp
    del keep


@pytest.mark.parametrize("source", [0, 1])
def test_bam_umi_dev_overflow_writes_nothing(torch, dev, stream, source):
    from rogtk_amd import RogtkError, _lib

    n = 200
    hb = C.hand_batch(3, n)
    with torch.cuda.stream(stream):
        b, keep = _batch(torch, dev, hb)
    exp = C.expect_umis(hb["names"], hb["seqs"], hb["valid"], source, 12, "_")
    total = int(C.column(exp)[0][-1])
    with torch.cuda.stream(stream):
        off = Guarded(torch, dev, n + 1, torch.int64)
        val = Guarded(torch, dev, total, torch.uint8)
        vw = Guarded(torch, dev, (n + 63) // 64, torch.int64, fill=-1)
        with pytest.raises(RogtkError, match="exceed values_cap") as e:
            _lib.call("rogtk_bam_umi_dev", ctypes.byref(b), n, source, 12, ord("_"), off.ptr, val.ptr, total - 1,
                      vw.ptr, _sp(stream))
        stream.synchronize()
    assert e.value.code == _lib.ROGTK_E_OVERFLOW
    assert (val.get() == CAN8).all()
    del keep


# ------------------------------------------------------------------ c. appends
def _append_all(torch, dev, stream, hb, source, cap=None):
    """The six batches of APPEND_COUNTS appended into one UMI column and one name column."""
    from rogtk_amd import _lib

    n = len(hb["names"])
    exp = C.expect_umis(hb["names"], hb["seqs"], hb["valid"], source, 12, "_")
    e_off, e_val, e_words = C.column(exp)
    total, ntotal = int(e_off[-1]), int(hb["name_off"][-1])
    cap = total if cap is None else cap
    with torch.cuda.stream(stream):
        off = Guarded(torch, dev, n + 1, torch.int64)
        val = Guarded(torch, dev, total, torch.uint8)
        vw = Guarded(torch, dev, (n + 63) // 64, torch.int64, fill=0)  # zeroed once
        base = Guarded(torch, dev, 1, torch.int64, fill=0)
        ovf = Guarded(torch, dev, 1, torch.int64, fill=0)
        noff = Guarded(torch, dev, n + 1, torch.int64)
        nval = Guarded(torch, dev, ntotal, torch.uint8)
        nbase = Guarded(torch, dev, 1, torch.int64, fill=0)
        novf = Guarded(torch, dev, 1, torch.int64, fill=0)
        keep, row = [], 0
        for c in C.APPEND_COUNTS:
            b, t = _batch(torch, dev, C.slice_batch(hb, row, row + c))
            keep.append(t)
            _lib.call("rogtk_bam_umi_append", ctypes.byref(b), c, source, 12, ord("_"), off.ptr, val.ptr, cap, vw.ptr,
                      row, base.ptr, ovf.ptr, _sp(stream))
            _lib.call("rogtk_bam_append_strings", ctypes.c_void_p(b.offsets[0]), ctypes.c_void_p(b.values[0]), c,
                      noff.ptr, nval.ptr, ntotal, row, nbase.ptr, novf.ptr, _sp(stream))
            row += c
        assert row == n
        stream.synchronize()
    return (off, val, vw, base, ovf, noff, nval, nbase, novf), (exp, e_off, e_val, e_words, total)


@pytest.mark.parametrize("source", [0, 1])
def test_appends_equal_the_whole_column(torch, dev, stream, source):
    n = sum(C.APPEND_COUNTS)
    hb = C.hand_batch(3, n)
    (off, val, vw, base, ovf, noff, nval, nbase, novf), (exp, e_off, e_val, e_words, total) = _append_all(
        torch, dev, stream, hb, source)
    assert np.array_equal(off.get(), e_off)
    assert np.array_equal(val.get(), e_val)
    words = _u64(vw.get())
    assert np.array_equal(words, e_words), [hex(int(x) ^ int(y)) for x, y in zip(words, e_words)]
    assert int(base.get()[0]) == total and int(ovf.get()[0]) == 0
    assert C.column_items(off.get(), val.get(), words, n) == exp
    # the names: the same append without a validity
    assert np.array_equal(noff.get(), hb["name_off"]) and np.array_equal(nval.get(), hb["name_val"])
    assert int(nbase.get()[0]) == int(hb["name_off"][-1]) and int(novf.get()[0]) == 0


@pytest.mark.parametrize("source", [0, 1])
def test_appends_past_a_cap_are_counted_not_written(torch, dev, stream, source):
    n = sum(C.APPEND_COUNTS)
    hb = C.hand_batch(3, n)
    e_off = C.column(C.expect_umis(hb["names"], hb["seqs"], hb["valid"], source, 12, "_"))[0]
    mid = int(np.flatnonzero(np.diff(e_off) >= 2)[n // 3])  # a cap inside a row in the middle of the column
    cap = int(e_off[mid]) + 1
    (off, val, vw, base, ovf, *_), (exp, e_off, e_val, e_words, total) = _append_all(torch, dev, stream, hb, source,
                                                                                     cap=cap)
    past = e_off[1:] > cap
    assert 0 < past.sum() < n and 0 < cap < total
    assert int(ovf.get()[0]) == int(past.sum())
    assert np.array_equal(off.get(), e_off) and int(base.get()[0]) == total
    assert np.array_equal(_u64(vw.get()), e_words)
    v = val.get()
    first = int(np.flatnonzero(past)[0])
    assert np.array_equal(v[:e_off[first]], e_val[:e_off[first]])  # earlier rows intact
    assert (v[e_off[first]:] == CAN8).all()  # nothing of a row past the cap, nothing past the cap


@pytest.mark.parametrize("source", [0, 1])
def test_dev_column_grows_on_the_stream(torch, dev, stream, source):
    """_DevColumn from 64 rows / 16 bytes: offsets, validity words and values all grow several
    times between the appends, by copies on the stream."""
    from rogtk_amd import RogtkError
    from rogtk_amd import bam as B

    n = sum(C.APPEND_COUNTS)
    hb = C.hand_batch(3, n)
    exp = C.expect_umis(hb["names"], hb["seqs"], hb["valid"], source, 12, "_")
    for understate in (False, True):
        with torch.cuda.stream(stream):
            umi = B._DevColumn(dev, stream, rows=64, nbytes=16)
            names = B._DevColumn(dev, stream, rows=64, nbytes=16)
            sizes = [(umi.off.numel(), umi.vw.numel(), umi.val.numel())]
            keep, row = [], 0
            for c in C.APPEND_COUNTS:
                s = C.slice_batch(hb, row, row + c)
                b, t = _batch(torch, dev, s)
                keep.append(t)
                nbytes = int(s["name_off"][-1])
                bound = 0 if understate else (12 * c if source == 0 else nbytes)
                umi.append_umi(b, c, source, 12, "_", bound)
                names.append_strings(b.offsets[0], b.values[0], c, nbytes)
                sizes.append((umi.off.numel(), umi.vw.numel(), umi.val.numel()))
                row += c
            if understate:
                assert umi.val.numel() == 16
                with pytest.raises(RogtkError, match=r"\d+ rows past the value capacity"):
                    umi.finish()
                stream.synchronize()
                continue
            off, val, vw, rows = umi.finish()
            got = C.column_items(off.cpu().numpy(), val.cpu().numpy(), _u64(vw.cpu().numpy()), rows)
            words = _u64(vw.cpu().numpy())
            name_col = names.to_host_strings()
        assert rows == n and got == exp
        assert np.array_equal(words, C.pack_bits([u is not None for u in exp]))
        assert name_col.cast("binary").to_pylist() == hb["names"]
        for k in range(3):  # each buffer grew more than once
            assert len({s[k] for s in sizes}) >= 3, sizes


# ------------------------------------------------------------------ d. NULL columns
def _next_dev_raw(reader, max_records, mode, inc_seq, inc_qual, stream):
    from rogtk_amd import _lib
    from rogtk_amd import bam as B

    b = _lib.BamBatch()
    n = ctypes.c_int64()
    _lib.call("rogtk_bam_next_dev", reader._h, max_records, B.MODES[mode], inc_seq, inc_qual, ctypes.byref(n),
              ctypes.byref(b), _sp(stream))
    return int(n.value), b


@pytest.mark.parametrize("mode", C.MODES)
def test_columns_not_asked_for_are_null(torch, dev, stream, files, mode):
    """rogtk_bam_next_dev returns NULL sequence / quality columns unless asked (as
    rogtk_bam_next), so the UMI entries refuse source = sequence instead of reading up to
    umi_len bytes per row from values that were never filled. The pointers are asserted
    first: a build that still returns them fails there and never launches the read."""
    from rogtk_amd import RogtkError, _lib
    from rogtk_amd import bam as B

    with torch.cuda.stream(stream), B.BamReader(files["f"], 4) as r:
        n, b = B._next_dev(r, 100, mode, False, stream)
        assert n == 100
        assert b.offsets[2] is None and b.values[2] is None and b.validity[2] is None
        assert b.offsets[3] is None and b.values[3] is None and b.validity[3] is None
        assert b.offsets[0] and b.values[0] and b.offsets[1] and b.values[1] and b.validity[1]
        assert all(b.u32[c] for c in range(3)) and b.u32_validity[0] and b.u32_validity[1]
        off = Guarded(torch, dev, n + 1, torch.int64)
        val = Guarded(torch, dev, 12 * n, torch.uint8)
        vw = Guarded(torch, dev, 2, torch.int64, fill=0)
        base = Guarded(torch, dev, 1, torch.int64, fill=0)
        ovf = Guarded(torch, dev, 1, torch.int64, fill=0)
        with pytest.raises(RogtkError, match="no sequence column") as e:
            _lib.call("rogtk_bam_umi_dev", ctypes.byref(b), n, 0, 12, ord("_"), off.ptr, val.ptr, 12 * n, vw.ptr,
                      _sp(stream))
        assert e.value.code == _lib.ROGTK_E_INVALID
        with pytest.raises(RogtkError, match="no sequence column") as e:
            _lib.call("rogtk_bam_umi_append", ctypes.byref(b), n, 0, 12, ord("_"), off.ptr, val.ptr, 12 * n, vw.ptr, 0,
                      base.ptr, ovf.ptr, _sp(stream))
        assert e.value.code == _lib.ROGTK_E_INVALID
        stream.synchronize()
        assert (off.get() == CAN64).all() and (val.get() == CAN8).all() and (vw.get() == 0).all()
        # pointers are non-NULL only when asked, for each of the two columns
        for inc_seq, inc_qual in ((1, 1), (0, 1), (1, 0), (0, 0)):
            n, b = _next_dev_raw(r, 100, mode, inc_seq, inc_qual, stream)
            assert n == 100
            for c, inc in ((2, inc_seq), (3, inc_qual)):
                got = (bool(b.offsets[c]), bool(b.values[c]), bool(b.validity[c]))
                assert got == (bool(inc),) * 3, (inc_seq, inc_qual, c, got)
        r.check(stream)


# ------------------------------------------------------------------ e. device decode
def _d2h(ptr, dtype, count, stream):
    from rogtk_amd import _lib

    out = np.empty(count, dtype=dtype)
    if count:
        assert ptr
        _lib.call("rogtk_copy", ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(ptr), out.nbytes, _sp(stream))
    return out


def _batch_rows(b, n, include_quality, stream):
    """A device batch copied back column by column and turned into the oracle's rows."""
    words = (n + 63) // 64

    def strings(c):
        off = _d2h(b.offsets[c], np.int64, n + 1, stream)
        assert off[0] == 0 and (np.diff(off) >= 0).all()
        raw = _d2h(b.values[c], np.uint8, int(off[n]), stream).tobytes()
        valid = C.unpack_bits(_d2h(b.validity[c], np.uint64, words, stream), n) if b.validity[c] else np.ones(n, bool)
        return [raw[off[i]:off[i + 1]] if valid[i] else None for i in range(n)]

    def u32(c):
        vals = _d2h(b.u32[c], np.uint32, n, stream)
        valid = (C.unpack_bits(_d2h(b.u32_validity[c], np.uint64, words, stream), n) if b.u32_validity[c]
                 else np.ones(n, bool))
        return [int(vals[i]) if valid[i] else None for i in range(n)]

    assert b.validity[0] is None and b.u32_validity[2] is None  # name and flags are non-null
    cols = {"name": [x.decode() for x in strings(0)], "chrom": [None if x is None else x.decode() for x in strings(1)],
            "start": u32(0), "end": u32(1), "flags": u32(2), "sequence": strings(2)}
    if include_quality:
        cols["quality_scores"] = strings(3)
    return [{k: v[i] for k, v in cols.items()} for i in range(n)]


def _expect_rows(rows, include_quality):
    out = []
    for r in rows:
        r = dict(r)
        if r["sequence"] is not None:
            r["sequence"] = r["sequence"].encode()
        if not include_quality:
            del r["quality_scores"]
        out.append(r)
    return out


DECODE_CASES = [(m, q, mr, None) for m in C.MODES for q in (0, 1) for mr in (97, 1 << 20)] + [("htslib", 1, 97, "4096")]


@pytest.mark.parametrize("mode,include_quality,max_records,chunk", DECODE_CASES)
def test_device_decode_matches_oracle(torch, stream, files, monkeypatch, mode, include_quality, max_records, chunk):
    """Device-mode decode (value buffers sized from host bounds, no sync per batch) of names
    that grow 3x when lossy, "*" names, empty / IUPAC sequences, 0xFF qualities and two
    records of hundreds of BGZF blocks, in every mode, row for row against the oracle."""
    from rogtk_amd import bam as B

    if chunk:
        monkeypatch.setenv("ROGTK_BAM_CHUNK", chunk)
    ref = _expect_rows(oracle_rows(files["f"], mode), include_quality)
    got = []
    with torch.cuda.stream(stream), B.BamReader(files["f"], 4) as r:
        while True:
            n, b = _next_dev_raw(r, max_records, mode, 1, include_quality, stream)
            if n == 0:
                break
            assert n <= max_records
            batch = _batch_rows(b, n, include_quality, stream)
            # the host bounds that size the value buffers (and _DevColumn's growth) hold
            raw = r.batch_bytes()
            assert sum(len(x["name"].encode()) for x in batch) <= 3 * raw + 7 * n
            assert sum(len(x["sequence"] or b"") for x in batch) <= raw
            got += batch
        r.check(stream)
        assert r.tail() == -1
    assert len(got) == len(ref) == C.N_RECORDS + 2
    bad = [i for i in range(len(ref)) if got[i] != ref[i]]
    assert not bad, (bad[:3], {k: (got[bad[0]][k], ref[bad[0]][k]) for k in ref[bad[0]]
                               if got[bad[0]][k] != ref[bad[0]][k] and len(str(ref[bad[0]][k])) < 900})


# ------------------------------------------------------------------ f. corrupt records
def test_corrupt_records_are_an_error_not_data(torch, stream, files, tmp_path):
    """Two records whose l_seq / n_cigar_op overrun block_size: the host path fails in the
    batch, the device path decodes on (their variable fields read as empty: no load depends on
    the corrupt lengths) and fails in rogtk_bam_check; other readers are unaffected."""
    from rogtk_amd import RogtkError
    from rogtk_amd import bam as B
    from rogtk_amd import synth_bam

    recs = C.device_records(C.SEED, 300)
    recs[50] = C.corrupt(recs[50], "l_seq")
    recs[200] = C.corrupt(recs[200], "n_cigar")
    p = str(tmp_path / "corrupt.bam")
    synth_bam.write_bam(p, C.REFS, recs, text=C.TEXT, block=C.BLOCK)
    msg = r"2 record\(s\) whose fields overrun"
    for mode in C.MODES:
        with B.BamReader(p, 4) as r:
            with pytest.raises(RogtkError, match=msg):
                r.next_batch(1 << 20, mode)
    with torch.cuda.stream(stream):
        for mode in C.MODES:
            with B.BamReader(p, 4) as r:
                total = 0
                while True:
                    n, _ = B._next_dev(r, 97, mode, True, stream)  # every call returns
                    if n == 0:
                        break
                    total += n
                assert total == 300
                with pytest.raises(RogtkError, match=msg):
                    r.check(stream)
        for source in SOURCES:
            with pytest.raises(RogtkError, match=msg):
                B.bam_umis_dev(p, 12, source, "_", "htslib", 4)
        # a reader of a clean file afterwards
        (off, val, vw, n), names = B.bam_umis_dev(files["f"], 12, "name", "_", "htslib", 4, with_names=True)
        stream.synchronize()
        rows = oracle_rows(files["f"], "htslib")
        assert n == len(rows) and names.to_pylist() == [r["name"] for r in rows]
        assert C.column_items(off.cpu().numpy(), val.cpu().numpy(), _u64(vw.cpu().numpy()), n) == C.oracle_umis(
            rows, "name")


# ------------------------------------------------------------------ g. end to end
_CLUSTERS = {}


def oracle_clusters(key, umis, md):
    if (key, md) not in _CLUSTERS:
        _CLUSTERS[key, md] = P.umi_cluster(P.StrCol.from_list(umis), C.UMI_LEN, md)[:3]
    return _CLUSTERS[key, md]


def _check_table(t, rows, umis, key, md):
    assert t.num_rows == len(rows)
    assert t.column("umi").to_pylist() == [None if u is None else u.decode() for u in umis]
    assert t.column("name").to_pylist() == [r["name"] for r in rows]
    rc, rv, rk = oracle_clusters(key, umis, md)
    valid = np.array([u is not None for u in umis])
    assert np.array_equal(rv, valid)
    assert np.array_equal(np.asarray(t.column("cluster_id").is_valid()), valid)
    assert int(t.schema.metadata[b"n_clusters"]) == rk
    got = t.column("cluster_id").to_numpy(zero_copy_only=False)
    assert np.array_equal(got[valid].astype(np.uint32), rc[valid])


@pytest.mark.parametrize("md", [0, 1])
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("mode", C.MODES)
def test_bam_umi_cluster_on_edge_records(files, monkeypatch, mode, source, md):
    from rogtk_amd import bam as B

    monkeypatch.setattr(B, "DECODE_RECORDS", 97)  # 16 device batches, every bit offset
    t = B.bam_umi_cluster(files["f"], umi_len=12, max_distance=md, source=source, mode=mode)
    rows = oracle_rows(files["f"], mode)
    _check_table(t, rows, C.oracle_umis(rows, source), ("f", mode, source), md)


@pytest.mark.parametrize("md", [0, 1])
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("names,per_file", [(("f",), 5), (("f", "f2"), 3)])
def test_bams_umi_cluster_ranges_in_row_order(files, monkeypatch, names, per_file, source, md):
    """World 1: the files cut into ranges, decoded concurrently, concatenated
    (rogtk_concat_strings_dev at row counts that are no multiple of 64) and clustered; compared
    in row order (names repeat across and within the files)."""
    from rogtk_amd import bam as B

    monkeypatch.setattr(B, "DECODE_RECORDS", 97)
    paths = [files[k] for k in names]
    t = B.bams_umi_cluster(paths, umi_len=12, max_distance=md, source=source, ranges_per_file=per_file)
    rows = [r for p in paths for r in oracle_rows(p, "htslib")]
    _check_table(t, rows, C.oracle_umis(rows, source), (names, source), md)
    assert t.column("source").to_pylist() == [p for p in paths for _ in oracle_rows(p, "htslib")]


@pytest.mark.parametrize("source", SOURCES)
def test_header_only_bam_gives_an_empty_table(files, source):
    from rogtk_amd import bam as B

    for t in (B.bam_umi_cluster(files["empty"], umi_len=12, max_distance=1, source=source),
              B.bams_umi_cluster([files["empty"]], umi_len=12, max_distance=1, source=source, ranges_per_file=4)):
        assert t.num_rows == 0
        assert t.schema.metadata[b"n_clusters"] == b"0"
        assert t.column("umi").to_pylist() == [] and t.column("name").to_pylist() == []
        assert t.column("cluster_id").to_pylist() == []
