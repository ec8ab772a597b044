"""Cell-barcode correction against a whitelist.

Observed barcodes are mapped onto a known whitelist at one mismatch, on the GPU
(rogtk_amd/csrc/barcode.hip), before anything is grouped by cell. The answer is one
dense u32 per row, the whitelist index, which is what ``groups=`` of the UMI calls takes.
The reference has no counterpart.

    wl = rg.BarcodeWhitelist(whitelist)           # built once, reused across batches
    res = wl.correct(batch["cbc"])                # ambiguous="counts" (default) or "reject"
    res.index           # pa.UInt32Array, null where the row is neither exact nor corrected
    res.status          # numpy u8: 0 exact, 1 corrected, 2 ambiguous, 3 no_match, 4 null
    res.corrected       # the whitelist string, null otherwise
    res.exact_counts    # numpy u32 [W]: exact rows per entry
    res.counts          # numpy u32 [W]: exact or corrected rows per entry
    res.totals          # rows per status
    rg.umi_correct(batch["umi"], 12, method="directional", groups=res.keys)
    total = wl.count(b1); wl.count(b2, into=total)        # a file in batches: count first,
    wl.correct(b1, counts=total)                          # correct second
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import pyarrow as pa

from . import _lib
from .columns import ColumnLike, as_u32, one_chunk, text_type

STATUS = ("exact", "corrected", "ambiguous", "no_match", "null")
AMBIGUOUS = ("counts", "reject")
NO_INDEX = 0xFFFFFFFF
MAX_LEN = 32


@dataclass
class BarcodeCorrection:
    index: pa.Array
    status: np.ndarray
    corrected: pa.Array
    exact_counts: np.ndarray
    counts: np.ndarray
    totals: Dict[str, int]

    @property
    def keys(self) -> np.ndarray:
        """``index`` as plain uint32 with 0xFFFFFFFF where it is null: the ``groups=`` of the UMI calls."""
        return np.asarray(self.index.fill_null(NO_INDEX).to_numpy(zero_copy_only=False), dtype=np.uint32)


def validate_whitelist(ch) -> int:
    """The whitelist rules of DESIGN.md §4e over one host chunk; returns L. A ValueError names
    the first offending row. No library call."""
    W = ch.n
    if W < 1:
        raise ValueError("barcode whitelist: empty")
    if W >= 2**32 - 1:
        raise ValueError(f"barcode whitelist: {W} rows, at most 2^32 - 2")
    if ch.arrow.null_count:
        row = int(np.flatnonzero(~np.asarray(ch.arrow.is_valid().to_numpy(zero_copy_only=False), dtype=bool))[0])
        raise ValueError(f"barcode whitelist: row {row} is null")
    offs = ch.offsets.astype(np.int64)
    lens = np.diff(offs)
    L = int(lens[0])
    if not 1 <= L <= MAX_LEN:
        raise ValueError(f"barcode whitelist: row 0 has {L} bytes, outside 1..{MAX_LEN}")
    odd = np.flatnonzero(lens != L)
    if odd.size:
        raise ValueError(f"barcode whitelist: row {int(odd[0])} has {int(lens[odd[0]])} bytes, row 0 has {L}")
    rows = ch.values[:W * L].reshape(W, L)
    lut = np.full(256, 255, dtype=np.uint8)
    lut[np.frombuffer(b"ACGT", np.uint8)] = np.arange(4, dtype=np.uint8)
    digits = lut[rows]
    bad = np.flatnonzero((digits == 255).any(axis=1))
    if bad.size:
        r = int(bad[0])
        j = int(np.flatnonzero(digits[r] == 255)[0])
        raise ValueError(f"barcode whitelist: row {r} has byte 0x{int(rows[r, j]):02x} at position {j} (only ACGT)")
    codes = np.zeros(W, dtype=np.uint64)
    for j in range(L):
        codes = (codes << np.uint64(2)) | digits[:, j].astype(np.uint64)
    order = np.argsort(codes, kind="stable")
    same = np.flatnonzero(codes[order][1:] == codes[order][:-1])
    if same.size:
        raise ValueError(f"barcode whitelist: row {int(order[same + 1].min())} repeats an earlier barcode")
    return L


def _ambiguous(ambiguous: str) -> int:
    if ambiguous not in AMBIGUOUS:
        raise ValueError(f"ambiguous must be one of {AMBIGUOUS}, got {ambiguous!r}")
    return AMBIGUOUS.index(ambiguous)


class BarcodeWhitelist:
    """The device handle of a whitelist: immutable, bound to the device current at creation,
    reusable across calls and batches. whitelist: Arrow, numpy or a list of str / bytes; its
    row number is the barcode's index."""

    def __init__(self, whitelist: ColumnLike):
        ch = one_chunk(whitelist)
        self.barcode_len = validate_whitelist(ch)
        self.size = ch.n
        self._h = ctypes.c_void_p(None)
        desc = ch.desc()
        _lib.check(_lib.hip().rogtk_barcode_whitelist_create(ctypes.byref(desc), ctypes.byref(self._h)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                _lib.hip().rogtk_barcode_whitelist_free(h)
            except Exception:  # interpreter shutdown: the library may be gone already
                pass
            h.value = None

    def __len__(self) -> int:
        return self.size

    @property
    def handle(self) -> ctypes.c_void_p:
        """The C handle (rogtk_barcode_correct_dev / rogtk_barcode_count_dev)."""
        return self._h

    def info(self) -> Dict[str, int]:
        W, dev = ctypes.c_int64(0), ctypes.c_int64(0)
        L, P = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(_lib.hip().rogtk_barcode_whitelist_info(self._h, ctypes.byref(W), ctypes.byref(L), ctypes.byref(P),
                                                           ctypes.byref(dev)))
        return {"W": int(W.value), "L": int(L.value), "prefix_digits": int(P.value), "device_bytes": int(dev.value)}

    def correct(self, column: ColumnLike, ambiguous: str = "counts", counts=None) -> BarcodeCorrection:
        """Every row against the whitelist. A multi-chunk column is one batch.
        counts (u32 [W], optional): the prior counts under ambiguous="counts"; default: the
        exact rows of this call."""
        amb = _ambiguous(ambiguous)
        prior = None if counts is None else as_u32(counts, "counts", rows=self.size)
        ch = one_chunk(column)
        n, W = ch.n, self.size
        index = np.zeros(max(n, 1), dtype=np.uint32)
        status = np.zeros(max(n, 1), dtype=np.uint8)
        exact, final = np.zeros(W, dtype=np.uint32), np.zeros(W, dtype=np.uint32)
        totals = (ctypes.c_int64 * 5)()
        corrected = _lib.StrResult()
        desc, p = ch.desc(), _lib.ptr
        _lib.call("rogtk_barcode_correct_host", self._h, ctypes.byref(desc), amb, p(prior), p(index), p(status),
                  ctypes.byref(corrected), p(exact), p(final), totals)
        out = _lib.take_str(corrected, text_type(ch))
        index, status = index[:n], status[:n]
        idx = pa.array(index, type=pa.uint32(), mask=status > 1) if n else pa.array([], type=pa.uint32())
        return BarcodeCorrection(idx, status, out, exact, final, {k: int(totals[i]) for i, k in enumerate(STATUS)})

    def correct_device(self, offsets, values, validity=None, ambiguous: str = "counts", counts=None):
        """The same over a device column, torch tensors in and out (rogtk_barcode_correct_dev):
        offsets int64 [n + 1] from 0, values uint8, validity uint8 LSB bits or None, counts int32
        [W] holding the u32 bits or None. Returns (index, status, exact_counts, counts, totals);
        index and the two count tensors are int32 holding the u32 bits. Synchronises the current
        stream."""
        import torch

        amb = _ambiguous(ambiguous)
        n, W = int(offsets.numel()) - 1, self.size
        if counts is not None and (counts.dtype != torch.int32 or tuple(counts.shape) != (W,)):
            raise ValueError(f"counts must be an int32 device tensor of {W} entries (the u32 bits)")
        dev = values.device
        index = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        exact = torch.empty(W, dtype=torch.int32, device=dev)
        final = torch.empty(W, dtype=torch.int32, device=dev)
        totals = (ctypes.c_int64 * 5)()
        p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        _lib.check(_lib.hip().rogtk_barcode_correct_dev(
            self._h, p(offsets), p(values), p(validity), n, amb, p(counts), p(index), p(status), p(exact), p(final),
            totals, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return index[:n], status[:n], exact, final, {k: int(totals[i]) for i, k in enumerate(STATUS)}

    def count(self, column: ColumnLike, into: Optional[np.ndarray] = None) -> np.ndarray:
        """The exact rows of every entry (the exact pass alone), added into ``into`` (u32 [W],
        in place) when given. A file read in batches is counted first and corrected second."""
        if into is None:
            into = np.zeros(self.size, dtype=np.uint32)
        elif not (isinstance(into, np.ndarray) and into.dtype == np.uint32 and into.shape == (self.size,)
                  and into.flags.c_contiguous and into.flags.writeable):
            raise ValueError(f"into must be a writable contiguous uint32 array of {self.size} entries")
        desc = one_chunk(column).desc()
        _lib.call("rogtk_barcode_count_host", self._h, ctypes.byref(desc), _lib.ptr(into), None)
        return into


def barcode_correct(column: ColumnLike, whitelist, ambiguous: str = "counts", counts=None) -> BarcodeCorrection:
    """``BarcodeWhitelist(whitelist).correct(column, ...)``; whitelist may be a BarcodeWhitelist."""
    _ambiguous(ambiguous)
    wl = whitelist if isinstance(whitelist, BarcodeWhitelist) else BarcodeWhitelist(whitelist)
    return wl.correct(column, ambiguous, counts)


class BarcodeNamespace:
    """``rg.col(c).barcode``."""

    def __init__(self, column: ColumnLike):
        self._c = column

    def correct(self, whitelist, ambiguous: str = "counts", counts=None):
        """The corrected column alone."""
        return barcode_correct(self._c, whitelist, ambiguous, counts).corrected
