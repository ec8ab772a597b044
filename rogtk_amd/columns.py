"""What a Python wrapper hands to the C ABI: Arrow string columns as host buffers (offsets,
values, validity) and per-row integer arguments as uint32 arrays.

The reference receives polars String series (possibly multi-chunk) through the
polars plugin ABI (src/expressions.rs:1236 `inputs[0].str()?`). Here a column is
any of: pyarrow (Large)StringArray / ChunkedArray, a Python sequence of
str/bytes/None, or a numpy fixed-width bytes array ('S<L>'). Each chunk is handed
to librogtk_hip as plain host buffers, with offsets rebased to 0 for the entries that ask
for that and as Arrow holds them for the entries whose upload rebases.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Iterator, Optional, Sequence, Union

import numpy as np
import pyarrow as pa

from . import _lib

NO_ID = 0xFFFFFFFF  # the u32 id of a row that belongs nowhere (what an Arrow null becomes)
ColumnLike = Union[pa.Array, pa.ChunkedArray, Sequence[Optional[Union[str, bytes]]], np.ndarray]


@dataclass
class HostChunk:
    """One Arrow string chunk as contiguous host buffers. The numpy views keep Arrow's memory."""

    offsets: np.ndarray           # int32 or int64, n+1
    values: np.ndarray            # uint8
    validity: Optional[np.ndarray]  # uint8 bitmap (LSB order) or None
    validity_offset: int
    n: int
    arrow: pa.Array               # the source chunk (for its validity buffer / name)

    @property
    def offset_width(self) -> int:
        return self.offsets.dtype.itemsize

    def loose(self) -> tuple:
        """The column as the seven arguments of the entries that take it loose."""
        return (_lib.ptr(self.offsets), self.offset_width, _lib.ptr(self.values), self.values.size,
                _lib.ptr(self.validity), self.validity_offset, self.n)

    def desc(self) -> _lib.StrCol:
        """The column as a rogtk_str_col. It holds raw addresses, so it carries the chunk."""
        d = _lib.StrCol(*self.loose())
        d.chunk = self
        return d


def text_type(ch: HostChunk):
    """The Arrow type of a string output of the chunk: binary in, binary out."""
    t = ch.arrow.type
    return pa.large_binary() if pa.types.is_binary(t) or pa.types.is_large_binary(t) else pa.large_string()


def _to_arrow(col: ColumnLike) -> Union[pa.Array, pa.ChunkedArray]:
    if isinstance(col, (pa.Array, pa.ChunkedArray)):
        t = col.type
        if pa.types.is_string(t) or pa.types.is_large_string(t):
            return col
        if pa.types.is_binary(t) or pa.types.is_large_binary(t):
            return col
        if pa.types.is_string_view(t):
            return col.cast(pa.large_string())
        raise TypeError(f"expected a string column, got {t}")
    if isinstance(col, np.ndarray):
        if col.dtype.kind == "S":
            return pa.array(list(col), type=pa.large_binary())
        if col.dtype.kind in ("U", "O"):
            return pa.array(list(col), type=pa.large_string())
        raise TypeError(f"expected bytes/str numpy array, got {col.dtype}")
    items = list(col)
    if any(isinstance(x, (bytes, bytearray)) for x in items):
        return pa.array([None if x is None else bytes(x) for x in items], type=pa.large_binary())
    return pa.array(items, type=pa.large_string())


def chunks(col: ColumnLike) -> Iterator[HostChunk]:
    arr = _to_arrow(col)
    parts = arr.chunks if isinstance(arr, pa.ChunkedArray) else [arr]
    for a in parts:
        yield _chunk(a)


def one_chunk(col: ColumnLike, rebase: bool = True) -> HostChunk:
    """The column as one batch: what a call whose answer is global to the column takes."""
    arr = _to_arrow(col)
    if isinstance(arr, pa.ChunkedArray):
        if arr.num_chunks == 1:
            arr = arr.chunk(0)
        else:
            arr = arr.combine_chunks() if arr.num_chunks else pa.array([], type=arr.type)
    return _chunk(arr, rebase)


def _chunk(a: pa.Array, rebase: bool = True) -> HostChunk:
    """rebase: offsets from 0 over the chunk's own bytes (a copy of the offsets for a slice). Not
    rebase: Arrow's offsets from a.offset on and the whole values buffer, for the entries whose
    upload rebases; no pass over the offsets."""
    n = len(a)
    validity_buf, offsets_buf, values_buf = a.buffers()[:3]
    wide = pa.types.is_large_string(a.type) or pa.types.is_large_binary(a.type)
    odt = np.int64 if wide else np.int32
    if offsets_buf is not None:
        offs = np.frombuffer(offsets_buf, dtype=odt, count=a.offset + n + 1)[a.offset:]
    else:
        offs = np.zeros(n + 1, dtype=odt)
    values = np.zeros(1, dtype=np.uint8)
    if not rebase:
        if values_buf is not None and values_buf.size:
            values = np.frombuffer(values_buf, dtype=np.uint8)
    else:
        base, end = int(offs[0]), int(offs[-1])
        if values_buf is not None and end > base:
            values = np.frombuffer(values_buf, dtype=np.uint8, count=end)[base:end]
        if base:
            offs = np.ascontiguousarray(offs - base, dtype=odt)
    validity = None
    voff = 0
    if a.null_count > 0 and validity_buf is not None:
        validity = np.frombuffer(validity_buf, dtype=np.uint8)
        voff = a.offset
    return HostChunk(offs, values, validity, voff, n, a)


def as_u32(x, name: str, *, rows: Optional[int] = None, nulls_to: Optional[int] = None) -> np.ndarray:
    """A per-row integer argument (numpy, Arrow or chunked Arrow) as a contiguous uint32 array,
    x's own memory when it already is one. Anything that is not `rows` integers in 0..2^32-1 is
    a ValueError, in this order: type, nulls (filled with nulls_to when given), shape, range."""
    if isinstance(x, pa.ChunkedArray):
        x = x.combine_chunks() if x.num_chunks else pa.array([], type=x.type)
    if isinstance(x, pa.Array):
        if not pa.types.is_integer(x.type):
            raise ValueError(f"{name} must be an integer array, got {x.type}")
        if x.null_count:
            if nulls_to is None:
                raise ValueError(f"{name} has {x.null_count} nulls")
            x = (x if pa.types.is_uint64(x.type) else x.cast(pa.int64())).fill_null(nulls_to)
        x = x.to_numpy(zero_copy_only=False)
    a = np.asarray(x)
    if a.dtype.kind not in "iu" and (a.size or isinstance(x, np.ndarray)):  # a sequence without items has no type
        raise ValueError(f"{name} must be an integer array, got dtype {a.dtype}")
    if a.ndim != 1:
        raise ValueError(f"{name} must be 1-D, got shape {a.shape}")
    if rows is not None and a.size != rows:
        raise ValueError(f"{name} has shape {a.shape}, expected ({rows},)")
    if a.size and (int(a.min()) < 0 or int(a.max()) > 0xFFFFFFFF):
        raise ValueError(f"{name} must hold values in 0..2^32-1")
    return np.ascontiguousarray(a, dtype=np.uint32)


def largest_plus_one(x) -> int:
    """1 + the largest value other than 0xFFFFFFFF of a u32 column (numpy array or tensor); 0 if none."""
    if is_tensor(x):
        import torch

        x = x.view(torch.int32).to(torch.int64) & NO_ID
    real = x[x != NO_ID]
    return int(real.max()) + 1 if len(real) else 0


def is_tensor(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


def u32_tensor(t, name: str, like=None, like_name: str = "") -> None:
    """A u32 column on a device: a 1-D contiguous int32 / uint32 torch tensor holding the u32 bits,
    and, beside the call's first tensor `like`, on its device with its length. Else a ValueError."""
    import torch

    if not is_tensor(t):
        raise ValueError(f"{name} must be a torch tensor, as {like_name} is")
    if t.dim() != 1:
        raise ValueError(f"{name} must be 1-D, got shape {tuple(t.shape)}")
    if t.dtype not in (torch.int32, torch.uint32) or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous int32 / uint32 device tensor (the u32 bits)")
    if like is not None and t.device != like.device:
        raise ValueError(f"{name} is on {t.device}, {like_name} on {like.device}")
    if like is not None and t.numel() != like.numel():
        raise ValueError(f"{name} has {t.numel()} rows, {like_name} has {like.numel()}")


def dev_ptr(t):
    """A device tensor (or None) as a pointer argument; NULL for an empty one."""
    return None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())


def device_temp(entry: str, *sizes, device):
    """The temp buffer of a Level-1 call, sized by its *_temp_bytes entry: a uint8 tensor."""
    import torch

    tb = ctypes.c_int64(0)
    _lib.call(entry, *sizes, ctypes.byref(tb))
    return torch.empty(tb.value, dtype=torch.uint8, device=device)


def current_stream() -> ctypes.c_void_p:
    import torch

    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def validity_buffer(chunk: HostChunk) -> Optional[pa.Buffer]:
    """Validity bitmap for an output of `chunk` (null in -> null out), offset 0."""
    if chunk.validity is None:
        return None
    bits = np.unpackbits(chunk.validity, bitorder="little")[chunk.validity_offset:chunk.validity_offset + chunk.n]
    return pa.py_buffer(np.packbits(bits, bitorder="little"))


def concat(arrays, typ):
    if not arrays:
        return pa.array([], type=typ)
    if len(arrays) == 1:
        return arrays[0]
    return pa.chunked_array(arrays, type=typ)
