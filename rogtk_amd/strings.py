"""Element-wise DNA / CIGAR / PHRED string expressions on the GPU.

Mirrors the reference's Python surface (rogtk/__init__.py) on pyarrow columns:

    rogtk/__init__.py:57-69     DnaNamespace.reverse_complement  -> reverse_complement_series
    rogtk/__init__.py:72-80     parse_cigar(expr, block_dels)    -> parse_cigar_series
    rogtk/__init__.py:82-90     phred_to_numeric_str(expr, base) -> phred_to_numeric_series_str
    src/expressions.rs:598-630  phred_to_numeric_series (List[u8]; not registered in Python)
    rogtk/__init__.py:532-658   CigarNamespace.enrich_insertions / align_to_ref / align_to_query
    rogtk/__init__.py:661-696   extract_cigar_insertions(seq_col, cigar_col)
    rogtk/__init__.py:351-410   FuzzyExpr.match / replace_target / contains / replace
                                -> fuzzy_*_expr (rogtk_amd/csrc/fuzzy.hip, wave per row)

Every call runs rogtk_str_transform_host (rogtk_amd/csrc/strings.hip): a measuring
and a filling kernel over the rows, thread per row. There is no CPU path.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional

import numpy as np
import pyarrow as pa

from . import _lib
from .columns import ColumnLike, one_chunk

REVCOMP, PARSE_CIGAR, ALIGNED_REF, ALIGNED_QUERY, CIGAR_INSERTIONS, ENRICH_ALLELE, PHRED_STR, PHRED_LIST = range(1, 9)


def _run(op: int, cols: List[ColumnLike], param: int = 0) -> _lib.StrResult:
    """rogtk_str_transform_host over the columns. Rows of the output: the reference zips its
    inputs (the shortest wins); the aligned expressions broadcast a 1-row reference next to a
    longer query column (expressions.rs:344-349)."""
    chs = [one_chunk(c, rebase=False) for c in cols]
    lens = [ch.n for ch in chs]
    scalar_ref = op in (ALIGNED_REF, ALIGNED_QUERY) and lens[0] == 1 and lens[1] > 1
    n = min(lens[1:]) if scalar_ref else min(lens)
    chs = [ch if ch.n == n or (scalar_ref and i == 0) else one_chunk(ch.arrow.slice(0, n), rebase=False)
           for i, ch in enumerate(chs)]
    descs = (_lib.StrCol * len(chs))(*[ch.desc() for ch in chs])
    res = _lib.StrResult()
    _lib.check(_lib.hip().rogtk_str_transform_host(op, descs, len(chs), n, int(param), ctypes.byref(res)))
    return res


def _transform(op: int, cols: List[ColumnLike], param: int = 0):
    """The output's raw buffers: (n, offsets, values, validity bytes, null_count)."""
    return _lib.take_str_buffers(_run(op, cols, param))


def reverse_complement(column: ColumnLike) -> pa.Array:
    """reverse_complement_series (expressions.rs:957-977): chars reversed, A<->T, C<->G."""
    return _lib.take_str(_run(REVCOMP, [column]))


def parse_cigar(column: ColumnLike, block_dels: bool = False) -> pa.Array:
    """parse_cigar_series (expressions.rs:450-505): "D,pos,len|I,pos,len|..."."""
    return _lib.take_str(_run(PARSE_CIGAR, [column], int(bool(block_dels))))


def phred_to_numeric_str(column: ColumnLike, base: int = 33) -> pa.Array:
    """phred_to_numeric_series_str (expressions.rs:632-665): "q1|q2|..."."""
    return _lib.take_str(_run(PHRED_STR, [column], base))


def phred_to_numeric(column: ColumnLike, base: int = 33) -> pa.Array:
    """phred_to_numeric_series (expressions.rs:598-630): List[UInt8]; rows of null
    strings are skipped by the reference's `for_each`, so the output is shorter."""
    n, offs, vals, bits, nulls = _transform(PHRED_LIST, [column], base)
    keep = np.unpackbits(bits, bitorder="little")[:n].astype(bool)
    lens = np.diff(offs)[keep]
    starts = offs[:-1][keep]
    idx = np.concatenate([np.arange(s, s + l) for s, l in zip(starts, lens)]) if len(lens) else np.zeros(0, np.int64)
    loffs = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=loffs[1:])
    return pa.LargeListArray.from_arrays(pa.array(loffs), pa.array(vals[idx.astype(np.int64)], type=pa.uint8()))


def extract_cigar_insertions(seq_col: ColumnLike, cigar_col: ColumnLike) -> pa.Array:
    """extract_cigar_insertions_expr (expressions.rs:207-251): "pos:SEQ|..." sorted by pos."""
    return _lib.take_str(_run(CIGAR_INSERTIONS, [seq_col, cigar_col]))


class DnaNamespace:
    """rogtk/__init__.py:57-69 (`pl.col(..).dna.*`)."""

    def __init__(self, column: ColumnLike):
        self._c = column

    def reverse_complement(self):
        return reverse_complement(self._c)


class CigarNamespace:
    """rogtk/__init__.py:532-658 (`pl.col(..).cigar.*`); the column is the allele (enrich)
    or the reference sequence (align_to_*), which may be a 1-row scalar."""

    def __init__(self, column: ColumnLike):
        self._c = column

    def enrich_insertions(self, seq_col: ColumnLike, cigar_col: ColumnLike):
        """enrich_allele_insertions_expr (expressions.rs:172-205): [pos:NI] -> [pos:NI:SEQ]."""
        return _lib.take_str(_run(ENRICH_ALLELE, [self._c, seq_col, cigar_col]))

    def align_to_ref(self, query_col: ColumnLike, cigar_col: ColumnLike):
        """cigar_aligned_ref_expr (expressions.rs:338-394)."""
        return _lib.take_str(_run(ALIGNED_REF, [self._c, query_col, cigar_col]))

    def align_to_query(self, query_col: ColumnLike, cigar_col: ColumnLike):
        """cigar_aligned_query_expr (expressions.rs:396-444)."""
        return _lib.take_str(_run(ALIGNED_QUERY, [self._c, query_col, cigar_col]))


# ------------------------------------------------------------------ fuzzy
class FuzzyProgram:
    """A compiled fuzzy pattern (rogtk_fuzzy_program, include/rogtk_hip.h): an ordered list of
    alternatives over literal bytes, "." and an optional ".". Compiling and ``describe`` need
    no GPU; a pattern outside the supported grammar raises RogtkError (ROGTK_E_UNSUPPORTED)."""

    def __init__(self, handle):
        self._h = handle

    @staticmethod
    def _bytes(s) -> bytes:
        return s.encode("utf-8") if isinstance(s, str) else bytes(s)

    @classmethod
    def native(cls, target, wildcard: Optional[str] = None, include_original: Optional[bool] = None,
               max_length: Optional[int] = None) -> "FuzzyProgram":
        """generate_fuzzy_pattern (expressions.rs:983-1013); None = the reference's default."""
        t = cls._bytes(target)
        h = ctypes.c_void_p()
        _lib.call("rogtk_fuzzy_compile_native", t, len(t), cls._bytes(".{0,1}" if wildcard is None else wildcard),
                  1 if include_original is None else int(bool(include_original)),
                  100 if max_length is None else int(max_length), ctypes.byref(h))
        return cls(h)

    @classmethod
    def pattern(cls, pattern, literal: Optional[bool] = None) -> "FuzzyProgram":
        p = cls._bytes(pattern)
        h = ctypes.c_void_p()
        _lib.call("rogtk_fuzzy_compile_pattern", p, len(p), int(bool(literal)), ctypes.byref(h))
        return cls(h)

    @property
    def handle(self) -> ctypes.c_void_p:
        return self._h

    def set_replacement(self, replacement) -> "FuzzyProgram":
        r = self._bytes(replacement)
        _lib.call("rogtk_fuzzy_set_replacement", self._h, r, len(r))
        return self

    def describe(self) -> str:
        """The alternatives joined by '|': literal bytes, '.' (any), '?' (optional any)."""
        need = ctypes.c_int64(0)
        rc = _lib.hip().rogtk_fuzzy_describe(self._h, None, 0, ctypes.byref(need))
        if rc not in (_lib.ROGTK_OK, _lib.ROGTK_E_OVERFLOW):
            _lib.check(rc)
        buf = ctypes.create_string_buffer(max(int(need.value), 1))
        _lib.call("rogtk_fuzzy_describe", self._h, buf, int(need.value), ctypes.byref(need))
        return buf.raw[: need.value].decode("utf-8", "replace")

    def contains(self, column: ColumnLike) -> pa.Array:
        ch = one_chunk(column, rebase=False)
        n = ch.n
        d = ch.desc()
        bits = np.zeros(max((n + 63) // 64, 1), dtype=np.uint64)
        vbits = np.zeros_like(bits)
        _lib.call("rogtk_fuzzy_contains_host", self._h, ctypes.byref(d), _lib.ptr(bits), _lib.ptr(vbits))
        nulls = ch.arrow.null_count
        return pa.Array.from_buffers(pa.bool_(), n, [pa.py_buffer(vbits) if nulls else None, pa.py_buffer(bits)],
                                     null_count=nulls)

    def replace(self, column: ColumnLike, replace_all: bool) -> pa.Array:
        d = one_chunk(column, rebase=False).desc()
        res = _lib.StrResult()
        _lib.call("rogtk_fuzzy_replace_host", self._h, ctypes.byref(d), int(bool(replace_all)), ctypes.byref(res))
        return _lib.take_str(res)

    def close(self) -> None:
        if self._h is not None and self._h.value:
            _lib.hip().rogtk_fuzzy_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FuzzyNamespace:
    """rogtk/__init__.py:351-410 (`pl.col(..).fuzzy.*`). ``match`` / ``contains`` return a
    BooleanArray, the replace methods a large_string array; null in, null out."""

    def __init__(self, column: ColumnLike):
        self._c = column

    def replace(self, pattern: str, replacement: str, literal: bool = False):
        """fuzzy_replace_expr (expressions.rs:1104-1129): every match (Regex::replace_all / str::replace)."""
        return FuzzyProgram.pattern(pattern, literal).set_replacement(replacement).replace(self._c, True)

    def contains(self, pattern: str, literal: bool = False):
        """fuzzy_contains_expr (expressions.rs:1131-1162)."""
        return FuzzyProgram.pattern(pattern, literal).contains(self._c)

    def match(self, target: str, wildcard: str = ".{0,1}", include_original: bool = True, max_length: int = 100):
        """fuzzy_contains_native_expr (expressions.rs:1164-1188)."""
        return FuzzyProgram.native(target, wildcard, include_original, max_length).contains(self._c)

    def replace_target(self, target: str, replacement: str, wildcard: str = ".{0,1}", include_original: bool = True,
                       max_length: int = 100, replace_all: bool = False):
        """fuzzy_replace_native_expr (expressions.rs:1190-1216)."""
        prog = FuzzyProgram.native(target, wildcard, include_original, max_length).set_replacement(replacement)
        return prog.replace(self._c, bool(replace_all))
