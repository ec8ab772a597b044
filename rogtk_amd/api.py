"""Host-side mirror of rogtk's UMI/Hamming expression API, backed by librogtk_hip.

Reference surface (rogtk/__init__.py) and what each call here replaces:

================================================  ==========================================
reference                                          rogtk_amd
================================================  ==========================================
``pl.col(c).umi.complexity_all()`` (:417)          ``col(c).umi.complexity_all()``
``.umi.all_scores()`` (:426)                       ``col(c).umi.all_scores()``
``.umi.shannon_entropy()`` … ``.dust_score()``     ``col(c).umi.<same name>()``
(:430-491)
``umi_complexity_scores(expr)`` (:493)             ``umi_complexity_scores(c)``
``pl.col(c).hamming.distance(target)`` (:331)      ``col(c).hamming.distance(target)``
``pl.col(c).hamming.within(target, 1)`` (:341)     ``col(c).hamming.within(target, 1)``
``df.group_by('umi')`` (caller, :206-214)          ``umi_cluster(c, max_distance=0|1)``
(no counterpart: group_by + mode on the host)      ``umi_correct(c)``, ``col(c).umi.correct()``
k-mer front end of ``assemble_sequences*`` per     ``kmer_spectrum(c, k, min_coverage,
group (fracture.rs:105-256, debruijn                auto_k, group_offsets)``
filter_kmers)
================================================  ==========================================

polars is not part of this build's image, so an "expression" is evaluated eagerly
on an Arrow column (any pyarrow string array / chunked array, a list of
str/None, or a numpy bytes array). Results are pyarrow arrays with the
reference's dtypes, field names and null propagation (null in -> null out):
Struct{shannon_entropy f64, linguistic_complexity f64, homopolymer_fraction f64,
dinucleotide_entropy f64, longest_homopolymer_run u32, dust_score f64,
combined_score f64} (src/expressions.rs:1219-1232), UInt32 (hamming distance,
u32::MAX on byte-length mismatch) and Boolean (within).

All computation runs in librogtk_hip.so on the GPU; errors are RogtkError.
"""
from __future__ import annotations

import ctypes
from typing import Union

import numpy as np
import pyarrow as pa

from . import _lib
from .columns import ColumnLike, as_u32, chunks, concat, one_chunk, validity_buffer

FIELDS = (
    ("shannon_entropy", pa.float64()),
    ("linguistic_complexity", pa.float64()),
    ("homopolymer_fraction", pa.float64()),
    ("dinucleotide_entropy", pa.float64()),
    ("longest_homopolymer_run", pa.uint32()),
    ("dust_score", pa.float64()),
    ("combined_score", pa.float64()),
)
_FIELD_NAMES = tuple(f for f, _ in FIELDS)
STRUCT_TYPE = pa.struct([pa.field(n, t) for n, t in FIELDS])


class _PinnedBlock:
    """A rogtk_host_alloc block (pinned host memory: direct DMA for the D2H of results),
    returned to the library's cache when the last array over it is collected."""

    def __init__(self, nbytes: int):
        p = ctypes.c_void_p()
        _lib.call("rogtk_host_alloc", nbytes, ctypes.byref(p))
        self.ptr, self.nbytes = p.value, nbytes

    def __del__(self):
        try:
            _lib.hip().rogtk_host_free(ctypes.c_void_p(self.ptr))
        except Exception:
            pass


def _out(n: int, dtype, zero: bool = False) -> np.ndarray:
    """Output array of n elements in pinned host memory (numpy views keep it alive)."""
    nbytes = max(n, 1) * np.dtype(dtype).itemsize
    blk = _PinnedBlock(nbytes)
    a = np.frombuffer(pa.foreign_buffer(blk.ptr, nbytes, base=blk), dtype=dtype)
    if zero:
        a[:] = 0
    return a


def _complexity_chunk(ch, want: tuple):
    n = ch.n
    out = {}
    for name, typ in FIELDS:
        if name in want:
            out[name] = _out(n, np.uint32 if name == "longest_homopolymer_run" else np.float64)
    sc = _lib.UmiScores(*[_lib.ptr(out.get(name)) for name in _FIELD_NAMES])
    _lib.call("rogtk_umi_complexity_host", *ch.loose(), ctypes.byref(sc))
    return {k: a[:n] for k, a in out.items()}


def _field_array(name, typ, values, vbuf, n):
    return pa.Array.from_buffers(typ, n, [vbuf, pa.py_buffer(np.ascontiguousarray(values))])


def umi_complexity(column: ColumnLike, fields=_FIELD_NAMES):
    """All (or the selected) complexity fields. Returns {name: pa.Array}."""
    want = tuple(fields)
    parts = {name: [] for name in want}
    for ch in chunks(column):
        res = _complexity_chunk(ch, want)
        vbuf = validity_buffer(ch)
        for name, typ in FIELDS:
            if name in want:
                parts[name].append(_field_array(name, typ, res[name], vbuf, ch.n))
    return {name: concat(parts[name], dict(FIELDS)[name]) for name in want}


def umi_complexity_scores(column: ColumnLike) -> Union[pa.StructArray, pa.ChunkedArray]:
    """umi_complexity_all_expr (src/expressions.rs:1234-1284) as a StructArray."""
    arrays = []
    for ch in chunks(column):
        res = _complexity_chunk(ch, _FIELD_NAMES)
        vbuf = validity_buffer(ch)
        children = [_field_array(name, typ, res[name], vbuf, ch.n) for name, typ in FIELDS]
        # df.into_struct (expressions.rs:1283): struct rows stay valid, a null UMI gives
        # a row whose seven fields are null (:1258-1266)
        arrays.append(pa.StructArray.from_arrays(children, fields=list(STRUCT_TYPE)))
    return concat(arrays, STRUCT_TYPE)


def hamming_distance(column: ColumnLike, target: Union[str, bytes]):
    """hamming_distance_expr (src/expressions.rs:1048-1073): UInt32, u32::MAX on length mismatch."""
    return _hamming(column, target, None, want_dist=True)


def hamming_within(column: ColumnLike, target: Union[str, bytes], max_distance: int = 1):
    """hamming_within_expr (src/expressions.rs:1075-1101): Boolean, default max_distance 1."""
    return _hamming(column, target, max_distance, want_dist=False)


def _hamming(column, target, max_distance, want_dist):
    if target is None:
        raise TypeError("target is required")  # HammingKwargs.target: String (expressions.rs:1018)
    t = target.encode("utf-8") if isinstance(target, str) else bytes(target)
    tb = np.frombuffer(t, dtype=np.uint8) if t else np.zeros(1, np.uint8)
    maxd = 1 if max_distance is None else int(max_distance)
    if maxd < 0 or maxd > 0xFFFFFFFF:
        raise ValueError("max_distance must fit in u32")
    arrays = []
    for ch in chunks(column):
        n = ch.n
        dist = _out(n, np.uint32) if want_dist else None
        bits = None if want_dist else _out((n + 7) // 8, np.uint8)
        _lib.call("rogtk_hamming_host", *ch.loose(), _lib.ptr(tb), len(t), maxd, _lib.ptr(dist), _lib.ptr(bits))
        vbuf = validity_buffer(ch)
        if want_dist:
            arrays.append(pa.Array.from_buffers(pa.uint32(), n, [vbuf, pa.py_buffer(dist)]))
        else:
            arrays.append(pa.Array.from_buffers(pa.bool_(), n, [vbuf, pa.py_buffer(bits)]))
    return concat(arrays, pa.uint32() if want_dist else pa.bool_())


UMI_METHODS = ("cluster", "directional")


def umi_method_entry(method: str, max_distance: int, cluster_entry: str, directional_entry: str) -> str:
    """The C entry point of ``method``; any other string is a ValueError. The
    directional entries' max_distance error is raised here, before any buffer is allocated."""
    if method not in UMI_METHODS:
        raise ValueError(f"method must be one of {UMI_METHODS}, got {method!r}")
    if method == "cluster":
        return cluster_entry
    if int(max_distance) not in (0, 1):
        raise _lib.RogtkError(_lib.ROGTK_E_UNSUPPORTED, f"max_distance {max_distance}: only 0 and 1 are supported")
    return directional_entry


def grouped_method(method: str, max_distance: int) -> int:
    """The C ``method`` of a grouped call (0 cluster, 1 directional); what the library would
    refuse is refused here, before any buffer is allocated."""
    if method not in UMI_METHODS:
        raise ValueError(f"method must be one of {UMI_METHODS}, got {method!r}")
    if int(max_distance) not in (0, 1):
        raise _lib.RogtkError(_lib.ROGTK_E_UNSUPPORTED, f"max_distance {max_distance}: only 0 and 1 are supported")
    if method == "cluster" and int(max_distance) == 1:
        raise _lib.RogtkError(_lib.ROGTK_E_UNSUPPORTED,
                              'method="cluster" with max_distance 1 is not supported within groups; '
                              'use method="directional"')
    return UMI_METHODS.index(method)


def umi_cluster(column: ColumnLike, umi_len: int = 0, max_distance: int = 1, method: str = "cluster", groups=None):
    """H3 cluster id per row: dense ids, exact (0) or Hamming<=1 components (1).
    method="directional": the count-aware rule at one edit; an abundant UMI
    absorbs a neighbour only when count(abundant) >= 2 * count(neighbour) - 1.
    groups (one unsigned 32-bit key per row): rows cluster only with rows of
    the same key; method="directional" at max_distance 0 or 1, method="cluster" at 0.

    Returns (pa.UInt32Array with nulls for null rows, n_clusters, resolved umi_len).
    A multi-chunk column is clustered as one batch (ids are global to the column).
    """
    if groups is not None:
        entry, m = "rogtk_umi_cluster_grouped_host", grouped_method(method, max_distance)
    else:
        entry = umi_method_entry(method, max_distance, "rogtk_umi_cluster_host", "rogtk_umi_cluster_directional_host")
    ch = one_chunk(column)
    n = ch.n
    cid = _out(n, np.uint32)
    nclu, rl = ctypes.c_int64(0), ctypes.c_int(0)
    rule = [int(umi_len), int(max_distance)]
    tail = []
    if groups is not None:  # the keys before the rule, the method in it; the clusters' keys are not asked for
        keys = as_u32(groups, "groups", rows=n)
        rule = [_lib.ptr(keys, null_if_empty=True), rule[0], m, rule[1]]
        tail = [None]
    _lib.call(entry, *ch.loose(), *rule, _lib.ptr(cid), ctypes.byref(nclu), ctypes.byref(rl), *tail)
    out = pa.Array.from_buffers(pa.uint32(), n, [validity_buffer(ch), pa.py_buffer(cid)])
    return out, int(nclu.value), int(rl.value)


KMER_STATS = ("k_eff", "n_sequences", "node_count", "terminal_count", "isolated_count")


def kmer_spectrum(column: ColumnLike, k: int, min_coverage: int, auto_k: bool = False, group_offsets=None):
    """H4: k-mer spectra of read groups (include/rogtk_hip.h, rogtk_kmer_spectrum_host).

    ``group_offsets`` (n_groups + 1 row offsets, contiguous groups; None = one group)
    plays the role of polars' group_by: each group is what one call of the
    reference's assemble_sequences_expr sees. Returns a dict of numpy arrays:
    kmer_hi / kmer_lo (u64; hi only for k_eff 64), exts (u8), counts (u16),
    entry_offsets (n_groups + 1) and stats (n_groups x 5, columns KMER_STATS).
    """
    ch = one_chunk(column)
    n = ch.n
    cap = ctypes.c_int64(0)
    _lib.call("rogtk_kmer_capacity", _lib.ptr(ch.offsets), ch.offset_width, n, ctypes.byref(cap))
    capn = max(int(cap.value), 1)
    go = None if group_offsets is None else np.ascontiguousarray(group_offsets, dtype=np.int64)
    G = 1 if go is None else len(go) - 1
    km = np.empty(2 * capn, dtype=np.uint64)
    ex = np.empty(capn, dtype=np.uint8)
    cn = np.empty(capn, dtype=np.uint16)
    eo = np.empty(G + 1, dtype=np.int64)
    st = np.empty(5 * G, dtype=np.int64)
    _lib.call("rogtk_kmer_spectrum_host", *ch.loose(), _lib.ptr(go), 0 if go is None else G, int(k), int(bool(auto_k)),
              int(min_coverage), capn, _lib.ptr(km), _lib.ptr(ex), _lib.ptr(cn), _lib.ptr(eo), _lib.ptr(st))
    m = int(eo[G])
    return {"kmer_hi": km[0:2 * m:2].copy(), "kmer_lo": km[1:2 * m:2].copy(), "exts": ex[:m].copy(),
            "counts": cn[:m].copy(), "entry_offsets": eo, "stats": st.reshape(G, 5)}


# ------------------------------------------------------------ namespaces
class UmiNamespace:
    """rogtk/__init__.py:412-491 (`pl.col(..).umi.*`)."""

    def __init__(self, column: ColumnLike):
        self._c = column

    def complexity_all(self):
        return umi_complexity_scores(self._c)

    def all_scores(self):
        return self.complexity_all()

    def _one(self, name):
        return umi_complexity(self._c, (name,))[name]

    def shannon_entropy(self):
        return self._one("shannon_entropy")

    def linguistic_complexity(self):
        return self._one("linguistic_complexity")

    def homopolymer_fraction(self):
        return self._one("homopolymer_fraction")

    def dinucleotide_entropy(self):
        return self._one("dinucleotide_entropy")

    def combined_score(self):
        return self._one("combined_score")

    def longest_homopolymer_run(self):
        return self._one("longest_homopolymer_run")

    def dust_score(self):
        return self._one("dust_score")

    def cluster(self, umi_len: int = 0, max_distance: int = 1, method: str = "cluster", groups=None):
        """Extension (no reference counterpart): H3 cluster ids ("directional": DESIGN.md §4c;
        groups: within each key, §4d)."""
        return umi_cluster(self._c, umi_len, max_distance, method, groups)[0]

    def correct(self, umi_len: int = 0, max_distance: int = 1, method: str = "cluster", groups=None):
        """Extension (no reference counterpart): every row's UMI replaced by the
        representative of its cluster (method="directional": §4c; groups: §4d)."""
        from .correct import umi_correct

        return umi_correct(self._c, umi_len, max_distance, method, groups).corrected

    def dedup(self, umi_len: int = 0, score=None, max_distance: int = 1, method: str = "cluster", groups=None):
        """Extension (no reference counterpart): the keep mask of UMI deduplication, true for the
        row with the largest score of its cluster (ties: the first row), DESIGN.md §4f."""
        from .dedup import umi_dedup

        return umi_dedup(self._c, umi_len, score, max_distance, method, groups).keep


class HammingExpr:
    """rogtk/__init__.py:326-349 (`pl.col(..).hamming.*`)."""

    def __init__(self, column: ColumnLike):
        self._c = column

    def distance(self, target: str):
        return hamming_distance(self._c, target)

    def within(self, target: str, max_distance: int = 1):
        return hamming_within(self._c, target, max_distance)


class Col:
    """Eager stand-in for a polars expression over one string column."""

    def __init__(self, column: ColumnLike):
        self.column = column
        self.umi = UmiNamespace(column)
        self.hamming = HammingExpr(column)
        from .strings import CigarNamespace, DnaNamespace, FuzzyNamespace

        self.dna = DnaNamespace(column)
        self.cigar = CigarNamespace(column)
        self.fuzzy = FuzzyNamespace(column)
        from .barcode import BarcodeNamespace

        self.barcode = BarcodeNamespace(column)


def col(column: ColumnLike) -> Col:
    return Col(column)
