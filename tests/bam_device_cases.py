"""Cases for the device BAM path (config C5: rogtk_bam_next_dev -> rogtk_bam_umi_append /
rogtk_bam_append_strings -> rogtk_concat_strings_dev -> H3), shared by
tests/test_bam_device_cases.py (CPU: the conditions the cases must meet) and
tests/test_gpu_bam_device.py (GPU: the kernels against these expectations).

Pure Python / numpy: SAMv1 records through rogtk_amd.synth_bam.record_bytes, string columns
in the layout of rogtk_bam_batch (int64 offsets from 0, uint8 values, 64-bit validity words
in Arrow LSB order), and the expected UMI / concatenated columns restated in Python.

What the device path never saw before these cases: null UMIs (a validity bitmap that is not
all ones, so a wrong shift or a lost carry in the bit merges shows), empty but valid UMIs,
names that grow when decoded lossily (U+FFFD per invalid byte, 254 -> 762 bytes), "*" names,
records longer than a BGZF block or a read chunk, and corrupt records.
"""
from __future__ import annotations

import struct
from typing import List, Optional, Sequence

import numpy as np

from rogtk_amd import synth_bam

REFS = [(b"chr1", 1000), (b"chrX", 500), (b"contig_\xff\xfe", 10)]
TEXT = "@HD\tVN:1.6\n"
BLOCK = 997  # BGZF block payload: records straddle blocks, the long ones span hundreds
MODES = ("noodles", "htslib", "htslib_blocks")
UMI_LEN = 12
N_PARENTS = 40
# name kinds of device_records (kind k < 7 for rng.integers(0, 16) == k, "plain" otherwise)
NAME_KINDS = ("star", "bad_utf8", "no_sep", "sep_last", "long254", "ff254", "multi_sep", "plain")
SEED, SEED2, N_RECORDS = 5, 9, 1500


# ------------------------------------------------------------------ records
def _parents(rng) -> List[str]:
    return ["".join(rng.choice(list("ACGT"), UMI_LEN)) for _ in range(N_PARENTS)]


def _umi(rng, parents) -> str:
    """A parent, with one substitution from ACGTN in 30 % of the draws."""
    u = list(parents[int(rng.integers(N_PARENTS))])
    if rng.random() < 0.3:
        u[int(rng.integers(UMI_LEN))] = str(rng.choice(list("ACGTN")))
    return "".join(u)


def _name(kind: int, i: int, u: str, rng) -> bytes:
    if kind == 0:
        return b"*"
    if kind == 1:  # invalid bytes before and after the separator, a truncated 3-byte tail
        return b"bad\xff_\xc3(" + u.encode()[:6] + b"\xe2\x82"
    if kind == 2:
        return f"noumi{i}".encode()
    if kind == 3:  # the separator is the last byte: a valid, empty UMI
        return f"x{i}_".encode()
    if kind == 4:  # l_read_name = 255, the format's limit
        return b"n" * (254 - UMI_LEN - 1) + b"_" + u.encode()
    if kind == 5:  # 254 invalid bytes: 762 bytes once lossy
        return b"\xff" * 254
    if kind == 6:
        return f"a_b_{u[:int(rng.integers(1, UMI_LEN))]}".encode()
    return f"r{i}_{u}".encode()


def _specs(seed: int, n: int):
    rng = np.random.default_rng(seed)
    parents = _parents(rng)
    out = []
    for i in range(n):
        u = _umi(rng, parents)
        kind = int(rng.integers(0, 16))
        name = _name(kind, i, u, rng)
        l_seq = int(rng.choice([0, 1, 5, 11, 12, 13, 150, int(rng.integers(0, 300))]))
        alphabet = "=ACMGRSVTWYHKDBN" if kind in (7, 8) else "ACGT"
        seq = (u + "".join(rng.choice(list(alphabet), 300)))[:l_seq]
        qual = None if kind == 9 and l_seq else bytes(rng.integers(0, 42, size=l_seq, dtype=np.uint8))
        n_cig = int(rng.integers(0, 6))
        raw_cigar = [int(rng.integers(0, 200)) << 4 | int(rng.integers(0, 9)) for _ in range(n_cig)]
        out.append(dict(kind=NAME_KINDS[min(kind, 7)], name=name, ref_id=int(rng.choice([-1, 0, 1, 2, 3])),
                        pos=int(rng.choice([-1, 0, 12345])), flag=int(rng.integers(0, 1 << 16)), seq=seq, qual=qual,
                        raw_cigar=raw_cigar))
    return out


def device_records(seed: int, n: int) -> List[bytes]:
    """n SAMv1 records (block_size included) with the field spread of test_bam's random
    records and the name kinds of NAME_KINDS; the first 12 bases of SEQ and the name's tail
    carry a UMI drawn from 40 parents (30 % with one substitution from ACGTN)."""
    return [synth_bam.record_bytes(**{k: v for k, v in s.items() if k != "kind"}) for s in _specs(seed, n)]


def device_kinds(seed: int, n: int) -> List[str]:
    """The name kind of each record of device_records(seed, n)."""
    return [s["kind"] for s in _specs(seed, n)]


LONG_L_SEQ = (70_001, 200_000)


def long_records() -> List[bytes]:
    """Two reads of 70,001 and 200,000 bases named long<i>_<UMI>: each record spans hundreds
    of 997-byte BGZF blocks and several 4096-byte read chunks. Bases repeat a random motif of
    61 bases after the UMI and qualities step by 7 mod 41 (61 and 41 are odd primes: no
    position aliases with a 64-lane stride), which also keeps the two records a small share
    of the compressed file, so that every one of five equal ranges starts records."""
    rng = np.random.default_rng(77)
    out = []
    for i, l_seq in enumerate(LONG_L_SEQ):
        u = "".join(rng.choice(list("ACGT"), UMI_LEN))
        motif = "".join(rng.choice(list("ACGT"), 61))
        seq = (u + motif * (l_seq // 61 + 1))[:l_seq]
        qual = ((np.arange(l_seq, dtype=np.int64) * 7) % 41).astype(np.uint8).tobytes()
        out.append(synth_bam.record_bytes(name=f"long{i}_{u}".encode(), ref_id=i, pos=7, flag=0,
                                          cigar=[(l_seq, "M")], seq=seq, qual=qual))
    return out


def write_device_bam(path: str, seed: int = SEED, n: int = N_RECORDS, long: bool = True) -> None:
    """The file the decode and end-to-end tests read: device_records + long_records."""
    recs = device_records(seed, n) + (long_records() if long else [])
    synth_bam.write_bam(path, REFS, recs, text=TEXT, block=BLOCK)


def write_header_only_bam(path: str) -> None:
    synth_bam.write_bam(path, REFS, [], text=TEXT, block=BLOCK)


def corrupt(record: bytes, what: str) -> bytes:
    """The record with l_seq raised by 1000 ("l_seq") or n_cigar_op set to 0xFFFF
    ("n_cigar"); block_size is unchanged, so the record still frames but its variable fields
    no longer fit in it."""
    b = bytearray(record)
    if what == "l_seq":
        struct.pack_into("<I", b, 4 + 16, struct.unpack_from("<I", b, 4 + 16)[0] + 1000)
    elif what == "n_cigar":
        struct.pack_into("<H", b, 4 + 12, 0xFFFF)
    else:
        raise ValueError(what)
    return bytes(b)


def record_fits(record: bytes) -> bool:
    """RecView::fits() of bam.hip restated: the fixed and variable fields lie in block_size."""
    bs = struct.unpack_from("<I", record, 0)[0]
    l_name = record[4 + 8]
    n_cig = struct.unpack_from("<H", record, 4 + 12)[0]
    l_seq = struct.unpack_from("<I", record, 4 + 16)[0]
    return bs >= 32 and 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq <= bs


# ------------------------------------------------------------------ expectations
def is_regular(u: Optional[bytes], umi_len: int = UMI_LEN) -> bool:
    return u is not None and len(u) == umi_len and set(u) <= set(b"ACGT")


def oracle_umis(rows, source: str, umi_len: int = UMI_LEN, sep: str = "_") -> List[Optional[bytes]]:
    """The UMI column of oracle rows (oracle.pybam.bam_rows): the first umi_len bases of the
    sequence (null when it is null), or the decoded name after its last sep (null without)."""
    out = []
    for r in rows:
        if source == "sequence":
            s = r["sequence"]
            out.append(None if s is None else s[:umi_len].encode())
        else:
            nm = r["name"].encode()
            k = nm.rfind(sep.encode())
            out.append(None if k < 0 else nm[k + 1:])
    return out


def expect_umis(names: Sequence[bytes], seqs: Sequence[bytes], valid, source: int, umi_len: int,
                sep: str) -> List[Optional[bytes]]:
    """rogtk_bam_umi_dev restated: source 0 = the first umi_len bytes of the sequence, null
    where valid says so (valid None: every row valid); 1 = the name after its last sep."""
    out = []
    for i in range(len(names)):
        if source == 0:
            out.append(None if (valid is not None and not valid[i]) else bytes(seqs[i][:umi_len]))
        else:
            k = names[i].rfind(sep.encode())
            out.append(None if k < 0 else bytes(names[i][k + 1:]))
    return out


def pack_bits(valid) -> np.ndarray:
    """Bools -> 64-bit words, Arrow LSB order, bits past the end zero."""
    v = np.asarray(valid, dtype=bool)
    words = (len(v) + 63) // 64
    b = np.zeros(words * 64, dtype=np.uint8)
    b[: len(v)] = v
    return np.packbits(b, bitorder="little").view(np.uint64).copy() if words else np.zeros(0, np.uint64)


def unpack_bits(words, n: int) -> np.ndarray:
    w = np.ascontiguousarray(words, dtype=np.uint64)
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:n].astype(bool)


def column(items: Sequence[Optional[bytes]], null_bytes: Optional[Sequence[bytes]] = None):
    """(int64 offsets from 0 [n + 1], uint8 values, validity words) of a list of bytes | None.
    null_bytes[i] is what a null row still occupies in the values (default: nothing)."""
    off = np.zeros(len(items) + 1, dtype=np.int64)
    chunks = []
    for i, s in enumerate(items):
        b = s if s is not None else (null_bytes[i] if null_bytes is not None else b"")
        chunks.append(b)
        off[i + 1] = off[i] + len(b)
    val = np.frombuffer(b"".join(chunks), dtype=np.uint8).copy()
    return off, val, pack_bits([s is not None for s in items])


def column_items(off, val, words, n: int) -> List[Optional[bytes]]:
    """The inverse of column (nulls lose their bytes)."""
    v = unpack_bits(words, n) if words is not None else np.ones(n, bool)
    raw = np.asarray(val, dtype=np.uint8).tobytes()
    return [raw[int(off[i]):int(off[i + 1])] if v[i] else None for i in range(n)]


def expect_concat(parts):
    """rogtk_concat_strings_dev restated. parts: [(offsets from 0 [c + 1], values, validity
    words, c)]; bits past c in a part's last word are ignored. Returns (offsets [n + 1],
    values, validity words with the bits past n zero)."""
    off, vals, bits = [np.zeros(1, np.int64)], [], []
    base = 0
    for o, v, w, c in parts:
        o = np.asarray(o, dtype=np.int64)
        off.append(o[1:c + 1] + base)
        vals.append(np.asarray(v, dtype=np.uint8)[: int(o[c])])
        base += int(o[c])
        bits.append(unpack_bits(w, c))
    return (np.concatenate(off), np.concatenate(vals) if vals else np.zeros(0, np.uint8),
            pack_bits(np.concatenate(bits) if bits else np.zeros(0, bool)))


# ------------------------------------------------------------------ hand-built batches
HAND_SEQ_LENS = (0, 1, 11, 12, 13, 150)


def hand_batch(seed: int, n: int) -> dict:
    """A name column and a sequence column in the layout of rogtk_bam_batch, with no BAM file
    behind them: names of the kinds a decoded batch holds (plus two with ':' so that both
    separators find UMIs), sequences of HAND_SEQ_LENS bytes, about 20 % of the sequence rows
    null. A null row keeps its bytes in the values, so only the validity bit can make its UMI
    null. Keys: names, seqs (lists of bytes), valid (bools), name_off / name_val, seq_off /
    seq_val / seq_valid (numpy, the device layout)."""
    rng = np.random.default_rng(seed)
    parents = _parents(rng)
    names, seqs = [], []
    for i in range(n):
        u = _umi(rng, parents)
        kind = int(rng.integers(0, 12))
        if kind == 0:
            nm = b"*"
        elif kind == 1:
            nm = "bad\ufffd_\ufffd(".encode() + u.encode()[:6] + "\ufffd".encode()
        elif kind == 2:
            nm = f"noumi{i}".encode()
        elif kind == 3:
            nm = f"x{i}_".encode()
        elif kind == 4:
            nm = b"n" * (254 - UMI_LEN - 1) + b"_" + u.encode()
        elif kind == 5:
            nm = "\ufffd".encode() * 254
        elif kind == 6:
            nm = f"a_b_{u[:int(rng.integers(1, UMI_LEN))]}".encode()
        elif kind == 7:
            nm = f"m:{i}_{u}".encode()
        elif kind == 8:
            nm = f"q_{i}:{u}:".encode() if i % 2 else f"q_{i}:{u}".encode()
        else:
            nm = f"r{i}_{u}".encode()
        names.append(nm)
        l = int(rng.choice(HAND_SEQ_LENS))
        seqs.append((u + "".join(rng.choice(list("ACGTN"), 150)))[:l].encode())
    valid = rng.random(n) >= 0.2
    name_off, name_val, _ = column(names)
    seq_off, seq_val, _ = column(seqs)
    return dict(names=names, seqs=seqs, valid=valid, name_off=name_off, name_val=name_val, seq_off=seq_off,
                seq_val=seq_val, seq_valid=pack_bits(valid))


def slice_batch(hb: dict, a: int, b: int) -> dict:
    """Rows [a, b) of a hand batch as a batch of their own: offsets from 0, validity bits
    from bit 0."""
    out = dict(names=hb["names"][a:b], seqs=hb["seqs"][a:b], valid=hb["valid"][a:b])
    for c in ("name", "seq"):
        off = hb[c + "_off"]
        out[c + "_off"] = (off[a:b + 1] - off[a]).copy()
        out[c + "_val"] = hb[c + "_val"][int(off[a]):int(off[b])].copy()
    out["seq_valid"] = pack_bits(out["valid"])
    return out


# the appends of test (c): row bases 0, 5, 135, 136, 200, 259 (bit offsets 5, 7, 8 and 3; the
# 130-row batch spans three validity words)
APPEND_COUNTS = (5, 130, 1, 64, 59, 70)
# the parts of test (a): empty, one-row, exactly one word, one word and a bit, three words
CONCAT_COUNTS = (1, 63, 0, 64, 65, 2, 130, 7)


def concat_parts(seed: int, counts: Sequence[int] = CONCAT_COUNTS, p_valid: float = 0.7):
    """Random string columns of the given row counts: rows of 0-20 bytes, validity random at
    p_valid, and every bit past the count in a part's last word set (they must be masked)."""
    rng = np.random.default_rng(seed)
    parts = []
    for c in counts:
        lens = rng.integers(0, 21, size=c)
        off = np.concatenate([np.zeros(1, np.int64), np.cumsum(lens, dtype=np.int64)])
        val = rng.integers(1, 250, size=int(off[-1]), dtype=np.uint8)
        words = pack_bits(rng.random(c) < p_valid)
        if c % 64:
            words[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(c % 64)
        parts.append((off, val, words, int(c)))
    return parts
