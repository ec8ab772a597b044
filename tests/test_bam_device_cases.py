"""CPU checks of tests/bam_device_cases.py: the conditions the cases must meet so that the
GPU tests of the device BAM path (tests/test_gpu_bam_device.py) cannot pass vacuously: a
validity bitmap that is mixed in every word, empty but valid UMIs, names at the lossy 3x
bound, ranges whose row counts leave every kind of bit offset, clusters that merge under one
edit, corrupt records that frame but do not fit. Every figure is printed before it is
asserted. No GPU: the oracle, numpy and the host-only range entry points."""
from __future__ import annotations

from collections import Counter

import numpy as np
import pytest

import bam_device_cases as C
from oracle import pybam
from oracle import pyoracle as P

SOURCES = ("sequence", "name")


@pytest.fixture(scope="module")
def device_bam(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("bamdev") / "device.bam")
    C.write_device_bam(p)
    return p


@pytest.fixture(scope="module")
def rows(device_bam):
    return {m: pybam.bam_rows(device_bam, m) for m in C.MODES}


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("mode", C.MODES)
def test_umi_column_is_mixed(rows, mode, source):
    umis = C.oracle_umis(rows[mode], source)
    n = len(umis)
    assert n == C.N_RECORDS + 2
    valid = np.array([u is not None for u in umis])
    null_share = 1 - valid.mean()
    regular_share = sum(C.is_regular(u) for u in umis) / n
    empty = sum(u == b"" for u in umis)
    words = [valid[i:i + 64] for i in range(0, n - 63, 64)]
    mixed = sum(1 for w in words if w.any() and not w.all())
    longest = max(len(r["name"].encode()) for r in rows[mode])
    print(f"{mode}/{source}: null {null_share:.3f}, regular {regular_share:.3f}, empty {empty}, "
          f"mixed words {mixed}/{len(words)}, longest name {longest} B")
    assert 0.10 <= null_share <= 0.30
    assert regular_share >= 0.40
    assert len(words) == 23 and mixed == len(words)  # no full word all ones or zero
    if source == "name":
        assert empty >= 50
    assert longest == 762  # 254 invalid bytes, U+FFFD each: the decode's 3x bound is reached


def test_every_name_kind_occurs(rows):
    kinds = Counter(C.device_kinds(C.SEED, C.N_RECORDS))
    print(dict(kinds))
    assert set(kinds) == set(C.NAME_KINDS)
    assert min(kinds.values()) >= 20
    # the kinds are what they say, on the decoded names (htslib keeps "*", noodles: "unknown")
    by = {k: [i for i, x in enumerate(C.device_kinds(C.SEED, C.N_RECORDS)) if x == k] for k in C.NAME_KINDS}
    h, nd = rows["htslib"], rows["noodles"]
    assert all(h[i]["name"] == "*" and nd[i]["name"] == "unknown" for i in by["star"])
    assert all("\ufffd" in h[i]["name"] and "_" in h[i]["name"] for i in by["bad_utf8"])
    assert all(C.oracle_umis([h[i]], "name")[0].endswith("\ufffd".encode()) for i in by["bad_utf8"])
    assert all("_" not in h[i]["name"] for i in by["no_sep"])
    assert all(h[i]["name"].endswith("_") for i in by["sep_last"])
    assert all(len(h[i]["name"]) == 254 and len(C.oracle_umis([h[i]], "name")[0]) == 12 for i in by["long254"])
    assert all(h[i]["name"] == "\ufffd" * 254 for i in by["ff254"])
    assert all(h[i]["name"].count("_") == 2 and 1 <= len(C.oracle_umis([h[i]], "name")[0]) <= 11
               for i in by["multi_sep"])
    # sequence lengths around the UMI length, IUPAC rows and missing qualities are all there
    lens = Counter(0 if r["sequence"] is None else len(r["sequence"]) for r in h)
    assert all(lens[l] >= 20 for l in (0, 1, 5, 11, 12, 13, 150)), lens
    assert sum(r["sequence"] is not None and r["quality_scores"] is None for r in h) >= 20
    assert sum(bool(set(r["sequence"] or "") - set("ACGTN")) for r in rows["htslib_blocks"]) >= 50


def test_long_records_span_blocks_and_chunks(rows):
    import struct

    recs = C.long_records()
    assert [struct.unpack_from("<I", r, 20)[0] for r in recs] == list(C.LONG_L_SEQ)
    assert all(len(r) > 100 * C.BLOCK and len(r) > 20 * 4096 for r in recs)
    for i, r in enumerate(rows["htslib"][-2:]):
        assert r["name"].startswith(f"long{i}_") and len(r["sequence"]) == C.LONG_L_SEQ[i]
        assert C.is_regular(C.oracle_umis([r], "name")[0])
        assert C.oracle_umis([r], "name") == C.oracle_umis([r], "sequence")


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("mode", C.MODES)
def test_one_edit_merges_clusters(rows, mode, source):
    umis = C.oracle_umis(rows[mode], source)
    col = P.StrCol.from_list(umis)
    _, _, k0, _ = P.umi_cluster(col, C.UMI_LEN, 0)
    cid, valid, k1, _ = P.umi_cluster(col, C.UMI_LEN, 1)
    reg = {int(cid[i]) for i, u in enumerate(umis) if valid[i] and C.is_regular(u)}
    irr = {int(cid[i]) for i, u in enumerate(umis) if valid[i] and not C.is_regular(u)}
    print(f"{mode}/{source}: {k0} clusters at distance 0, {k1} at 1, {len(reg & irr)} mixed clusters")
    assert k1 < k0
    assert len(reg & irr) >= 1  # an irregular string clustered with a regular one


@pytest.mark.parametrize("seed", [C.SEED, C.SEED2])
def test_ranges_leave_every_bit_offset(tmp_path, seed):
    """Five ranges of the file: all of them start records, and their row counts take at least
    three distinct non-zero values mod 64, so the concatenation shifts validity words by
    several amounts. (Host-only entry points: the library loads without a GPU.)"""
    from rogtk_amd import bam as B

    p = str(tmp_path / "r.bam")
    C.write_device_bam(p, seed)
    pts = B.bam_split_points(p, 5)
    assert len(pts) == 6
    counts = range_counts(p, pts)
    print(f"seed {seed}: range counts {counts}, mod 64 {[c % 64 for c in counts]}")
    assert sum(counts) == C.N_RECORDS + 2
    assert all(c > 0 for c in counts)
    assert len({c % 64 for c in counts} - {0}) >= 3


def range_counts(path, pts):
    """Records that start in each compressed range [pts[i], pts[i + 1]): from a plain walk of
    the blocks and rogtk_bam_find_record's skips."""
    import gzip
    import struct

    from rogtk_amd import bam as B

    raw = open(path, "rb").read()
    offs, o, u = {}, 0, 0
    while o < len(raw):
        bsize = struct.unpack_from("<H", raw, o + 16)[0] + 1
        offs[o] = u
        u += struct.unpack_from("<I", raw, o + bsize - 4)[0]
        o += bsize
    offs[len(raw)] = u
    data = gzip.decompress(raw)
    q = len(synth_header())
    starts = []
    while q < len(data):
        starts.append(q)
        q += 4 + struct.unpack_from("<I", data, q)[0]
    starts = np.array(starts)
    for c in pts[1:-1]:  # the range's first record is where find_record says
        nxt = starts[starts >= offs[c]]
        assert B.bam_find_record(path, c) == int(nxt[0] - offs[c])
    return [int(((starts >= offs[a]) & (starts < offs[b])).sum()) for a, b in zip(pts, pts[1:])]


def synth_header():
    from rogtk_amd import synth_bam

    return synth_bam.header_bytes(C.TEXT, C.REFS)


def test_corrupt_records_frame_but_do_not_fit():
    import struct

    recs = C.device_records(C.SEED, 300)
    assert all(C.record_fits(r) for r in recs)
    for what in ("l_seq", "n_cigar"):
        for r in recs[:50]:
            bad = C.corrupt(r, what)
            assert len(bad) == len(r) and bad[:4] == r[:4]  # block_size unchanged: it frames
            assert not C.record_fits(bad)
            diff = [i for i in range(len(r)) if bad[i] != r[i]]
            assert set(diff) <= (set(range(20, 24)) if what == "l_seq" else {16, 17})
    assert struct.unpack_from("<H", C.corrupt(recs[0], "n_cigar"), 16)[0] == 0xFFFF
    with pytest.raises(ValueError):
        C.corrupt(recs[0], "name")


@pytest.mark.parametrize("n", [200, 329])
def test_hand_batch_is_mixed(n):
    hb = C.hand_batch(3, n)
    assert sum(C.APPEND_COUNTS) == 329
    assert hb["name_off"][0] == 0 and hb["seq_off"][0] == 0
    assert hb["name_off"].dtype == np.int64 and hb["seq_valid"].dtype == np.uint64
    assert C.column_items(hb["name_off"], hb["name_val"], None, n) == hb["names"]
    assert C.column_items(hb["seq_off"], hb["seq_val"], None, n) == hb["seqs"]
    assert np.array_equal(C.unpack_bits(hb["seq_valid"], n), hb["valid"])
    assert {len(s) for s in hb["seqs"]} == set(C.HAND_SEQ_LENS)
    assert max(len(x) for x in hb["names"]) == 762
    null_share = 1 - hb["valid"].mean()
    null_with_bytes = sum(1 for i in range(n) if not hb["valid"][i] and len(hb["seqs"][i]) > 0)
    print(f"n {n}: null share {null_share:.3f}, null rows with bytes {null_with_bytes}")
    assert 0.1 <= null_share <= 0.3 and null_with_bytes >= 10
    for source, sep, umi_len in ((0, "_", 12), (1, "_", 12), (1, ":", 12), (0, "_", 1), (0, "_", 40)):
        umis = C.expect_umis(hb["names"], hb["seqs"], hb["valid"], source, umi_len, sep)
        v = np.array([u is not None for u in umis])
        words = [v[i:i + 64] for i in range(0, n - 63, 64)]
        empty = sum(u == b"" for u in umis)
        print(f"  source {source} sep {sep!r} umi_len {umi_len}: nulls {int((~v).sum())}, empty valid {empty}")
        assert words and all(w.any() and not w.all() for w in words)  # both bit values in every full word
        assert empty >= 3
        if source == 0:
            assert max(len(u) for u in umis if u is not None) == min(umi_len, 150)
            assert np.array_equal(v, hb["valid"])
    # without the validity no sequence row is null, whatever its length
    assert None not in C.expect_umis(hb["names"], hb["seqs"], None, 0, 12, "_")


def test_slices_rebuild_the_batch():
    hb = C.hand_batch(3, 329)
    bases = np.concatenate([[0], np.cumsum(C.APPEND_COUNTS)])
    assert list(bases[:-1]) == [0, 5, 135, 136, 200, 259]
    assert {int(b) % 64 for b in bases[1:-1]} == {5, 7, 8, 3}
    assert (bases[1] + 130 - 1) // 64 - bases[1] // 64 == 2  # the 130-row batch spans three words
    names, seqs, valid = [], [], []
    for a, b in zip(bases, bases[1:]):
        s = C.slice_batch(hb, int(a), int(b))
        assert s["name_off"][0] == 0 and s["seq_off"][0] == 0
        names += C.column_items(s["name_off"], s["name_val"], None, b - a)
        seqs += C.column_items(s["seq_off"], s["seq_val"], None, b - a)
        valid += list(C.unpack_bits(s["seq_valid"], b - a))
    assert names == hb["names"] and seqs == hb["seqs"] and valid == list(hb["valid"])


def test_expect_concat_against_a_list():
    parts = C.concat_parts(1)
    assert [p[3] for p in parts] == list(C.CONCAT_COUNTS) and sum(C.CONCAT_COUNTS) == 332
    items = []
    for off, val, words, c in parts:
        if c % 64:  # the bits past the count are set in the source: they must not reach the result
            assert int(words[-1]) >> (c % 64) == (1 << (64 - c % 64)) - 1
        items += C.column_items(off, val, words, c)
    off, val, words = C.expect_concat(parts)
    n = len(items)
    assert len(off) == n + 1 and len(words) == (n + 63) // 64
    v = C.unpack_bits(words, n)
    raw = val.tobytes()
    for i, it in enumerate(items):  # null rows keep their bytes in a concatenation
        assert bool(v[i]) == (it is not None)
        if it is not None:
            assert raw[off[i]:off[i + 1]] == it
    assert int(words[-1]) >> (n % 64) == 0
    share = 1 - v.mean()
    assert 0.2 <= share <= 0.4
    full = [v[i:i + 64] for i in range(0, n - 63, 64)]
    assert all(w.any() and not w.all() for w in full)
    lens = np.diff(off)
    assert lens.min() == 0 and lens.max() == 20
    o0, v0, w0 = C.expect_concat([])
    assert list(o0) == [0] and len(v0) == 0 and len(w0) == 0
