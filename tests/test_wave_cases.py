"""CPU checks of tests/wave_cases.py: every case hits what its name says (its figures from
the pure-Python oracle, its predicted classes), and the C++ oracle the GPU tests compare
against agrees with the pure-Python one on it. This is what keeps the GPU tests from passing
on cases that drifted off their limits."""
from __future__ import annotations

import numpy as np
import pytest

import wave_cases as W

CASES = W.all_cases()


def _oracle_rows(ref, g, K):
    """Group g of a kmer_spectrum result as py_kmer_spectrum's [(kmer, exts, count)]."""
    from oracle import pyoracle as P

    a, b = int(ref["group_offsets"][g]), int(ref["group_offsets"][g + 1])
    return [(P.kmer_to_str(ref["kmer_hi"][i], ref["kmer_lo"][i], K), int(ref["exts"][i]), int(ref["counts"][i]))
            for i in range(a, b)]


@pytest.mark.parametrize("name", list(CASES))
def test_case_hits_its_limit(name):
    c = CASES[name]
    f = c.figures()
    for key, want in c.expect.items():
        if isinstance(want, tuple):
            assert want[0] <= f[key] <= want[1], (key, f[key], want)
        else:
            assert f[key] == want, (key, f[key], want)
    assert c.predict() == (c.init, c.final), (c.predict(), f)
    nrows, words, obs = W.group_shape(c.rows, c.K)
    if "words" in c.extra:
        assert words == c.extra["words"]
    if c.init in (2, 6):
        assert nrows <= W.WAVE_ROWS and words <= W.WAVE_WORDS[c.init] and obs > 0
        assert c.init == 2 or words > W.WAVE_WORDS[2]
    # without the wave class (rogtk_kmer_set_path(2)) no group starts in it
    assert c.predict(wave=False)[0] in (0, 3, 1, 4)
    ex = c.extra
    if "claim_loop" in ex or "L0_eq_Ls" in ex or "L0" in ex:
        sg = W.segments(c.rows, c.K)
        t = W.claim_trip(c.rows, c.K, W.WAVE_CLAIM[2])
        if ex.get("L0_eq_Ls"):
            assert sg["L0"] == sg["Ls"]
        if "L0" in ex:
            assert sg["L0"] == ex["L0"] and sg["Ls"] > 40
        if ex.get("claim_loop") == "uniform":
            assert t is not None and t < sg["L0"]
        if ex.get("claim_loop") == "tail":
            assert t is not None and t >= sg["L0"]
        if ex.get("mid"):
            assert t < sg["Ls"] - 8  # well before its last trip
    elif c.init == 2 and c.K == 16:
        # the replay of the insert order agrees with the count: a bail-out by claims iff past the cap
        assert (W.claim_trip(c.rows, c.K, W.WAVE_CLAIM[2]) is not None) == (f["distinct_not_allt"] > W.WAVE_CLAIM[2])


def test_cpp_oracle_equals_python_oracle():
    """oracle.pyoracle.kmer_spectrum (C++) == py_kmer_spectrum on every case: entries and stats."""
    from oracle import pyoracle as P

    for (k, mc), groups in W.general_layouts().items():
        items, go = W.flatten(groups)
        ref = P.kmer_spectrum(P.StrCol.from_list(items), k, mc, False, np.array(go))
        for g, c in enumerate(groups):
            want, stats = W._spectrum(tuple(c.rows), k, mc)
            assert _oracle_rows(ref, g, c.K) == want, c.name
            assert tuple(int(x) for x in ref["stats"][g]) == stats, c.name


def test_restated_classifier_edges():
    K = 16
    ic = W.initial_class
    assert [ic(64, 192, 1, K), ic(64, 193, 1, K), ic(64, 320, 1, K), ic(64, 321, 1, K), ic(65, 10, 1, K)] == [2, 6, 6, 3, 3]
    assert [ic(192, 576, 1, K), ic(193, 576, 1, K), ic(192, 577, 1, K), ic(256, 768, 1, K), ic(257, 768, 1, K),
            ic(512, 4096, 1, K), ic(513, 600, 1, K), ic(512, 4097, 1, K)] == [3, 1, 1, 1, 4, 4, 0, 0]
    assert ic(10, 10, 0, K) == 0 and ic(10, 10, 5, 64) == 0 and ic(10, 10, 5, 32) == 3
    assert ic(64, 192, 1, K, wave=False) == 3
    fc = W.final_class
    # (class, words, distinct, distinct without all-T, valid, top bucket)
    assert fc(2, 100, 833, 832, 512, 256) == 2  # the all-T key claims no slot
    assert fc(2, 100, 833, 833, 1, 1) == 6 and fc(2, 100, 513, 513, 513, 1) == 6 and fc(2, 100, 300, 300, 300, 257) == 3
    assert fc(6, 300, 1664, 1664, 1024, 256) == 6 and fc(6, 300, 1665, 1665, 1, 1) == 1 and fc(6, 300, 1025, 1025, 1025, 1) == 1
    assert fc(3, 300, 1472, 1472, 1024, 1) == 3 and fc(3, 300, 1473, 1473, 1, 1) == 1 and fc(1, 300, 2049, 2049, 1, 1) == 4
    assert fc(4, 300, 6144, 6144, 2048, 1) == 4 and fc(4, 300, 6145, 6145, 1, 1) == 0 and fc(4, 300, 3000, 3000, 2049, 1) == 0
    assert W.bucket_of(W.kmer_key("T" * 16), 16) == 255 and W.bucket_of(W.kmer_key("ACGT"), 4) == W.kmer_key("ACG")
    assert W.bucket_of(W.kmer_key("ACGTTTTT"), 8) == W.kmer_key("ACGT")


def test_shape_cases_cover_the_segment_arithmetic():
    """Groups of 1..64 rows: odd and even Ls, an empty uniform loop and a long one, lanes with
    no position and with one, rows that yield nothing, every word-multiple length as a group's
    last row and inside it."""
    shapes = [c for c in CASES.values() if c.extra.get("shape")]
    assert sorted({len(c.rows) for c in shapes}) == list(W.SHAPE_ROWS)
    sgs = [W.segments(c.rows, 16) for c in shapes]
    assert {s["Ls"] & 1 for s in sgs} == {0, 1}
    assert any(s["L0"] == 0 for s in sgs) and any(s["L0"] >= 16 for s in sgs)
    nst = {n for s in sgs for n in s["nst"]}
    assert 0 in nst and 1 in nst
    assert {s["spr"] for s in sgs} >= {64, 32, 21, 3, 2, 1}
    rows = [r for c in shapes for r in c.rows]
    assert None in rows and b"" in rows
    assert any(r and b"N" in r for r in rows) and any(r and r.islower() for r in rows)
    assert any(r is not None and 0 < len(r) < 16 for r in rows) and any(r is not None and len(r) == 16 for r in rows)
    last = {len(c.rows[-1]) for c in shapes if c.rows[-1] is not None}
    inner = {len(r) for c in shapes for r in c.rows[:-1] if r is not None}
    assert last >= {32, 64, 96, 128, 160} and inner >= {32, 64, 96, 128, 160}
    assert {c.init for c in shapes} == {2, 6} and all(c.init == c.final for c in shapes)


def test_layouts():
    by = CASES
    st = W.layout_state()
    assert len(st) == W.CHUNK + 1 and all(c.init == 2 for c in st[:8]) and {(c.k, c.min_cov) for c in st} == {(16, 2)}
    assert [c.final for c in st[:8]] == [2, 2, 4, 2, 6, 2, 3, 2]
    assert st[3] is st[5] is st[7] is st[-1] is by["plain"] and all(c.init == 0 for c in st[8:-1])
    f = [c.figures() for c in st[:8]]
    assert f[0]["allt_count"] == 3 and f[1]["allt_count"] == 1  # valid, then below min_coverage 2
    assert f[2]["distinct_not_allt"] > W.WAVE_CLAIM[2] and f[4]["valid"] > W.WAVE_VALID[2] >= f[4]["distinct"] - 320
    assert f[6]["top_bucket"] >= W.WAVE_DEEP and f[6]["valid"] <= W.WAVE_VALID[2]
    pl = W.layout_pipeline()
    assert {(c.k, c.min_cov) for c in pl} == {(16, 2)}
    init = [c.init for c in pl]
    chunks = [init[i:i + W.CHUNK] for i in range(0, len(init), W.CHUNK)]
    assert [ch.count(2) for ch in chunks] == [1, 2, 3, 64, 3] and len(chunks[-1]) == 5
    for ch in chunks[:3]:
        assert {6, 3, 0} <= set(ch)
    assert any(c.init == 0 and len(c.rows) > 512 for c in pl) and any(len(c.rows) == 0 for c in pl)
    # every case runs in some call of its own (k, min_coverage)
    calls = W.general_layouts()
    assert sum(len(v) for v in calls.values()) == len(CASES) and set(calls) >= {(16, 1), (16, 2), (8, 1), (8, 2), (4, 1)}


def test_fixed_stride_predictions():
    """Fixed-stride staging counts stride words for every row: at 150-base rows (stride 5) the
    class 2 / 6 word limit lies between 38 and 39 rows, and 64 rows fill class 6."""
    for c in W.stride_limit_cases():
        assert c.predict(5) == (c.init, c.final), c.name
    got = {len(c.rows): c.init for c in W.stride_limit_cases()}
    assert got == {38: 2, 39: 6, 64: 6, 65: 3}
    for (k, mc), groups in W.layouts_fixed_stride().items():
        lens = [len(r) for c in groups for r in c.rows if r is not None]
        assert 128 < max(lens) <= 160 and W.effective_k(k) == 16, (k, mc)  # stride 5
        # a short-row case takes more words at the stride than ragged, never another class here
        # except by the word limit
        for c in groups:
            if c.init == 2 and len(c.rows) <= 38:
                assert c.predict(5) == (c.init, c.final), c.name
