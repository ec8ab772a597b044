"""CPU: the minimizer filter's model (tests/mz_spec.py) against brute force and the oracle,
and every family holding what it is built for, from the model's facts alone. The GPU side
is tests/test_gpu_mz_filter.py."""
import random
from collections import Counter

import numpy as np
import pytest

import mz_spec as S
from test_kmer_cert import norep
from test_kmer_minimizer import _group, minimizer_counts

FAMILIES = list(S.BUILDERS)


def _facts(fam):
    return {g: S.decision(fam.rows_of(g), fam.mc) for g in fam.candidates()}


@pytest.mark.parametrize("name", FAMILIES)
def test_groups_are_what_they_are_built_for(name):
    """Every candidate's model verdict and brute-force K-mer count are what its builder
    says, and emptied implies nothing valid; a group marked gave_up has more than 384
    distinct minimizers within 28-run rows and fills a batch alone."""
    fam = S.family(name)
    facts = _facts(fam)
    assert facts
    for g, d in facts.items():
        info = fam.groups[g]
        rows = fam.rows_of(g)
        valid = S.has_valid_kmer(rows, fam.mc)
        assert d.verdict == info.expect, (g, info.role, d)
        assert valid == info.valid, (g, info.role)
        assert not (d.verdict == "emptied" and valid), (g, info.role)
        assert all(norep(r.decode()) for r in rows)
    for g, info in fam.groups.items():
        if not info.candidate and info.valid is not None:
            assert S.has_valid_kmer(fam.rows_of(g), fam.mc) == info.valid, (g, info.role)
    if name != "chunks":  # one chunk of 64 groups or one group per batch: one wave's batching
        cand = fam.candidates()
        plan = S.plan_batches([int(fam.go[g + 1] - fam.go[g]) for g in cand])
        alone = {cand[b[0]] for b in plan if len(b) == 1}
        for g, info in fam.groups.items():
            if info.gave_up:
                assert g in alone and facts[g].distinct > S.CLAIM_CAP and facts[g].max_runs <= S.LIST_CAP, (g, facts[g])


@pytest.mark.parametrize("name", FAMILIES)
def test_oracle_agrees(name):
    """The CPU oracle gives no entry to a group the model empties (nor to one built without
    a valid K-mer) and entries to every group built as valid; fillers have none."""
    fam = S.family(name)
    ref = S.oracle_ref(name)
    n = np.diff(ref["group_offsets"])
    assert len(n) == fam.n_groups and (ref["stats"][:, 0] == 32).all()
    for g, info in fam.groups.items():
        if info.candidate and S.decision(fam.rows_of(g), fam.mc).verdict == "emptied":
            assert n[g] == 0, (g, info.role)
        if info.valid is not None:
            assert (n[g] > 0) == info.valid, (g, info.role)
    fillers = np.ones(fam.n_groups, bool)
    fillers[list(fam.groups)] = False
    assert not n[fillers].any()


def test_lean_oracle_driver_is_the_oracle():
    """oracle_lean (buffers allocated once, for the half-million groups of `chunks`) returns
    what oracle.pyoracle.kmer_spectrum returns: on every group of two small families and on
    the stretches of `chunks` around its candidates."""
    for name, g0, g1 in (("batches", 0, None), ("coverage3", 0, None), ("chunks", 0, 600),
                         ("chunks", S.CHUNKS_G - 400, S.CHUNKS_G)):
        fam = S.family(name)
        a, b = S.oracle_lean(fam, 17, g0, g1), S.oracle_full(fam, 17, g0, g1)
        for f in a:
            assert np.array_equal(a[f], b[f]), (name, f)
        assert name == "chunks" or a["group_offsets"][-1] > 0


def test_lengths_family():
    fam = S.family("lengths")
    facts = _facts(fam)
    seen = Counter()
    for g, info in fam.groups.items():
        L = len(fam.rows_of(g)[0])
        assert all(len(r) == L for r in fam.rows_of(g)) and info.candidate == (L >= 32)
        seen[L] += 1
        kind = info.role.split(":")[1]
        if not info.candidate:
            continue
        a, b = fam.rows_of(g)
        if kind == "head32":  # only the first K-mer is shared
            assert a[:32] == b[:32] and not S.has_valid_kmer([a[1:], b[1:]], 2)
        if kind == "tail32":  # only the last K-mer is shared: the row's last window, next to the padding
            assert a[-32:] == b[-32:] and not S.has_valid_kmer([a[:-1], b[:-1]], 2)
            assert a.count(b"T"[0], L - 32) >= 16 and b"T" * 16 not in a
        assert (facts[g].verdict == "emptied") == (kind == "unrelated")
    assert sorted(seen) == list(S.LENGTHS) and set(seen.values()) == {4}
    assert fam.stride == 7 and fam.max_len == 224


def test_list_cap_family():
    fam = S.family("list_cap")
    d = _facts(fam)
    assert all(len(r) == 224 for g in fam.groups for r in fam.rows_of(g))
    over = fam.rows_of(0)
    assert all(len(S.row_runs(r)) > S.LIST_CAP for r in over) and over[0][-40:] == over[1][-40:]
    assert d[0].verdict == "kept" and d[0].max_count == 2 and d[0].distinct <= S.CLAIM_CAP
    assert S.capped_max_count(over) < 2  # a list that stopped at 28 would count nothing twice
    assert d[1].verdict == "emptied" and d[1].max_runs <= S.LIST_CAP
    assert d[2].verdict == "emptied" and d[2].max_runs == S.LIST_CAP
    assert d[3].verdict == "kept" and d[3].max_runs == S.LIST_CAP + 1 and d[3].max_count == 1


def test_claim_cap_family():
    fam = S.family("claim_cap")
    d = _facts(fam)
    sizes = [int(fam.go[g + 1] - fam.go[g]) for g in range(fam.n_groups)]
    assert S.plan_batches(sizes) == [[0], [1, 2, 3], [4, 5]]
    assert sizes[0] > 64 and d[0].distinct > S.CLAIM_CAP and d[0].max_count == 1 and fam.groups[0].gave_up
    # the split batch: together and in the big group past the cap, the small ones on their own merits
    assert d[2].distinct > S.CLAIM_CAP and d[2].max_count == 1
    assert d[1].verdict == "kept" and d[1].distinct <= S.CLAIM_CAP and d[3].verdict == "emptied"
    # near the cap: within 10 % below it; with its neighbour more list entries than the cap, no more distinct
    assert S.CLAIM_CAP * 0.9 <= d[4].distinct <= S.CLAIM_CAP and d[4].verdict == "emptied"
    entries = sum(len(S.row_runs(r)) for g in (4, 5) for r in fam.rows_of(g))
    assert entries > S.CLAIM_CAP >= d[4].distinct + d[5].distinct and d[5].verdict == "kept"
    assert all(v.max_runs <= S.LIST_CAP for v in d.values())


def test_passes_family():
    fam = S.family("passes")
    d = _facts(fam)
    assert fam.stride == 2
    for i, n in enumerate(S.PASS_SIZES):
        plain, tpl = fam.rows_of(2 * i), fam.rows_of(2 * i + 1)
        assert len(plain) == len(tpl) == n
        assert d[2 * i].verdict == "emptied" and d[2 * i].distinct <= S.CLAIM_CAP
        assert d[2 * i + 1].verdict == "kept" and d[2 * i + 1].max_count == 2 and d[2 * i + 1].distinct <= S.CLAIM_CAP
        assert tpl[1] == tpl[-1]
        # no 64-row pass reaches the count alone (sizes past 64: rows 1 and n - 1 lie in different passes)
        for p in range(0, n, 64):
            assert n == 64 or S.decision(tpl[p:p + 64], 2).verdict == "emptied"
    last = fam.rows_of(2 * len(S.PASS_SIZES))
    assert len(last) == 192 and S.decision(last[:128], 2).distinct <= S.CLAIM_CAP < S.decision(last, 2).distinct


def test_batches_family():
    fam = S.family("batches")
    d = _facts(fam)
    assert fam.n_groups <= 64  # one chunk: one wave forms every batch
    cand = fam.candidates()
    sizes = [int(fam.go[g + 1] - fam.go[g]) for g in cand]
    plan = [[cand[i] for i in b] for b in S.plan_batches(sizes)]
    assert plan[0] == list(range(8)) and plan[1][0] == 8  # the 9th candidate starts a batch
    rows = lambda b: sum(int(fam.go[g + 1] - fam.go[g]) for g in b)
    assert [16, 17] in plan and rows([16, 17]) == 64 and [18] in plan and rows([18, 19]) == 65
    # one template once in group 0 and once in group 7 of one batch: together they would reach the count
    assert d[0].verdict == d[7].verdict == "emptied"
    assert S.decision(fam.rows_of(0) + fam.rows_of(7), 2).verdict == "kept"
    assert {d[g].verdict for g in plan[0]} == {"emptied", "kept"}
    assert d[8].verdict == "kept" and d[8].max_runs > S.LIST_CAP and d[8].max_count == 1  # kept by the row alone
    # candidates lie between groups that are none
    none = [g for g, i in fam.groups.items() if not i.candidate]
    assert len(none) == 3 and all(min(cand) < g < max(cand) for g in none)
    polya, single, large = (fam.rows_of(g) for g in none)
    assert not norep(polya[0].decode()) and len(single) == 1
    assert len(large) > S.C3_ROWS and len(large) * fam.stride > S.C3_WORDS


def test_chunks_family():
    fam = S.family("chunks")
    d = _facts(fam)
    cand = fam.candidates()
    chunk = [g // 64 for g in cand]
    assert len(cand) == 6 and chunk[:3] == [S.CHUNK_A] * 3 and chunk[3:] == [S.CHUNK_A + S.CHUNK_WAVES] * 3
    assert fam.n_groups > 64 * S.CHUNK_WAVES + 64 * (S.CHUNK_A + 1)  # the wave of chunk 3 has a second chunk
    assert sum(int(fam.go[g + 1] - fam.go[g]) for g in cand) <= 64  # one batch
    assert [d[g].verdict for g in cand].count("kept") == 1 and d[cand[4]].verdict == "kept"
    assert S.decision(fam.rows_of(cand[0]) + fam.rows_of(cand[3]), 2).verdict == "kept"  # the template of both chunks
    sizes = np.diff(fam.go)
    assert sizes.sum() - 12 == fam.n_groups - 6 and (np.delete(sizes, cand) == 1).all()  # fillers: single rows


@pytest.mark.parametrize("mc", [3, 20])
def test_coverage_family(mc):
    fam = S.family(f"coverage{mc}")
    d = _facts(fam)
    assert fam.mc == mc and [len(fam.rows_of(g)) for g in range(4)] == [mc, mc - 1, mc, mc]
    assert d[0].verdict == "kept" and d[0].max_count == mc
    assert not fam.groups[1].candidate and len(set(fam.rows_of(1))) == 1
    assert d[2].verdict == "emptied" and d[2].max_count == mc - 1
    assert d[3].verdict == "kept" and len(set(fam.rows_of(3))) == mc


def test_decision_agrees_with_minimizer_counts():
    """On the random groups of tests/test_kmer_minimizer.py, wherever no cap applies, the
    verdict is that file's count against min_coverage, for K 31 and 32."""
    rnd = random.Random(5)
    checked = emptied = 0
    for _ in range(120):
        mc = rnd.choice((2, 3, 5, 8))
        rows = _group(rnd, mc)
        for K in (31, 32):
            d = S.decision([r.encode() for r in rows], mc, K)
            c = minimizer_counts(rows, K)
            assert d.distinct == len(c) and d.max_count == max(c.values(), default=0)
            if d.max_runs <= S.LIST_CAP and d.distinct <= S.CLAIM_CAP:
                assert (d.verdict == "emptied") == (d.max_count < mc)
                checked += 1
                emptied += d.verdict == "emptied"
            else:
                assert d.verdict == "kept"
    assert checked > 150 and emptied > 20, (checked, emptied)
