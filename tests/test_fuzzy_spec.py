"""CPU tests of the fuzzy reference (tests/fuzzy_spec.py) and of the families it builds for
tests/test_gpu_fuzzy_programs.py: the spec against Python's `re` (bytes.find / bytes.replace for
a literal), `describe` against the spec's parser, the program's size caps, and the conditions
every family has to meet so that the GPU comparison exercises what it is there for. The
conditions are computed from the spec alone; no GPU is needed.
"""
from __future__ import annotations

import re
from collections import Counter

import pytest

import fuzzy_spec as S
from rogtk_amd import _lib
from rogtk_amd.strings import FuzzyProgram


def all_cases():
    """(name, case) of every program of the families."""
    out = [(("general", s), S.case_of("general", s)) for s in S.GENERAL_SEEDS]
    for k in range(len(S.ORDER_PAIRS)):
        one, two = S.order(k)
        out += [(("order", k, 0), one), (("order", k, 1), two)]
    out += [(("far", kind), S.case_of("far", kind)) for kind in S.FAR_KINDS]
    out += [(("wide", kind, j), S.case_of("wide", kind, j)) for kind in S.WIDE_KINDS for j in S.WIDE_J]
    out += [(("wide_combined",), S.case_of("wide_combined")), (("caps_many",), S.case_of("caps_many")),
            (("caps_long",), S.case_of("caps_long"))]
    return out


def _expected(name, case, repl=b"<R>"):
    if name[0] == "order":
        return S.expected_of(case, repl)
    return S.expected(*name, repl=repl)


def _decodes(row):
    try:
        row.decode()
        return True
    except UnicodeDecodeError:
        return False


# ------------------------------------------------------------------ the spec against re
def test_spec_known_answers():
    """The table of tests/test_fuzzy.py (target ACGT) and the rules one by one."""
    alts = S.parse("ACGT|.{0,1}CGT|A.{0,1}GT|AC.{0,1}T|ACG.{0,1}|ACG.")
    assert S.render(alts) == "ACGT|?CGT|A?GT|AC?T|ACG?|ACG."
    for row, first, every in [("TTACGTT", "TT<R>T", "TT<R>T"), ("GCGTA", "<R>A", "<R>A"), ("ACG", "<R>", "<R>"),
                              ("AXCGT", "A<R>", "A<R>"), ("AC\nGT", "AC\nGT", "AC\nGT"), ("AéGT", "<R>", "<R>"),
                              ("ACGTACGT", "<R>ACGT", "<R><R>"), ("AGTAGT", "<R>AGT", "<R><R>")]:
        assert S.replace(alts, row.encode(), b"<R>") == first.encode(), row
        assert S.replace_all(alts, row.encode(), b"<R>") == every.encode(), row
    assert S.search(S.parse("A.?C"), "xA€CAC".encode()) == (1, 6, 0, (3,))
    assert S.search(S.parse("A.?C"), b"xACAC") == (1, 3, 0, (0,))  # takes C, fails on A, gives it back
    assert S.search(S.parse("A.?C|AC"), b"xAC", 2) is None
    assert S.search(S.parse("A|AB"), b"AB")[:3] == (0, 1, 0) and S.search(S.parse("AB|A"), b"AB")[:3] == (0, 2, 0)
    assert S.search(S.parse("A."), "A€".encode()[:3]) is None  # a code point cut by the row's end
    assert S.search(S.parse(".B"), "€B".encode(), 1) is None  # no start inside a code point
    assert S.parse("A.C|A.?C|A.{0,1}C|AC.") == [(65, S.ANY, 67), (65, S.OPT, 67), (65, 67, S.ANY)]
    for bad in ("A(C|G)", "A.?.?C", "AC||GT", "", "A.??C"):
        with pytest.raises(S.Unsupported):
            S.parse(bad)


@pytest.mark.parametrize("repl", S.REPLACEMENTS)
def test_spec_equals_re_on_every_family(repl):
    checked = 0
    for name, case in all_cases():
        exp = _expected(name, case, repl)
        assert len(exp.contains) == len(case.rows) == len(case.notes), name
        if case.is_literal:
            for i, row in enumerate(case.rows):
                assert exp.contains[i] == (row.find(case.program) >= 0), (name, i)
                assert exp.first[i] == row.replace(case.program, repl, 1), (name, i)
                assert exp.all[i] == row.replace(case.program, repl), (name, i)
            checked += len(case.rows)
            continue
        rx = re.compile(case.program)
        r = repl.decode()
        for i, row in enumerate(case.rows):
            if not _decodes(row):  # a row that ends inside a code point: no text for `re` to read
                assert case.notes[i][0] == "cut", (name, i)
                continue
            s = row.decode()
            assert exp.contains[i] == (rx.search(s) is not None), (name, i)
            assert exp.first[i] == rx.sub(lambda m: r, s, count=1).encode(), (name, i)
            assert exp.all[i] == rx.sub(lambda m: r, s).encode(), (name, i)
            checked += 1
    assert checked > 5000


def test_a_row_cut_inside_a_code_point_does_not_match():
    """The rows `re` cannot read: the spec's own rule, by construction of the rows."""
    n = 0
    for kind in S.WIDE_KINDS:
        for j in S.WIDE_J:
            case, exp = S.case_of("wide", kind, j), S.expected("wide", kind, j)
            for row, note, hit in zip(case.rows, case.notes, exp.contains):
                if not _decodes(row):
                    assert note[0] == "cut" and not hit
                    n += 1
    assert n == 2 * 9 * 3 * 2


# ------------------------------------------------------------------ describe
def test_describe_equals_the_spec_parser():
    for name, case in all_cases():
        want = S.render(S.alts_of(case))
        assert FuzzyProgram.pattern(case.program, literal=case.is_literal).describe() == want, name
    dup = "AC.G|AC.{0,1}G|AC.G|AC.?G|ACG"
    assert FuzzyProgram.pattern(dup).describe() == S.render(S.parse(dup)) == "AC.G|AC?G|ACG"


# ------------------------------------------------------------------ caps
def _unsupported(fn):
    with pytest.raises(_lib.RogtkError) as ei:
        fn()
    assert ei.value.code == _lib.ROGTK_E_UNSUPPORTED, str(ei.value)
    return str(ei.value).split("] ", 1)[1]


def test_program_at_its_caps_compiles():
    words = S.caps_alts()
    assert len(set(words)) == S.MAX_ALTS == 512 and sum(map(len, words)) == S.MAX_ATOMS == 16384
    text = "|".join(words)
    assert FuzzyProgram.pattern(text).describe() == text == S.render(S.parse(text))
    # duplicates count towards neither cap: 600 alternatives, 512 of them distinct
    more = "|".join(words[:300] + words[:88] + words[300:])
    assert more.count("|") == 599
    assert FuzzyProgram.pattern(more).describe() == text == S.render(S.parse(more))
    long = S.case_of("caps_long").program
    assert [len(a) for a in S.parse(long)] == [4096] * 4
    assert FuzzyProgram.pattern(long).describe() == S.render(S.parse(long))


@pytest.mark.parametrize("name,text,needles", [
    ("513 alternatives", lambda: "|".join(S.caps_alts(513, 8)), ("513 alternatives", "4104 atoms", "512", "16384")),
    ("16,385 atoms", lambda: "|".join(S.caps_alts()) + "A", ("512 alternatives", "16385 atoms", "512", "16384")),
    ("one alternative of 16,385 atoms", lambda: "A" * 16385, ("1 alternatives", "16385 atoms", "16384")),
    # the per-alternative length check (16-bit packing) never decides under the atoms cap: it
    # only names the reason first, from 65,535 atoms on
    ("one alternative of 65,534 atoms", lambda: "A" * 65534, ("1 alternatives", "65534 atoms", "16384")),
    ("one alternative of 65,535 atoms", lambda: "A" * 65535, ("alternative 0 is too long",)),
])
def test_one_past_a_cap_is_refused(name, text, needles):
    """In the style of test_unsupported_cases_are_refused: the code and a message that names
    both counts and both caps."""
    t = text()
    msg = _unsupported(lambda: FuzzyProgram.pattern(t))
    for needle in needles:
        assert needle in msg, (name, needle, msg)
    with pytest.raises(S.Unsupported):
        S.parse(t)


# ------------------------------------------------------------------ family conditions
def test_general_family_conditions():
    rows = matched = later = first = many = blocked = 0
    widths, opts = Counter(), Counter()
    for seed in S.GENERAL_SEEDS:
        case = S.case_of("general", seed)
        alts = S.alts_of(case)
        assert 2 <= len(alts) <= 6 and len(case.rows) == 60
        _, sps = S.shared_prefixes(alts)
        assert any(0 < sp < len(a) for sp, a in zip(sps, alts)) and 0 in sps, seed
        for row, plants in zip(case.rows, case.notes):
            assert len(row.decode()) <= 200 + 2 * 31
            ms = S.matches(alts, row)
            rows += 1
            matched += bool(ms)
            many += len(ms) >= 2
            for b, e, a, ws in ms:
                later += a > 0
                first += a == 0
                widths.update(ws)
                if S.OPT in alts[a]:
                    k = sum(t >= 256 for t in alts[a][:alts[a].index(S.OPT)])
                    opts[ws[k] > 0] += 1
            for at, a, fills, take in plants:
                # an exact plant with "\n" under a wildcard: the alternative fails at its own
                # place, and holds there once the "\n" is another one-byte code point
                if fills is None or S.match_at(alts[a], row, at) is not None:
                    continue
                inst = S.instantiate(alts[a], fills, take)
                assert row[at:at + len(inst)] == inst
                if b"\n" in inst:
                    mended = row[:at] + inst.replace(b"\n", b"N") + row[at + len(inst):]
                    blocked += S.match_at(alts[a], mended, at) is not None
    assert rows == 3600
    assert 0.25 <= matched / rows <= 0.75, matched / rows
    assert later >= 200 and first >= 200, (later, first)
    assert many >= 100, many
    for w in range(5):
        assert widths[w] >= 20, (w, widths)
    assert opts[False] >= 20 and opts[True] >= 20, opts
    assert blocked >= 20, blocked


def test_order_family_conditions():
    for k, (one, two, differs) in enumerate(S.ORDER_PAIRS):
        a, b = S.order(k)
        assert (a.program, b.program) == (one, two)
        assert sorted(S.alts_of(a)) == sorted(S.alts_of(b)) and S.alts_of(a) != S.alts_of(b)
        for repl in S.REPLACEMENTS:
            ea, eb = S.expected_of(a, repl), S.expected_of(b, repl)
            assert ea.contains == eb.contains and any(ea.contains) and not all(ea.contains)
            if differs:
                assert sum(x != y for x, y in zip(ea.all, eb.all)) >= 2, (k, repl)
            else:
                # no row can tell these two orders apart (fuzzy_spec.ORDER_PAIRS): what differs
                # is the alternative that wins
                assert ea.all == eb.all and ea.first == eb.first
        wa = [[m[2] for m in S.matches(S.alts_of(a), r)] for r in a.rows]
        wb = [[m[2] for m in S.matches(S.alts_of(b), r)] for r in b.rows]
        assert sum(x != y for x, y in zip(wa, wb)) >= 2, k


def test_far_window_family_conditions():
    for kind in S.FAR_KINDS:
        case, exp = S.case_of("far", kind), S.expected("far", kind)
        alts = S.alts_of(case)
        assert all(600 <= len(r) <= 1300 for r in case.rows)
        assert max(map(len, alts)) >= (320 if kind == "literal" else 300)
        if kind == "dots":
            assert len(alts) == 1 and len(alts[0]) == 300 and sum(t == S.ANY for t in alts[0]) == 6
        if kind == "shared":
            assert len(alts) == 3 and all(a[:250] == alts[0][:250] for a in alts)
            assert len({a[250] for a in alts}) == 3
        seen = set()
        for row, (what, start, edge, a), hit, every in zip(case.rows, case.notes, exp.contains, exp.all):
            ms = S.matches(alts, row)
            if what == "exact":
                assert len(ms) == 1 and ms[0][0] == start and ms[0][2] == a
                assert ms[0][1] - start > 256  # it ends past the window of its chunk
                if kind == "dots":
                    seen.add(("widths", max(ms[0][3])))
            elif what == "miss":
                assert ms == []
            elif what == "twice":
                # the second search starts where the first match ended: not at a chunk's edge
                assert [m[0] for m in ms] == [start, ms[0][1]] and ms[0][1] % 64 and every.count(b"<R>") == 2
                seen.add(("from", ms[0][1] % 4))
            else:
                assert [m[0] for m in ms] == [start] and every.count(b"<R>") == 1
            seen.add((what, start, edge, hit))
        for start in S.FAR_STARTS:
            assert ("exact", start, None, True) in seen, (kind, start)
            for edge in S.FAR_EDGES + ("last",):
                assert ("miss", start, edge, False) in seen, (kind, start, edge)
        assert {s for s in seen if s[0] == "twice"} and {s for s in seen if s[0] == "twice-miss"}
        assert {("from", 1), ("from", 3)} & seen  # and at an odd offset in some row
        if kind == "dots":
            assert {("widths", 2), ("widths", 4)} <= seen


def test_wide_family_conditions():
    cells = set()
    for kind in S.WIDE_KINDS:
        for j in S.WIDE_J:
            case, exp = S.case_of("wide", kind, j), S.expected("wide", kind, j)
            alts = S.alts_of(case)
            assert len(alts) == 1 and len(alts[0]) == 16 and alts[0][j] == (S.ANY if kind == "." else S.OPT)
            for row, (what, start, width), hit in zip(case.rows, case.notes, exp.contains):
                # with the wildcard in front (j = 0) and nothing planted for it, it takes the
                # filler byte before the start offset instead
                filler = what == "absent" and j == 0 and start > 0
                # and a leading ".?" steps over the "\n": the match starts after it
                skipped = what == "newline" and j == 0 and kind == ".?"
                want = what == "match" or (what == "absent" and kind == ".?") or filler or skipped
                assert hit == want, (kind, j, what, width, start)
                if hit:
                    m = S.search(alts, row)
                    assert (m[0], m[3]) == ((start - 1, (1,)) if filler else (start + 1, (0,)) if skipped
                                            else (start, (width,)))
                cells.add((kind, j, width, what, start))
    for kind in S.WIDE_KINDS:
        for j in S.WIDE_J:
            for start in S.WIDE_STARTS:
                for width in (1, 2, 3, 4):
                    for what in ("match", "after", "last", "cut"):
                        assert (kind, j, width, what, start) in cells
                assert (kind, j, 0, "absent", start) in cells and (kind, j, 1, "newline", start) in cells
    # the combined program answers every row as the row's own program does: no alternative of
    # another cell matches it first
    comb, exp = S.case_of("wide_combined"), S.expected("wide_combined")
    assert len(S.alts_of(comb)) == 18
    own = [h for kind in S.WIDE_KINDS for j in S.WIDE_J for h in S.expected("wide", kind, j).contains]
    assert len(own) == len(comb.rows)
    assert sum(exp.contains) >= sum(own) and 0.1 < sum(exp.contains) / len(own) < 0.9
    ref, sps = S.shared_prefixes(S.alts_of(comb))
    assert sps[ref] == 8 and sorted(set(sps)) == list(range(9))


def test_caps_family_conditions():
    case, exp = S.case_of("caps_many"), S.expected("caps_many")
    alts = S.alts_of(case)
    assert len(alts) == 512 and sum(map(len, alts)) == 16384
    assert len(case.rows) <= 48 and max(map(len, case.rows)) <= 120
    won = Counter()
    for row, (a, what), hit in zip(case.rows, case.notes, exp.contains):
        assert hit == (a is not None and what == "exact")
        if hit:
            won[S.search(alts, row)[2]] += 1
    assert set(won) == {0, 255, 511} and Counter(n for n in case.notes)[(None, "exact")] >= 6
    assert sum(1 for a, what in case.notes if what == "miss") >= 6
    case, exp = S.case_of("caps_long"), S.expected("caps_long")
    assert exp.contains == [True, False, False, True]
    alts = S.alts_of(case)
    assert S.search(alts, case.rows[0]) == (70, 70 + 4098, 3, (3,)) and S.search(alts, case.rows[3])[2] == 1
    assert S.shared_prefixes(alts) == (0, [4096, 3000, 3000, 3000])
