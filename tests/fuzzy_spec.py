"""The fuzzy grammar restated in plain Python, independently of the library:
a parser of pattern text, a byte-wise matcher, and the seeded case builders of the families
that tests/test_fuzzy_spec.py (CPU) and tests/test_gpu_fuzzy_programs.py (GPU) share.

The matcher is deliberately the slow way: it tries every start offset and every alternative,
atom by atom. It has no window, no prefilter and no reference run, the three shortcuts of
fuzzy.hip, so it cannot share a mistake with them.

Rules. The match of a row starts at the smallest byte offset on a code-point boundary at
which some alternative matches; among those the first alternative in program order wins;
an OPT first takes one code point and gives it back only if the rest then fails; a wildcard
takes any code point but "\\n"; a code point cut by the row's end does not match.

Rows, literals and replacements are ``bytes``. An alternative is a tuple of atoms: 0..255 a
literal byte, ``ANY``, ``OPT``. numpy and the standard library only.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

ANY, OPT = 256, 257
MAX_ALTS, MAX_ATOMS = 512, 16 * 1024  # fuzzy.hip: kMaxAlts, kMaxAtoms

WIDE = ("A", "é", "€", "😀")  # code points of 1, 2, 3 and 4 bytes
ALPHABET = ("A", "C", "G", "T", "é", "€", "😀", "\n")


class Unsupported(ValueError):
    """Pattern text outside the grammar or a program past its caps."""


# ------------------------------------------------------------------ parser
def _is_alnum(c: int) -> bool:
    return 0x30 <= c <= 0x39 or 0x41 <= c <= 0x5A or 0x61 <= c <= 0x7A


def _finish(alts):
    keep = []
    for a, alt in enumerate(alts):
        if not any(t != OPT for t in alt):
            raise Unsupported(f"alternative {a} can match the empty string")
        if sum(t == OPT for t in alt) > 1:
            raise Unsupported(f"alternative {a} has more than one optional wildcard")
        if alt not in keep:
            keep.append(alt)
    atoms = sum(len(a) for a in keep)
    if len(keep) > MAX_ALTS or atoms > MAX_ATOMS:
        raise Unsupported(f"{len(keep)} alternatives and {atoms} atoms (at most {MAX_ALTS} and {MAX_ATOMS})")
    return keep


def parse(pattern) -> list:
    """Pattern text -> the alternatives in program order, duplicates of an earlier one dropped."""
    p = pattern.encode() if isinstance(pattern, str) else bytes(pattern)
    alts, cur, i = [], [], 0
    while i < len(p):
        c = p[i]
        if c == 0x7C:  # |
            alts.append(tuple(cur))
            cur = []
            i += 1
        elif _is_alnum(c):
            cur.append(c)
            i += 1
        elif c == 0x2E:  # .
            if p[i + 1:i + 2] == b"?":
                cur.append(OPT)
                i += 2
            elif p[i + 1:i + 6] == b"{0,1}":
                cur.append(OPT)
                i += 6
            else:
                cur.append(ANY)
                i += 1
        else:
            raise Unsupported(f"byte {i} (0x{c:02x}) is outside the grammar")
    alts.append(tuple(cur))
    return _finish(alts)


def literal(pattern) -> list:
    """A literal=True pattern: one alternative of its bytes."""
    p = pattern.encode() if isinstance(pattern, str) else bytes(pattern)
    if not p:
        raise Unsupported("an empty literal pattern")
    return _finish([tuple(p)])


def render(alts) -> str:
    """What `describe` gives: '.' for ANY, '?' for OPT, alternatives joined by '|'."""
    raw = b"|".join(bytes(0x2E if t == ANY else 0x3F if t == OPT else t for t in alt) for alt in alts)
    return raw.decode("utf-8", "replace")


# ------------------------------------------------------------------ matcher
def cp_len(lead: int) -> int:
    return 1 if lead < 0x80 else 2 if lead < 0xE0 else 3 if lead < 0xF0 else 4


def _walk(alt, row, pos, take_opt):
    """The alternative from `pos` on with its OPT (if any) taking a code point or not:
    (end, widths of the wildcards) or None."""
    n = len(row)
    widths = []
    for t in alt:
        if t < 256:
            if pos >= n or row[pos] != t:
                return None
            pos += 1
        elif t == OPT and not take_opt:
            widths.append(0)
        else:
            if pos >= n or row[pos] == 0x0A:
                return None
            w = cp_len(row[pos])
            if pos + w > n:
                return None
            widths.append(w)
            pos += w
    return pos, tuple(widths)


def match_at(alt, row, pos):
    """An alternative holds at most one OPT, so greedy-then-empty is two straight walks."""
    got = _walk(alt, row, pos, True)
    if got is None and OPT in alt:
        got = _walk(alt, row, pos, False)
    return got


def search(alts, row, start=0):
    """(begin, end, alt_index, widths) of the leftmost-first match at or after `start`, or None."""
    for b in range(start, len(row)):
        if row[b] & 0xC0 == 0x80:
            continue
        for a, alt in enumerate(alts):
            got = match_at(alt, row, b)
            if got is not None:
                return b, got[0], a, got[1]
    return None


def matches(alts, row, replace_all=True):
    out, pos = [], 0
    while True:
        m = search(alts, row, pos)
        if m is None:
            return out
        out.append(m)
        pos = m[1]
        if not replace_all:
            return out


def contains(alts, row) -> bool:
    return search(alts, row) is not None


def _replace(alts, row, repl, replace_all):
    out, pos = [], 0
    for b, e, _, _ in matches(alts, row, replace_all):
        out += [row[pos:b], repl]
        pos = e
    return b"".join(out) + row[pos:]


def replace(alts, row, repl) -> bytes:
    return _replace(alts, row, repl, False)


def replace_all(alts, row, repl) -> bytes:
    return _replace(alts, row, repl, True)


def shared_prefixes(alts):
    """(index of the reference alternative, per alternative `sp`): build_blob's reference run is
    the first longest run of leading literals; sp counts the leading literals an alternative
    shares with it at the same positions."""

    def lit_run(alt):
        k = 0
        while k < len(alt) and alt[k] < 256:
            k += 1
        return k

    ref = max(range(len(alts)), key=lambda a: (lit_run(alts[a]), -a))
    run = alts[ref][:lit_run(alts[ref])]
    sps = []
    for alt in alts:
        sp = 0
        while sp < len(alt) and sp < len(run) and alt[sp] == run[sp]:
            sp += 1
        sps.append(sp)
    return ref, sps


# ------------------------------------------------------------------ case builders
# A Case is one program and its rows. `program` is pattern text (str), or the literal's bytes
# when `is_literal`. `notes[i]` says what row i was built as (a tuple, family specific).
Case = namedtuple("Case", "program is_literal rows notes")


def alts_of(case):
    return literal(case.program) if case.is_literal else parse(case.program)


def instantiate(alt, fills, take_opt=True):
    """The bytes of an alternative with wildcard k holding the code point fills[k] (str); an OPT
    is left out when take_opt is false."""
    out, k = [], 0
    for t in alt:
        if t < 256:
            out.append(bytes([t]))
        else:
            if t == ANY or take_opt:
                out.append(fills[k].encode())
            k += 1
    return b"".join(out)


def _text(alt) -> str:
    return "".join("." if t == ANY else ".?" if t == OPT else chr(t) for t in alt)


def _word(rng, lo, hi):
    return [ord(c) for c in rng.choice(list("ACGT"), int(rng.integers(lo, hi + 1)))]


def _general_program(rng):
    base = _word(rng, 8, 24)
    n_alt = int(rng.integers(2, 7))
    n_other = 1 if n_alt < 4 else int(rng.integers(1, 3))
    alts = []
    for a in range(n_alt):
        if a < n_alt - n_other:
            alt = base[:int(rng.integers(4, len(base) + 1))] + _word(rng, 0, 6)
        else:
            alt = _word(rng, 4, 12)
        alt = [ANY if rng.random() < 0.12 else t for t in alt]
        alts.append(alt)
    if rng.random() < 0.7:
        alt = alts[int(rng.integers(n_alt))]
        alt[int(rng.integers(len(alt)))] = OPT
    order = rng.permutation(n_alt)
    return [tuple(alts[i]) for i in order]


def _general_alts(rng):
    """A program that meets the per-program conditions, by rejection."""
    while True:
        alts = _general_program(rng)
        if len(set(alts)) != len(alts) or any(all(t >= 256 for t in a) for a in alts):
            continue
        _, sps = shared_prefixes(alts)
        if any(0 < sp < len(a) for sp, a in zip(sps, alts)) and 0 in sps:
            return alts


GENERAL_SEEDS = tuple(range(60))
_ROW_WEIGHTS = np.array([4, 4, 4, 4, 2, 2, 2, 1], dtype=float) / 23


def general(seed) -> Case:
    """2-6 alternatives cut from one base word plus one or two unrelated ones; 60 rows over
    ALPHABET with 0-2 planted instantiations, half of them one code point off.
    notes[i]: the plants of row i as (byte offset, alternative, fills, took the OPT)."""
    rng = np.random.default_rng(7000 + seed)
    alts = _general_alts(rng)
    rows, notes = [], []
    for _ in range(60):
        L = int(rng.integers(0, 201))
        cps = [str(c) for c in rng.choice(ALPHABET, L, p=_ROW_WEIGHTS)] if L else []
        plants = []
        for _ in range(int(rng.integers(0, 3))):
            a = int(rng.integers(len(alts)))
            alt = alts[a]
            take = bool(rng.random() < 0.5)
            fills = [str(c) for c in rng.choice(ALPHABET, sum(t >= 256 for t in alt))]
            inst, k = [], 0
            for t in alt:
                if t < 256:
                    inst.append(chr(t))
                else:
                    if t == ANY or take:
                        inst.append(fills[k])
                    k += 1
            if rng.random() < 0.5:  # a near miss: one further substituted code point
                q = int(rng.integers(len(inst)))
                inst[q] = str(rng.choice([c for c in ALPHABET if c != inst[q]]))
                fills = None
            at = int(rng.integers(0, len(cps) + 1))
            cps[at:at] = ["".join(inst)]
            plants.append([at, a, fills, take])
        # code-point positions -> byte offsets (a later plant shifts an earlier one behind it)
        offs = np.concatenate([[0], np.cumsum([len(c.encode()) for c in cps])])
        done = []
        for i, (at, a, fills, take) in enumerate(plants):
            for later in plants[i + 1:]:
                at += later[0] <= at
            done.append((int(offs[at]), a, None if fills is None else tuple(fills), take))
        rows.append("".join(cps).encode())
        notes.append(tuple(done))
    return Case("|".join(_text(a) for a in alts), False, rows, notes)


# Pairs of programs that hold the same alternatives in the two orders. Under leftmost-first the
# first alternative that matches at a start wins, so A|AB never uses AB. For AC.?|ACG and
# A.C|A.?C the two orders CANNOT give different output: wherever ACG matches, AC.? (greedy)
# matches the same bytes, and wherever A.C matches, A.?C (greedy) does too, so only the winning
# alternative's index differs. The last two pairs are the wildcard forms where the order does
# show in the output.
ORDER_PAIRS = (
    ("A|AB", "AB|A", True),
    ("AC.?|ACG", "ACG|AC.?", False),
    ("A.C|A.?C", "A.?C|A.C", False),
    ("AC.?|ACGT", "ACGT|AC.?", True),
    ("A.C|A.?CG", "A.?CG|A.C", True),
)
ORDER_ROWS = tuple(s.encode() for s in (
    "AB", "A", "B", "", "xABAB", "ABA", "BAAB", "ACG", "ACGT", "ACT", "AC", "AC\n", "AC\nG", "ACGACG", "ACéACGT",
    "AC😀", "ACC", "ACCG", "AC", "AGC", "A€C", "A€CG", "ACG", "A\nC", "ACCGACCG", "xACCGxACGTxAB", "AéCGAB",
    "TTACGTACGTT", "ABABABABABABABABABABABABABABABABABABABABABABABABABABABABABABABABABAB",
))


def order(k) -> tuple:
    """Pair k of ORDER_PAIRS as two cases over ORDER_ROWS."""
    one, two, _ = ORDER_PAIRS[k]
    notes = [()] * len(ORDER_ROWS)
    return Case(one, False, list(ORDER_ROWS), notes), Case(two, False, list(ORDER_ROWS), notes)


# ---- far window
FAR_STARTS = (0, 1, 63, 64, 127)  # lanes 0, 1, 63 of the first chunk and 0, 63 of the second
FAR_EDGES = (255, 256, 257)  # chunk-relative: the window's last byte, the first two past it
FAR_KINDS = ("literal", "dots", "shared")
_FAR_DOTS = (5, 60, 130, 170, 230, 285)


def _acgt(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))


def _other(b: int) -> int:
    return b"CGTA"[b"ACGT".index(bytes([b]))]


def _far_program(kind, rng):
    if kind == "literal":
        return _acgt(rng, 320)
    if kind == "dots":
        w = list(_acgt(rng, 300))
        return "".join("." if i in _FAR_DOTS else chr(c) for i, c in enumerate(w))
    head = _acgt(rng, 250)
    tails = (_acgt(rng, 20), _acgt(rng, 50), _acgt(rng, 35))
    # the tails differ in their first letter, so the alternatives part at atom 250
    tails = tuple(bytes([b"ACG"[i]]) + t[1:] for i, t in enumerate(tails))
    return "|".join((head + t).decode() for t in tails)


def far_window(kind) -> Case:
    """A match that ends past the 256-byte window of its chunk. notes[i] = (what, start offset,
    chunk-relative offset of the changed byte or None / "last", instantiated alternative);
    what: "exact", "miss" (one literal byte changed), "twice" (two instantiations back to
    back after an odd prefix), "twice-miss" (the second with its last byte changed)."""
    rng = np.random.default_rng(9100 + FAR_KINDS.index(kind))
    prog = _far_program(kind, rng)
    alts = literal(prog) if kind == "literal" else parse(prog)
    insts = []  # (alternative, bytes)
    if kind == "dots":
        insts = [(0, instantiate(alts[0], ["é"] * 6)), (0, instantiate(alts[0], ["😀"] * 6)),
                 (0, instantiate(alts[0], ["A", "é", "€", "😀", "T", "é"]))]
    else:
        insts = [(a, instantiate(alt, [])) for a, alt in enumerate(alts)]
    wild = []  # per instantiation: the byte offsets that belong to a wildcard's code point
    for a, inst in insts:
        m = match_at(alts[a], inst, 0)
        assert m is not None and m[0] == len(inst)
        pos, k, taken = 0, 0, set()
        for t in alts[a]:
            w = 1 if t < 256 else m[1][k]
            if t >= 256:
                taken |= set(range(pos, pos + w))
                k += 1
            pos += w
        wild.append(taken)
    rows, notes = [], []

    def add(what, start, edge, a, body):
        total = int(rng.integers(600, 1301))
        rows.append(_acgt(rng, start) + body + _acgt(rng, max(total - start - len(body), 0)))
        notes.append((what, start, edge, a))

    for start in FAR_STARTS:
        c = start - start % 64
        for (a, inst), taken in zip(insts, wild):
            add("exact", start, None, a, inst)
            for edge in FAR_EDGES + ("last",):
                q = len(inst) - 1 if edge == "last" else c + edge - start
                assert 0 <= q < len(inst) and q not in taken, (kind, start, edge)
                add("miss", start, edge, a, inst[:q] + bytes([_other(inst[q])]) + inst[q + 1:])
    for prefix in (33, 97):
        for a, inst in insts:
            add("twice", prefix, None, a, inst + inst)
            add("twice-miss", prefix, "last", a, inst + inst[:-1] + bytes([_other(inst[-1])]))
    return Case(prog, kind == "literal", rows, notes)


# ---- wide code points
WIDE_KINDS = (".", ".?")
WIDE_J = tuple(range(9))
WIDE_STARTS = (0, 61)
_LETTERS = "ABCDEFGHIJKLMNOP"


def wide_text(kind, j) -> str:
    return _LETTERS[:j] + kind + _LETTERS[j + 1:]


def wide(kind, j) -> Case:
    """The 16-atom alternative with its wildcard at atom j, against code points of 1-4 bytes
    there. notes[i] = (what, start offset, width): "match", "after" (the literal right after
    the wildcard wrong), "last" (the last literal wrong), "absent" (no code point at the
    wildcard), "newline", "cut" (the row ends inside the wildcard's code point or one byte
    before the alternative's end)."""
    rng = np.random.default_rng(9300 + 16 * WIDE_KINDS.index(kind) + j)
    pre, post = _LETTERS[:j].encode(), _LETTERS[j + 1:].encode()
    rows, notes = [], []

    def add(what, width, body, tail=True):
        for start in WIDE_STARTS:
            fill = bytes(rng.choice(np.frombuffer(b"xyz", np.uint8), start))
            rows.append(fill + body + (b"xy" if tail and start == 0 else b""))
            notes.append((what, start, width))

    for width, ch in enumerate(WIDE, 1):
        w = ch.encode()
        add("match", width, pre + w + post)
        add("after", width, pre + w + b"q" + post[1:])
        add("last", width, pre + w + post[:-1] + b"q")
        add("cut", width, pre + w + post[:-1], tail=False)
        if width > 1:
            add("cut", width, pre + w[:-1], tail=False)
    add("absent", 0, pre + post)
    add("newline", 1, pre + b"\n" + post)
    return Case(wide_text(kind, j), False, rows, notes)


def wide_combined() -> Case:
    """All 18 alternatives as one program over the rows of every cell."""
    cases = [wide(kind, j) for kind in WIDE_KINDS for j in WIDE_J]
    return Case("|".join(c.program for c in cases), False, [r for c in cases for r in c.rows],
                [n for c in cases for n in c.notes])


# ---- caps
def caps_alts(n_alts=MAX_ALTS, length=32, seed=512):
    """n_alts distinct words of `length` bases."""
    rng = np.random.default_rng(seed)
    seen, out = set(), []
    while len(out) < n_alts:
        w = _acgt(rng, length).decode()
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out


def caps_many() -> Case:
    """512 alternatives of 32 atoms: both caps at once. notes[i] = (alternative or None, "exact" / "miss")."""
    words = caps_alts()
    rng = np.random.default_rng(513)
    rows, notes = [], []
    for r in range(48):
        a = (0, 255, 511, None)[r % 4]
        row = bytearray(_acgt(rng, int(rng.integers(40, 121))))
        what = "exact"
        if a is not None:
            w = bytearray(words[a].encode())
            if r % 8 >= 4:
                w[-1 if r % 16 < 8 else 17] = _other(w[-1 if r % 16 < 8 else 17])
                what = "miss"
            at = int(rng.integers(0, len(row) - 32 + 1))
            row[at:at + 32] = w
        rows.append(bytes(row))
        notes.append((a, what))
    return Case("|".join(words), False, rows, notes)


def caps_long() -> Case:
    """4 alternatives of 4,096 atoms (the atoms cap with few alternatives); they share their
    first 3,000 atoms and the last holds one '.'. notes[i] = (alternative or None, what)."""
    rng = np.random.default_rng(4096)
    head = _acgt(rng, 3000).decode()
    words = [head + "ACGT"[a] + _acgt(rng, 1095).decode() for a in range(4)]
    words[3] = words[3][:3500] + "." + words[3][3501:]
    alts = parse("|".join(words))
    full = instantiate(alts[3], ["€"])
    rows = [_acgt(rng, 70) + full + _acgt(rng, 9),
            _acgt(rng, 70) + full[:-1] + bytes([_other(full[-1])]) + _acgt(rng, 9),
            _acgt(rng, 200) + full[:2000],
            instantiate(alts[1], [])]
    return Case("|".join(words), False, rows, [(3, "exact"), (3, "miss"), (None, "cut"), (1, "exact")])


# ------------------------------------------------------------------ expected answers, computed once
Expected = namedtuple("Expected", "contains first all")
REPLACEMENTS = (b"<R>", b"")


@functools.lru_cache(maxsize=None)
def case_of(family, *key) -> Case:
    return {"general": general, "far": far_window, "wide": wide, "wide_combined": wide_combined,
            "caps_many": caps_many, "caps_long": caps_long}[family](*key)


@functools.lru_cache(maxsize=None)
def expected(family, *key, repl=b"<R>") -> Expected:
    """The spec's answers for a case (any test of a session computes them once)."""
    case = case_of(family, *key)
    return expected_of(case, repl)


def expected_of(case, repl=b"<R>") -> Expected:
    alts = alts_of(case)
    found = [matches(alts, row) for row in case.rows]
    first, every = [], []
    for row, ms in zip(case.rows, found):
        for dst, use in ((first, ms[:1]), (every, ms)):
            out, pos = [], 0
            for b, e, _, _ in use:
                out += [row[pos:b], repl]
                pos = e
            dst.append(b"".join(out) + row[pos:])
    return Expected([bool(ms) for ms in found], first, every)
