"""The `fuzzy` namespace (rogtk/__init__.py:351-410, src/expressions.rs:983-1216): one-edit
pattern match and replace.

The reference hands a generated pattern to the Rust `regex` crate. The patterns it can
generate are a closed grammar (literals, ".", ".?" / ".{0,1}", "|"), which this project
compiles into a program and matches on the GPU without a regex engine. The yardstick here
is Python's `re` on the pattern text (leftmost-first alternation and "." excluding only
"\\n", as the regex crate documents for itself), plus hand-derived known answers.

CPU tests: the pattern compiler through `describe`, every unsupported case, the plugin's
symbols / fields / kwargs. GPU tests (-m gpu): the eager API, the plugin and the Level-1
device entry points against `re`.
"""
from __future__ import annotations

import ctypes
import itertools
import re
import subprocess

import numpy as np
import pyarrow as pa
import pytest

from rogtk_amd import _lib, plugin
from rogtk_amd.strings import FuzzyNamespace, FuzzyProgram

NATIVE = ("fuzzy_contains_native_expr", "fuzzy_replace_native_expr")
PREGEN = ("fuzzy_contains_expr", "fuzzy_replace_expr")


# ------------------------------------------------------------------ the reference side
def gen_pattern(target, wildcard=".{0,1}", include_original=True, max_length=100):
    """generate_fuzzy_pattern (expressions.rs:983-1013) as text."""
    if not target:
        return target
    fuzz = [target] if include_original else []
    if len(target) <= max_length:
        fuzz += [target[:i] + wildcard + target[i + 1:] for i in range(len(target))]
        fuzz.append(target[:-1] + ".")
    return "|".join(fuzz)


def re_contains(pattern, rows):
    rx = re.compile(pattern)
    return [None if s is None else rx.search(s) is not None for s in rows]


def re_replace(pattern, repl, rows, replace_all):
    rx = re.compile(pattern)
    return [None if s is None else rx.sub(lambda m: repl, s, count=0 if replace_all else 1) for s in rows]


def _as_describe(pattern):
    """The canonical text `describe` gives for a pattern of the grammar (no duplicates)."""
    alts = []
    for a in pattern.split("|"):
        a = a.replace(".{0,1}", "?").replace(".?", "?")
        if a not in alts:
            alts.append(a)
    return "|".join(alts)


# ------------------------------------------------------------------ CPU: the compiler
def test_describe_native_default():
    assert FuzzyProgram.native("ACGT", ".{0,1}", True, 100).describe() == "ACGT|?CGT|A?GT|AC?T|ACG?|ACG."
    assert FuzzyProgram.native("ACGT").describe() == "ACGT|?CGT|A?GT|AC?T|ACG?|ACG."  # None = the defaults
    assert FuzzyProgram.native("ACGT", ".?").describe() == "ACGT|?CGT|A?GT|AC?T|ACG?|ACG."


def test_describe_native_options():
    assert FuzzyProgram.native("ACGT", ".{0,1}", False, 100).describe() == "?CGT|A?GT|AC?T|ACG?|ACG."
    assert FuzzyProgram.native("ACGT", ".{0,1}", True, 3).describe() == "ACGT"
    assert FuzzyProgram.native("ACGT", ".{0,1}", True, 4).describe() == "ACGT|?CGT|A?GT|AC?T|ACG?|ACG."
    # wildcard ".": the last variant equals the end-substitution and is dropped
    assert FuzzyProgram.native("ACGT", ".", True, 100).describe() == "ACGT|.CGT|A.GT|AC.T|ACG."
    assert FuzzyProgram.native("A", ".").describe() == "A|."
    assert FuzzyProgram.native("a0Z9").describe() == "a0Z9|?0Z9|a?Z9|a0?9|a0Z?|a0Z."


def test_describe_native_100_characters():
    t = "".join("ACGT"[(i * 7 + i // 3) % 4] for i in range(100))
    d = FuzzyProgram.native(t).describe().split("|")
    assert len(d) == 102 and d[0] == t and d[-1] == t[:-1] + "."
    assert d[1] == "?" + t[1:] and d[100] == t[:-1] + "?" and all(len(a) == 100 for a in d)


@pytest.mark.parametrize("wildcard", [".{0,1}", ".?", "."])
@pytest.mark.parametrize("include_original", [True, False])
def test_pregenerated_pattern_compiles_to_the_native_program(wildcard, include_original):
    for target in ("AC", "ACGT", "GATTACA01", "ACGT" * 25):
        text = gen_pattern(target, wildcard, include_original, 100)
        want = FuzzyProgram.native(target, wildcard, include_original, 100).describe()
        assert FuzzyProgram.pattern(text).describe() == want == _as_describe(text)


def test_describe_pattern_forms():
    assert FuzzyProgram.pattern("A.C|A.?C|A.{0,1}C|AC.").describe() == "A.C|A?C|AC."
    assert FuzzyProgram.pattern("A.C", literal=True).describe() == "A.C"  # three literal bytes
    assert FuzzyProgram.pattern("é|$", literal=True).describe() == "é|$"


def _unsupported(fn):
    with pytest.raises(_lib.RogtkError) as ei:
        fn()
    assert ei.value.code == _lib.ROGTK_E_UNSUPPORTED, str(ei.value)
    msg = str(ei.value).split("] ", 1)[1]
    assert msg.strip(), "empty message"
    return msg


@pytest.mark.parametrize("name,fn,needle", [
    ("empty target", lambda: FuzzyProgram.native(""), "empty"),
    ("1-character target with .{0,1}", lambda: FuzzyProgram.native("A", ".{0,1}"), "empty string"),
    ("target AC.T", lambda: FuzzyProgram.native("AC.T"), "0x2e"),
    ("target é", lambda: FuzzyProgram.native("é"), "0xc3"),
    ("101-character target", lambda: FuzzyProgram.native("A" * 101), "101"),
    ("wildcard [ACGT]", lambda: FuzzyProgram.native("ACGT", "[ACGT]"), "[ACGT]"),
    ("pattern A(C|G)", lambda: FuzzyProgram.pattern("A(C|G)"), "0x28"),
    ("pattern A.?.?C", lambda: FuzzyProgram.pattern("A.?.?C"), "optional"),
    ("include_original false, max_length < len", lambda: FuzzyProgram.native("ACGT", ".{0,1}", False, 3), "empty"),
    ("regex replacement x$1", lambda: FuzzyProgram.native("ACGT").set_replacement("x$1"), "$"),
    ("empty literal pattern", lambda: FuzzyProgram.pattern("", literal=True), "empty"),
    ("empty pattern", lambda: FuzzyProgram.pattern(""), "empty"),
    ("empty alternative", lambda: FuzzyProgram.pattern("AC||GT"), "empty string"),
    ("lazy quantifier", lambda: FuzzyProgram.pattern("A.??C"), "0x3f"),
])
def test_unsupported_cases_are_refused(name, fn, needle):
    assert needle in _unsupported(fn), name


def test_literal_replacement_may_hold_a_dollar():
    FuzzyProgram.pattern("ACGT", literal=True).set_replacement("x$1")
    FuzzyProgram.native("ACGT").set_replacement("no dollar \\1 here")


# ------------------------------------------------------------------ CPU: the plugin
def test_plugin_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.HIP_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for n in NATIVE + PREGEN:
        assert n in plugin.EXPRESSIONS
        assert "_polars_plugin_" + n in have and "_polars_plugin_field_" + n in have, n
    for n in ("compile_native", "compile_pattern", "set_replacement", "free", "describe", "contains",
              "replace_measure", "replace_fill", "contains_host", "replace_host"):
        assert "rogtk_fuzzy_" + n in have, n


@pytest.mark.parametrize("name,typ", [
    ("fuzzy_contains_native_expr", pa.bool_()), ("fuzzy_replace_native_expr", pa.string_view()),
    ("fuzzy_contains_expr", pa.bool_()), ("fuzzy_replace_expr", pa.string_view()),
])
def test_plugin_output_fields(name, typ):
    f = plugin.call_plugin_field(name, [pa.field("seq", pa.string_view())])
    assert f.name == "seq" and f.type == typ


def test_plugin_kwargs_round_trip():
    kw = {"target": "ACGT", "replacement": "", "wildcard": None, "include_original": False, "max_length": None,
          "replace_all": True, "literal": None}
    lines = dict(ln.split("=", 1) for ln in plugin.kwargs_as_parsed(kw).splitlines())
    assert lines == {"target": "'ACGT'", "replacement": "''", "wildcard": "None", "include_original": "False",
                     "max_length": "None", "replace_all": "True", "literal": "None"}


def _plugin_error(name, inputs, kwargs):
    with pytest.raises(_lib.RogtkError) as ei:
        plugin.call_plugin(name, inputs, kwargs)
    return str(ei.value)


def test_plugin_refuses_unsupported_patterns_with_a_message():
    seq = pa.array(["ACGT"], type=pa.string_view())
    assert "0x28" in _plugin_error("fuzzy_contains_expr", [seq], {"pattern": "A(C|G)", "literal": False})
    assert "[ACGT]" in _plugin_error("fuzzy_contains_native_expr", [seq], {"target": "ACGT", "wildcard": "[ACGT]"})
    assert "'$'" in _plugin_error("fuzzy_replace_native_expr", [seq], {"target": "ACGT", "replacement": "$0"})
    assert "missing field `target`" in _plugin_error("fuzzy_contains_native_expr", [seq], {"wildcard": "."})
    assert "missing field `replacement`" in _plugin_error("fuzzy_replace_expr", [seq], {"pattern": "AC"})
    assert "expected `String`, got `i64`" in _plugin_error("fuzzy_contains_expr", [pa.array([1])], {"pattern": "AC"})


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _check(got: pa.Array, want, what=""):
    g = got.to_pylist()
    assert len(g) == len(want), (what, len(g), len(want))
    for i, (a, b) in enumerate(zip(g, want)):
        assert a == b, (what, i, a, b)


KNOWN = [  # row, replace-first, replace-all (target ACGT, replacement <R>)
    ("TTACGTT", "TT<R>T", "TT<R>T"),
    ("GCGTA", "<R>A", "<R>A"),
    ("CGTA", "<R>A", "<R>A"),
    ("ACGA", "<R>", "<R>"),
    ("ACG", "<R>", "<R>"),
    ("AGT", "<R>", "<R>"),
    ("AXCGT", "A<R>", "A<R>"),
    ("AC\nGT", "AC\nGT", "AC\nGT"),
    ("AéGT", "<R>", "<R>"),
    ("éCGT", "<R>", "<R>"),
    ("ACGTACGT", "<R>ACGT", "<R><R>"),
    ("AGTAGT", "<R>AGT", "<R><R>"),
]


@pytest.mark.gpu
def test_gpu_known_answers(gpu):
    rows = [k[0] for k in KNOWN]
    ns = FuzzyNamespace(pa.array(rows, type=pa.large_string()))
    m = ns.match("ACGT")
    assert m.type == pa.bool_()
    _check(m, [k[0] != k[1] for k in KNOWN], "match")
    first = ns.replace_target("ACGT", "<R>")
    assert first.type == pa.large_string()
    _check(first, [k[1] for k in KNOWN], "first")
    _check(ns.replace_target("ACGT", "<R>", replace_all=True), [k[2] for k in KNOWN], "all")
    # and the table itself agrees with re
    pat = gen_pattern("ACGT")
    assert re_replace(pat, "<R>", rows, False) == [k[1] for k in KNOWN]
    assert re_replace(pat, "<R>", rows, True) == [k[2] for k in KNOWN]


@pytest.mark.gpu
def test_gpu_chunk_boundaries(gpu):
    """Matches that end before, across and after start offset 64 (the lanes of a wave take
    64 consecutive starts), and rows around the multiples of 64."""
    target = "GATTACAGATTACACCGTGA"
    rng = np.random.default_rng(11)
    rows = []
    for off in range(44, 67):
        for t in (target, target[:9] + target[10:]):
            for fill in ("N", "G"):
                rows.append((fill * off + t + fill * 200)[:200])
    for L in (0, 1, 19, 63, 64, 65, 127, 128, 129, 300):
        base = "".join(rng.choice(list("ACGT"), L))
        rows.append(base)
        rows.append((base + target)[-L:] if L else "")  # the target at the very end
        rows.append((base[:max(L - 19, 0)] + target[1:])[:L])  # a deletion at the end (cut when L < 19)
        rows.append("é" * (L // 2) + "A" * (L % 2))
    pat = gen_pattern(target)
    ns = FuzzyNamespace(pa.array(rows, type=pa.large_string()))
    want = re_contains(pat, rows)
    assert sum(want) >= 92  # every planted row of the offset sweep
    _check(ns.match(target), want, "match")
    _check(ns.replace_target(target, "[x]"), re_replace(pat, "[x]", rows, False), "first")
    _check(ns.replace_target(target, "[x]", replace_all=True), re_replace(pat, "[x]", rows, True), "all")


# ---- random rows: the generator of the CPU check that preceded this feature
WILDCARDS = (".{0,1}", ".?", ".")
REPLACEMENTS = ("", "xy", "0123456789" * 4, "é")
ALPHABETS = ("ACGT", "AC", "ACGTN\né")
ROWS_PER_CASE = 84


def _random_cases():
    rng = np.random.default_rng(2024)
    # (wildcard, include_original, max_length above the target length?) without the unsupported
    # include_original = False with max_length below
    configs = [c for c in itertools.product(WILDCARDS, (True, False), (True, False)) if c[1] or c[2]]
    cases = []
    combos = itertools.product((2, 3, 4, 5, 6, 7, 8, 9, 32, 100), ALPHABETS, (True, False))
    for i, (tlen, alphabet, short) in enumerate(combos):
        letters = [c for c in alphabet if c.isascii() and c.isalnum()]
        target = "".join(rng.choice(letters, tlen))
        wildcard, include_original, above = configs[i % len(configs)]
        max_length = (tlen if i % 2 else 100) if above else tlen - 1
        rows = []
        for _ in range(ROWS_PER_CASE):
            L = int(rng.integers(0, 41)) if short else int(rng.integers(100, 301))
            s = list(rng.choice(list(alphabet), L)) if L else []
            if rng.random() < 0.5:
                t = list(target)
                kind, p = int(rng.integers(4)), int(rng.integers(len(t)))
                if kind == 0:
                    t[p] = str(rng.choice(list(alphabet)))  # substitution
                elif kind == 1:
                    del t[p]  # deletion
                elif kind == 2:
                    t.insert(p, str(rng.choice(list(alphabet))))  # insertion
                q = int(rng.integers(0, L + 1))
                s[q:q + len(t)] = t
            rows.append("".join(s))
        cases.append(dict(target=target, wildcard=wildcard, include_original=include_original,
                          max_length=max_length, rows=rows, alphabet=alphabet, short=short, repl=REPLACEMENTS[i % len(REPLACEMENTS)],
                          pattern=gen_pattern(target, wildcard, include_original, max_length)))
    return cases


@pytest.fixture(scope="module")
def random_cases():
    """The cases with their `re` answers, computed once."""
    cases = _random_cases()
    for c in cases:
        c["contains"] = re_contains(c["pattern"], c["rows"])
        c["first"] = re_replace(c["pattern"], c["repl"], c["rows"], False)
        c["all"] = re_replace(c["pattern"], c["repl"], c["rows"], True)
    return cases


def test_random_cases_cover_both_outcomes(random_cases):
    """The condition on the reference side: neither outcome dominates, and every option occurs."""
    flat = [h for c in random_cases for h in c["contains"]]
    assert 4900 <= len(flat) <= 5100
    rate = sum(flat) / len(flat)
    assert 0.30 <= rate <= 0.70, rate
    assert {c["wildcard"] for c in random_cases} == set(WILDCARDS)
    assert {c["include_original"] for c in random_cases} == {True, False}
    assert any(c["max_length"] < len(c["target"]) for c in random_cases)
    assert any(c["max_length"] >= len(c["target"]) for c in random_cases)
    assert {c["repl"] for c in random_cases} == set(REPLACEMENTS)
    assert {len(c["target"]) for c in random_cases} >= {2, 9, 32, 100}
    assert sum(a != b for c in random_cases for a, b in zip(c["first"], c["all"])) > 50  # several matches a row


@pytest.mark.gpu
def test_gpu_random_rows_native(gpu, random_cases):
    for i, c in enumerate(random_cases):
        ns = FuzzyNamespace(pa.array(c["rows"], type=pa.large_string()))
        opts = (c["wildcard"], c["include_original"], c["max_length"])
        _check(ns.match(c["target"], *opts), c["contains"], ("match", i))
        _check(ns.replace_target(c["target"], c["repl"], *opts), c["first"], ("first", i))
        _check(ns.replace_target(c["target"], c["repl"], *opts, replace_all=True), c["all"], ("all", i))


@pytest.mark.gpu
def test_gpu_random_rows_pregenerated_and_literal(gpu, random_cases):
    for i, c in enumerate(random_cases[::3]):
        ns = FuzzyNamespace(pa.array(c["rows"], type=pa.large_string()))
        _check(ns.contains(c["pattern"]), c["contains"], ("contains", i))
        _check(ns.replace(c["pattern"], c["repl"]), c["all"], ("replace", i))
        # literal: str::contains / str::replace of the pattern text and of the target
        for lit in (c["target"][:5], c["pattern"][:7], "é", "\n", "$"):
            _check(ns.contains(lit, literal=True), [lit in s for s in c["rows"]], ("lit contains", i, lit))
            _check(ns.replace(lit, "$é" + c["repl"], literal=True),
                   [s.replace(lit, "$é" + c["repl"]) for s in c["rows"]], ("lit replace", i, lit))


@pytest.mark.gpu
@pytest.mark.parametrize("n_rows", [0, 1, 63, 64, 65, 1000])
def test_gpu_layouts_and_sizes(gpu, n_rows):
    rng = np.random.default_rng(100 + n_rows)
    target, pat = "ACGTTGCA", gen_pattern("ACGTTGCA")
    rows = []
    for r in range(n_rows):
        s = "".join(rng.choice(list("ACGT"), int(rng.integers(0, 90))))
        if r % 2:
            q = int(rng.integers(0, len(s) + 1))
            s = s[:q] + target[:3] + target[4:] + s[q:]
        rows.append(None if r % 7 == 3 else s)
    want_m, want_r = re_contains(pat, rows), re_replace(pat, "-", rows, True)
    for typ in (pa.string(), pa.large_string()):
        arr = pa.array(rows, type=typ)
        ns = FuzzyNamespace(arr)
        got = ns.match(target)
        assert got.null_count == arr.null_count
        _check(got, want_m, ("match", typ))
        got = ns.replace_target(target, "-", replace_all=True)
        assert got.null_count == arr.null_count
        _check(got, want_r, ("replace", typ))
        # a slice with a non-zero offset (offsets, values and validity all shifted)
        big = pa.array(["ACGTTGCA", None, "TT"] + rows + ["ACGTTGCA"] * 2, type=typ).slice(3, n_rows)
        _check(FuzzyNamespace(big).match(target), want_m, ("sliced match", typ))
        _check(FuzzyNamespace(big).replace_target(target, "-", replace_all=True), want_r, ("sliced replace", typ))
    # a chunked column is one column
    if n_rows > 1:
        ch = pa.chunked_array([pa.array(rows[:n_rows // 3], type=pa.string()),
                               pa.array(rows[n_rows // 3:], type=pa.string())])
        _check(FuzzyNamespace(ch).match(target), want_m, "chunked")


@pytest.mark.gpu
def test_gpu_all_null_column(gpu):
    for n in (1, 64, 130):
        arr = pa.array([None] * n, type=pa.large_string())
        ns = FuzzyNamespace(arr)
        assert ns.match("ACGT").to_pylist() == [None] * n
        assert ns.replace_target("ACGT", "x").to_pylist() == [None] * n
        assert ns.contains("AC", literal=True).null_count == n


@pytest.mark.gpu
def test_gpu_col_namespace(gpu):
    import rogtk_amd as rg

    c = rg.col(["TTACGTT", None, "TTTT"])
    assert c.fuzzy.match("ACGT").to_pylist() == [True, None, False]
    assert c.fuzzy.replace_target("ACGT", "").to_pylist() == ["TTT", None, "TTTT"]


def _pick(cases, tlen):
    """A case with that target length, the fuzzy variants on, and both outcomes."""
    for c in cases:
        rate = sum(c["contains"]) / len(c["contains"])
        if len(c["target"]) == tlen and c["max_length"] >= tlen and 0.2 < rate < 0.8:
            return c
    raise AssertionError(f"no such case for target length {tlen}")


def _layouts(values):
    n = len(values)
    cut = [0, n // 3, n // 3, 2 * n // 3, n]  # an empty chunk among them
    out = {t: pa.array(values, type=typ) for t, typ in
           (("view", pa.string_view()), ("utf8", pa.string()), ("large", pa.large_string()))}
    for t, typ in (("view", pa.string_view()), ("utf8", pa.string()), ("large", pa.large_string())):
        out["chunked_" + t] = pa.chunked_array([pa.array(values[a:b], type=typ) for a, b in zip(cut, cut[1:])],
                                               type=typ)
    out["sliced_utf8"] = pa.array(["GG"] * 5 + list(values) + ["TT"], type=pa.string()).slice(5, n)
    return out


@pytest.mark.gpu
def test_gpu_plugin_matches_the_eager_api(gpu, random_cases):
    c = _pick(random_cases, 9)
    rows = list(c["rows"]) + ["ACGTACGTACGTAC", "short", ""]
    for r in range(5, len(rows), 11):
        rows[r] = None
    ns = FuzzyNamespace(pa.array(rows, type=pa.large_string()))
    nat = {"target": c["target"], "wildcard": c["wildcard"], "include_original": c["include_original"],
           "max_length": c["max_length"]}
    lit = c["target"][:4]
    want = {
        "native contains": ns.match(c["target"], c["wildcard"], c["include_original"], c["max_length"]).to_pylist(),
        "native first": ns.replace_target(c["target"], "<é>", c["wildcard"], c["include_original"],
                                          c["max_length"]).to_pylist(),
        "native all": ns.replace_target(c["target"], "<é>", c["wildcard"], c["include_original"], c["max_length"],
                                        replace_all=True).to_pylist(),
        "defaults": ns.match(c["target"]).to_pylist(),
        "contains": ns.contains(c["pattern"]).to_pylist(),
        "replace": ns.replace(c["pattern"], "").to_pylist(),
        "literal contains": ns.contains(lit, literal=True).to_pylist(),
        "literal replace": ns.replace(lit, "$1", literal=True).to_pylist(),
    }
    assert any(want["native contains"]) and not all(x for x in want["native contains"] if x is not None)
    for lname, col in _layouts(rows).items():
        got = {
            "native contains": plugin.call_plugin("fuzzy_contains_native_expr", [col], nat),
            "native first": plugin.call_plugin("fuzzy_replace_native_expr", [col], dict(nat, replacement="<é>")),
            "native all": plugin.call_plugin("fuzzy_replace_native_expr", [col],
                                             dict(nat, replacement="<é>", replace_all=True)),
            # None = the reference's defaults
            "defaults": plugin.call_plugin("fuzzy_contains_native_expr", [col],
                                           {"target": c["target"], "wildcard": None, "include_original": None,
                                            "max_length": None}),
            "contains": plugin.call_plugin("fuzzy_contains_expr", [col], {"pattern": c["pattern"], "literal": None}),
            "replace": plugin.call_plugin("fuzzy_replace_expr", [col], {"pattern": c["pattern"], "replacement": ""}),
            "literal contains": plugin.call_plugin("fuzzy_contains_expr", [col], {"pattern": lit, "literal": True}),
            "literal replace": plugin.call_plugin("fuzzy_replace_expr", [col],
                                                  {"pattern": lit, "replacement": "$1", "literal": True}),
        }
        for k, v in got.items():
            assert v.type == (pa.bool_() if "contains" in k or k == "defaults" else pa.string_view()), (lname, k)
            assert v.to_pylist() == want[k], (lname, k)
    # an unsupported pattern is an error message, not a crash
    assert "0x5b" in _plugin_error("fuzzy_contains_expr", [pa.array(rows, type=pa.string_view())],
                                   {"pattern": "A[CG]T"})


@pytest.mark.gpu
def test_gpu_level1_device_columns(gpu, random_cases):
    """compile -> contains, replace_measure -> replace_fill on device tensors and an explicit
    stream, against the host-column (Level 2) entry points."""
    torch = gpu
    c = _pick(random_cases, 32)
    rows = list(c["rows"])
    for r in range(3, len(rows), 9):
        rows[r] = None
    arr = pa.array(rows, type=pa.large_string())
    n = len(arr)
    prog = FuzzyProgram.native(c["target"], c["wildcard"], c["include_original"], c["max_length"])
    prog.set_replacement("<<>>")
    want_m = prog.contains(arr)
    want_r = prog.replace(arr, True)

    bufs = arr.buffers()
    dev = torch.device("cuda:0")
    offs = torch.from_numpy(np.frombuffer(bufs[1], dtype=np.int64, count=n + 1).copy()).to(dev)
    vals = torch.from_numpy(np.frombuffer(bufs[2], dtype=np.uint8).copy()).to(dev)
    valid = torch.from_numpy(np.frombuffer(bufs[0], dtype=np.uint8).copy()).to(dev)
    col = _lib.StrCol(offs.data_ptr(), 8, vals.data_ptr(), vals.numel(), valid.data_ptr(), 0, n)
    words = (n + 63) // 64
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        bits = torch.zeros(words, dtype=torch.int64, device=dev)
        vbits = torch.zeros(words, dtype=torch.int64, device=dev)
        s = ctypes.c_void_p(stream.cuda_stream)
        _lib.call("rogtk_fuzzy_contains", prog.handle, ctypes.byref(col), bits.data_ptr(), vbits.data_ptr(), s)
        tb = ctypes.c_int64(0)
        _lib.call("rogtk_str_temp_bytes", n, ctypes.byref(tb))
        temp = torch.zeros(tb.value, dtype=torch.uint8, device=dev)
        out_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        rvbits = torch.zeros(words, dtype=torch.int64, device=dev)
        _lib.call("rogtk_fuzzy_replace_measure", prog.handle, ctypes.byref(col), 1, out_off.data_ptr(),
                  rvbits.data_ptr(), temp.data_ptr(), tb.value, s)
        stream.synchronize()
        total = int(out_off[n].item())
        out = torch.zeros(max(total, 1), dtype=torch.uint8, device=dev)
        _lib.call("rogtk_fuzzy_replace_fill", prog.handle, ctypes.byref(col), 1, out_off.data_ptr(),
                  out.data_ptr(), s)
        stream.synchronize()

    def unpack(t):
        return np.unpackbits(t.cpu().numpy().view(np.uint8), bitorder="little")[:n].astype(bool)

    ok = unpack(vbits)
    assert np.array_equal(ok, unpack(rvbits)) and ok.tolist() == [r is not None for r in rows]
    hit = unpack(bits)
    assert [bool(h) if v else None for h, v in zip(hit, ok)] == want_m.to_pylist()
    o = out_off.cpu().numpy()
    data = out.cpu().numpy().tobytes()
    got = [data[o[i]:o[i + 1]].decode() if ok[i] else None for i in range(n)]
    assert all(o[i] == o[i + 1] for i in range(n) if not ok[i])
    assert got == want_r.to_pylist() and total == len("".join(x for x in got if x is not None).encode())


@pytest.mark.gpu
@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_gpu_level1_device_layouts(gpu, random_cases, n):
    """The device entry points under the layouts Level 2 never hands them (it uploads int64
    offsets from 0): int32 and int64 offsets, a first offset that is not 0 inside a larger
    values buffer, validity at bit offsets 3 and 69; row counts around a wave and a block.
    contains, replace-measure and replace-fill equal Level 2 on the same rows; the output
    validity words are rebased to bit 0 with zero bits past n."""
    torch = gpu
    c = _pick(random_cases, 32)
    rows = (list(c["rows"]) * (n // len(c["rows"]) + 1))[:n]
    for r in range(3, n, 9):
        rows[r] = None
    arr = pa.array(rows, type=pa.large_string())
    prog = FuzzyProgram.native(c["target"], c["wildcard"], c["include_original"], c["max_length"])
    prog.set_replacement("<<>>")
    want_m = prog.contains(arr).to_pylist()
    want_r = prog.replace(arr, True)
    want_off = np.frombuffer(want_r.buffers()[1], dtype=np.int64, count=n + 1)
    want_val = want_r.buffers()[2].to_pybytes()[:int(want_off[n])]
    assert any(want_m) and not all(x for x in want_m if x is not None)

    dev = torch.device("cuda:0")
    words = (n + 63) // 64
    canary = 0x5A5A5A5A5A5A5A5A
    stream = torch.cuda.Stream(device=dev)
    s = ctypes.c_void_p(stream.cuda_stream)
    tb = ctypes.c_int64(0)
    _lib.call("rogtk_str_temp_bytes", n, ctypes.byref(tb))
    data = [b"zz" if r is None else r.encode() for r in rows]  # null rows own bytes, as Arrow allows
    for ow, pre, voff in itertools.product((4, 8), (b"", b"\x82\xacPREFIX"), (3, 69)):
        offs = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(d) for d in data], out=offs[1:])
        offs += len(pre)
        bits = np.ones(voff + n + 13, dtype=np.uint8)  # junk outside the column's window
        bits[:voff] = np.arange(voff) % 3 == 0
        bits[voff:voff + n] = [r is not None for r in rows]
        t_off = torch.from_numpy(offs.astype(np.int32 if ow == 4 else np.int64)).to(dev)
        t_val = torch.from_numpy(np.frombuffer(pre + b"".join(data) + b"\x80POST", dtype=np.uint8).copy()).to(dev)
        t_bits = torch.from_numpy(np.packbits(bits, bitorder="little")).to(dev)
        col = _lib.StrCol(t_off.data_ptr(), ow, t_val.data_ptr(), t_val.numel(), t_bits.data_ptr(), voff, n)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            hit = torch.full((words + 1,), canary, dtype=torch.int64, device=dev)
            vb = torch.full((words + 1,), canary, dtype=torch.int64, device=dev)
            rvb = torch.full((words + 1,), canary, dtype=torch.int64, device=dev)
            out_off = torch.full((n + 2,), canary, dtype=torch.int64, device=dev)
            temp = torch.zeros(tb.value, dtype=torch.uint8, device=dev)
            _lib.call("rogtk_fuzzy_contains", prog.handle, ctypes.byref(col), hit.data_ptr(), vb.data_ptr(), s)
            _lib.call("rogtk_fuzzy_replace_measure", prog.handle, ctypes.byref(col), 1, out_off.data_ptr(),
                      rvb.data_ptr(), temp.data_ptr(), tb.value, s)
            stream.synchronize()
            o = out_off.cpu().numpy()
            total = int(o[n])
            out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device=dev)
            _lib.call("rogtk_fuzzy_replace_fill", prog.handle, ctypes.byref(col), 1, out_off.data_ptr(),
                      out.data_ptr(), s)
            stream.synchronize()
        what = (ow, len(pre), voff)
        for t in (hit, vb, rvb):
            assert int(t[words].item()) == canary, what
        assert o[n + 1] == canary, what

        def unpack(t):
            return np.unpackbits(t[:words].cpu().numpy().view(np.uint8), bitorder="little")

        valid = [r is not None for r in rows]
        for t in (vb, rvb):  # rebased to bit 0, zero past n
            assert unpack(t)[:n].astype(bool).tolist() == valid and not unpack(t)[n:].any(), what
        h = unpack(hit)
        assert [bool(x) if v else None for x, v in zip(h[:n], valid)] == want_m, what
        assert np.array_equal(o[:n + 1], want_off), what
        data_out = out.cpu().numpy()
        assert data_out[:total].tobytes() == want_val and (data_out[total:] == 0xA5).all(), what
