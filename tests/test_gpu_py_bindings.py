"""The form of an input does not change a host wrapper's answer: every column
form of tests/py_binding_cases.py, and the per-row integer arguments as numpy, Arrow and chunked
Arrow, against the same rows passed as a plain Python list. The answers for a list are checked
against the restatements by the wrappers' own test files; nothing here says what they are."""
from __future__ import annotations

import numpy as np
import pyarrow as pa
import pytest

import py_binding_cases as C

pytestmark = pytest.mark.gpu

UMIS, CIGARS = C.umi_rows(), C.cigar_rows()
WHITELIST = sorted({u for u in UMIS if u is not None and len(u) == 12 and set(u) <= set("ACGT")})[:6]


@pytest.fixture(scope="module")
def rg():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import rogtk_amd

    return rogtk_amd


@pytest.fixture(scope="module")
def wl(rg):
    return rg.BarcodeWhitelist(WHITELIST)


def _plain(x):
    """An answer as plain Python values; repr() so that NaN equals NaN."""
    if isinstance(x, (pa.Array, pa.ChunkedArray)):
        return repr(x.to_pylist())
    if isinstance(x, np.ndarray):
        return repr(x.tolist())
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return [_plain(v) for v in x]
    return repr(x)


def _call(rg, fn):
    """fn()'s answer, or the library's refusal: a form must not change that either."""
    try:
        return _plain(fn())
    except rg.RogtkError as e:
        return ("RogtkError", e.code)


def _correction(r):
    return [r.corrected, r.cluster_id, r.n_clusters, r.clusters, r.umi_len]


def _umi_answers(rg, wl, col, n):
    groups = (np.arange(n) % 3).astype(np.uint32)
    score = (np.arange(n) * 7 % 5).astype(np.uint32)
    ids = rg.umi_cluster(col, 12, 1)
    calls = {
        "complexity": lambda: rg.umi_complexity_scores(col),
        "hamming_within": lambda: rg.hamming_within(col, "ACGTACGTACGT", 2),
        "hamming_distance": lambda: rg.hamming_distance(col, "ACGTACGTACGT"),
        "cluster": lambda: ids,
        "cluster_directional": lambda: rg.umi_cluster(col, 12, 1, method="directional"),
        "cluster_groups": lambda: rg.umi_cluster(col, 12, 1, method="directional", groups=groups),
        "correct": lambda: _correction(rg.umi_correct(col, 12, 1)),
        "correct_directional": lambda: _correction(rg.umi_correct(col, 12, 1, method="directional")),
        "correct_groups": lambda: _correction(rg.umi_correct(col, 12, 1, method="directional", groups=groups)),
        "summary": lambda: rg.umi_cluster_summary(col, ids[0], ids[1], 12),
        "dedup": lambda: _dedup(rg.umi_dedup(col, 12, score=score, method="directional")),
        "barcode_correct": lambda: _barcode(wl.correct(col)),
        "barcode_count": lambda: wl.count(col),
        "reverse_complement": lambda: rg.reverse_complement(col),
        "fuzzy_contains": lambda: rg.col(col).fuzzy.contains("ACGT"),
        "fuzzy_replace_target": lambda: rg.col(col).fuzzy.replace_target("ACGTA", "<R>"),
        "kmer_spectrum": lambda: rg.kmer_spectrum(col, 5, 1),
    }
    return {name: _call(rg, fn) for name, fn in calls.items()}


def _dedup(r):
    return [r.keep, r.rows, r.best, r.n_kept, r.cluster_id, r.n_clusters, r.umi_len]


def _barcode(r):
    return [r.index, r.status, r.corrected, r.exact_counts, r.counts, r.totals]


@pytest.mark.parametrize("kind", list(C.TYPES))
def test_column_form_does_not_change_the_answer(rg, wl, kind):
    from_list = {}
    for name, col, rows in C.forms(UMIS, kind):
        key = tuple(rows)
        if key not in from_list:
            from_list[key] = _umi_answers(rg, wl, rows, len(rows))
            assert len(rows) < C.N_ROWS or "RogtkError" not in repr(from_list[key])
        got = _umi_answers(rg, wl, col, len(rows))
        for fn, want in from_list[key].items():
            assert got[fn] == want, (kind, name, fn)
    for name, col, rows in C.forms(CIGARS, kind):
        for block_dels in (False, True):
            want = _call(rg, lambda: rg.parse_cigar(rows, block_dels))
            assert _call(rg, lambda: rg.parse_cigar(col, block_dels)) == want, (kind, name, block_dels)


def test_key_array_form_does_not_change_the_answer(rg, wl):
    n = len(UMIS)
    keys = (np.arange(n) * 5 % 4).astype(np.uint32)
    prior = np.arange(len(WHITELIST), dtype=np.uint32) * 3

    def answers(groups, score, counts):
        return {
            "cluster": _call(rg, lambda: rg.umi_cluster(UMIS, 12, 1, method="directional", groups=groups)),
            "correct": _call(rg, lambda: _correction(rg.umi_correct(UMIS, 12, 0, groups=groups))),
            "dedup": _call(rg, lambda: _dedup(rg.umi_dedup(UMIS, 12, score=score, groups=groups,
                                                          method="directional"))),
            "best_rows": _call(rg, lambda: _dedup(rg.cluster_best_rows(groups, score))),
            "barcode": _call(rg, lambda: _barcode(wl.correct(UMIS, counts=counts))),
        }

    want = answers(keys, keys, prior)
    assert "RogtkError" not in repr(want)
    as_forms = [
        lambda a: a.astype(np.int64),
        lambda a: pa.array(a.astype(np.uint8)),
        lambda a: pa.chunked_array([pa.array(a[:3], type=pa.uint32()), pa.array(a[3:], type=pa.uint32())]),
    ]
    for form in as_forms:
        assert answers(form(keys), form(keys), form(prior)) == want
