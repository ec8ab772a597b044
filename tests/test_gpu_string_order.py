"""The byte order of the string sort of irregular.hip: an LSD radix sort, one pass on the byte
length and one per zero-padded big-endian 8-byte chunk, exact through zero padding + the length
pass + a byte compare of neighbours. The same sort numbers the irregular clusters, ranks every
string for the correction's tie-break and feeds the max_distance 1 masked-record edges.

One hostile column (tests/backend_cases.py): NUL bytes inside and at the end of strings, strings
that differ only in their trailing NULs or only at byte 0, 6, 7, 8 or their last byte, bytes on
both sides of 0x80, lengths around every chunk edge up to 257 bytes, regular rows with every
one-byte variant, about 6 000 shuffled rows with repeats and nulls. Expected values come from
oracle.pyoracle.py_cluster_bruteforce, correct_spec (restate, summarize) and sorted() on bytes:
exact equality."""
from __future__ import annotations

import numpy as np
import pyarrow as pa
import pytest

import backend_cases as B
from correct_spec import as_bytes, is_regular, restate, summarize, table_of

pytestmark = pytest.mark.gpu

L = B.HOSTILE_LEN


@pytest.fixture(scope="module")
def rg():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import rogtk_amd

    assert rogtk_amd.device_count() >= 1
    return rogtk_amd


def _check_cluster(rg, col, rows, umi_len, md, want):
    ids, k = want[0], want[1]
    got, gk, _ = rg.umi_cluster(col, umi_len, md)
    assert gk == k
    assert got.to_pylist() == ids
    assert got.null_count == sum(x is None for x in rows)


def _check_correct(rg, col, rows, umi_len, md, want):
    ids, k, table, corrected = want
    res = rg.umi_correct(col, umi_len, md)
    assert res.n_clusters == k
    assert res.cluster_id.to_pylist() == ids
    assert table_of(res.clusters) == table
    assert as_bytes(res.corrected) == corrected
    assert res.corrected.null_count == sum(x is None for x in rows)


@pytest.mark.parametrize("md", [0, 1])
def test_cluster_ids(rg, md):
    rows = B.hostile_rows()
    want = B.hostile_restated(L, md)
    _check_cluster(rg, pa.array(rows, type=pa.large_binary()), rows, L, md, want)
    if md == 0:
        # regular clusters in code order, then the irregular strings by their rank in sorted()
        distinct = {x for x in rows if x is not None}
        regular = sorted(x for x in distinct if is_regular(x, L))
        irregular = sorted(x for x in distinct if not is_regular(x, L))
        rank = {s: j for j, s in enumerate(regular + irregular)}
        assert want[0] == [None if x is None else rank[x] for x in rows] and want[1] == len(rank)
        assert irregular[0] == b"" and irregular[1] == b"\0" and irregular[-1][0] == 0xFF
    else:
        assert want[1] < len(set(rows)) // 4  # the one-byte variants merge


@pytest.mark.parametrize("md", [0, 1])
def test_correction(rg, md):
    rows = B.hostile_rows()
    _check_correct(rg, pa.array(rows, type=pa.large_binary()), rows, L, md, B.hostile_restated(L, md))


def test_summary_with_caller_ids(rg):
    """Strings of different lengths and equal counts in one cluster: the representative is the
    byte-lexicographically smallest string (bytes compare unsigned, a proper prefix first), after
    a regular string if the cluster has one."""
    rows, ids, k = B.caller_id_rows()
    spec_ids = [None if x is None else i for x, i in zip(rows, ids)]
    table, _ = summarize(rows, spec_ids, k, L)
    assert [t[0] for t in table[:3]] == [b"A", b"ACGTACGT", b"\x7f"] and table[4][0] == b"" and table[-1] == (b"", 0, 0)
    assert table[3][0][64] == 0x10
    col = pa.array(rows, type=pa.large_binary())
    got = rg.umi_cluster_summary(col, np.array(ids, dtype=np.uint32), n_clusters=k, umi_len=L)
    assert table_of(got) == table
    # at umi_len 7 ACGTACG is the regular string of cluster 1
    table7, _ = summarize(rows, spec_ids, k, 7)
    assert table7[1][0] == b"ACGTACG"
    assert table_of(rg.umi_cluster_summary(col, np.array(ids, dtype=np.uint32), n_clusters=k, umi_len=7)) == table7


@pytest.mark.parametrize("form", ["binary", "large_binary", "slice", "chunks"])
def test_column_forms(rg, form):
    """4-byte and 8-byte offsets; a slice whose first row is row 3 (offsets that do not start at
    0 and a validity bitmap with a bit offset); three chunks."""
    rows = B.hostile_rows()
    first = 0
    if form == "binary":
        col = pa.array(rows, type=pa.binary())
    elif form == "large_binary":
        col = pa.array(rows, type=pa.large_binary())
    elif form == "slice":
        first = 3
        col = pa.array(rows, type=pa.binary()).slice(first)
        assert col.offset == 3 and col.null_count > 0 and col.buffers()[1] is not None
    else:
        cuts = [0, 1999, 2000, len(rows)]
        col = pa.chunked_array([pa.array(rows[a:b], type=pa.large_binary()) for a, b in zip(cuts[:-1], cuts[1:])])
        assert col.num_chunks == 3
    rows = rows[first:]
    want = B.hostile_restated(L, 1, first)
    _check_cluster(rg, col, rows, L, 1, want)
    _check_correct(rg, col, rows, L, 1, want)


@pytest.mark.parametrize("md", [0, 1])
def test_all_irregular_at_umi_len_40(rg, md):
    """No row is regular: every id and every rank comes from the string sort."""
    rows = B.hostile_rows()
    want = B.hostile_restated(40, md)
    col = pa.array(rows, type=pa.large_binary())
    _check_cluster(rg, col, rows, 40, md, want)
    _check_correct(rg, col, rows, 40, md, want)


@pytest.mark.parametrize("md", [0, 1])
def test_one_long_row_among_short_ones(rg, md):
    """One row of 257 bytes, the others at most 3: 33 chunk passes that move padding only."""
    rows = B.one_long_row()
    assert sorted(len(x) for x in rows if x is not None)[-2:] == [3, 257]
    want = restate(list(rows), 40, md)
    if md == 0:
        distinct = sorted({x for x in rows if x is not None})
        assert want[0] == [None if x is None else distinct.index(x) for x in rows]
        assert distinct.index(b"A" + b"\0" * 256) == distinct.index(b"A\0\0") + 1
    col = pa.array(rows, type=pa.large_binary())
    _check_cluster(rg, col, rows, 40, md, want)
    _check_correct(rg, col, rows, 40, md, want)
