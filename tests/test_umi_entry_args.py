"""The argument rules of the UMI cluster / correct C entries (include/rogtk_hip.h), in one table:
the twelve rogtk_umi_{cluster,correct}[_directional|_grouped]_{host,dev} entries and the two
rogtk_cluster_summary_{host,dev} entries, called through _lib.hip() with one bad argument each.

Every refusal comes before the library looks for a device or at a buffer, so the table runs on
a machine without a GPU; the "device" pointers of the *_dev entries are host arrays that no
accepted call ever sees. The expected codes are the library's answers as they stand, also
where sibling entries disagree:

* rogtk_umi_cluster_host and rogtk_umi_cluster_dev (and the directional host entry at
  max_distance 0, which is the same call) have no row limit, so n = 2^31 is not a case for
  them; with NULL buffers rogtk_umi_cluster_dev answers INVALID where its siblings, which
  check the row count first, answer UNSUPPORTED.
* n < 0 is INVALID on the host entries and on rogtk_umi_cluster_dev, UNSUPPORTED (the row
  limit) on the other device entries.
* The host entries want an offsets array even for n = 0.
* The host correct / summary entries reach the device for an empty column too (they allocate
  the empty results there), the cluster entries return before it.
* rogtk_cluster_summary_dev wants its outputs even for n = 0.

Which of two bad arguments answers is one order for all twelve entries (row limit, method,
max_distance, NULL buffer, umi_len; on the host entries the column's own checks first) and is
pinned only where a case below names two.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from rogtk_amd import _lib

OK, E, U, NODEV = _lib.ROGTK_OK, _lib.ROGTK_E_INVALID, _lib.ROGTK_E_UNSUPPORTED, _lib.ROGTK_E_NODEVICE
BIG = 1 << 31
EMPTY = "empty"  # the expected answer for an empty column on an entry that reaches the device

N = 3
_OFF = np.arange(N + 1, dtype=np.int64) * 4
_VAL = np.frombuffer(b"ACGTACGAACGT", dtype=np.uint8).copy()
_U32 = np.zeros(8, dtype=np.uint32)
_U64 = np.zeros(8, dtype=np.uint64)
_I64 = np.zeros(8, dtype=np.int64)
_OUT = np.zeros(16, dtype=np.uint8)
_IDS_PAST_END = np.array([0, 5, 0], dtype=np.uint32)  # with n_clusters 1


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


HOST_COL = ("offsets", "ow", "values", "values_len", "validity", "voff", "n")
DEV_COL = ("offsets", "values", "validity", "n")
CORRECT_OUT = ("corrected", "representatives", "n_reads", "n_distinct")
SPEC = {
    "rogtk_umi_cluster_host": HOST_COL + ("umi_len", "max_distance", "cluster_id", "n_clusters", "resolved"),
    "rogtk_umi_cluster_directional_host": HOST_COL + ("umi_len", "max_distance", "cluster_id", "n_clusters", "resolved"),
    "rogtk_umi_cluster_grouped_host": HOST_COL + ("groups", "umi_len", "method", "max_distance", "cluster_id",
                                                  "n_clusters", "resolved", "cluster_group"),
    "rogtk_umi_cluster_dev": DEV_COL + ("umi_len", "max_distance", "cluster_id", "n_clusters", "stream"),
    "rogtk_umi_cluster_directional_dev": DEV_COL + ("umi_len", "cluster_id", "n_clusters", "root_code", "stream"),
    "rogtk_umi_cluster_grouped_dev": DEV_COL + ("groups", "umi_len", "method", "max_distance", "cluster_id",
                                                "n_clusters", "root_code", "cluster_group_dev", "stream"),
    "rogtk_umi_correct_host": ("col", "umi_len", "max_distance", "cluster_id") + CORRECT_OUT + ("n_clusters", "resolved"),
    "rogtk_umi_correct_directional_host": ("col", "umi_len", "max_distance", "cluster_id") + CORRECT_OUT
                                          + ("n_clusters", "resolved"),
    "rogtk_umi_correct_grouped_host": ("col", "groups", "umi_len", "method", "max_distance", "cluster_id") + CORRECT_OUT
                                      + ("cluster_group", "n_clusters", "resolved"),
    "rogtk_umi_correct_dev": DEV_COL + ("umi_len", "max_distance", "cluster_id", "n_clusters", "corrected_values",
                                        "stream"),
    "rogtk_umi_correct_directional_dev": DEV_COL + ("umi_len", "cluster_id", "n_clusters", "corrected_values", "stream"),
    "rogtk_umi_correct_grouped_dev": DEV_COL + ("groups", "umi_len", "method", "max_distance", "cluster_id",
                                                "n_clusters", "corrected_values", "cluster_group_dev", "stream"),
    "rogtk_cluster_summary_host": ("col", "umi_len", "cluster_id", "n_clusters_in", "representatives", "n_reads",
                                   "n_distinct"),
    "rogtk_cluster_summary_dev": DEV_COL + ("umi_len", "cluster_id", "n_clusters_in", "n_reads_dev", "n_distinct_dev",
                                            "rep_rows", "rep_offsets", "rep_values_len", "stream"),
}
ENTRIES = tuple(SPEC)
HOST = tuple(e for e in ENTRIES if e.endswith("_host"))
DEV = tuple(e for e in ENTRIES if e.endswith("_dev"))
COL_HOST = tuple(e for e in HOST if "col" in SPEC[e])       # the column as a rogtk_str_col
IDS = tuple(e for e in ENTRIES if "summary" not in e)        # the twelve
GROUPED = tuple(e for e in ENTRIES if "grouped" in e)
HAS_MAXD = tuple(e for e in ENTRIES if "max_distance" in SPEC[e])
ROW_LIMIT = tuple(e for e in ENTRIES if e not in ("rogtk_umi_cluster_host", "rogtk_umi_cluster_dev"))


def _call(entry, **bad):
    """One call of `entry` with good arguments but for `bad`. Returns (status, *n_clusters, message)."""
    nk = ctypes.c_int64(77)
    results = {"corrected": _lib.StrResult(), "representatives": _lib.StrResult(), "n_reads": _lib.U32Result(),
               "n_distinct": _lib.U32Result(), "cluster_group": _lib.U32Result()}
    good = {"offsets": _p(_OFF), "ow": 8, "values": _p(_VAL), "values_len": _VAL.size, "validity": None, "voff": 0,
            "n": N, "umi_len": 4, "method": 1, "max_distance": 1, "groups": _p(_U32), "cluster_id": _p(_U32),
            "n_clusters": ctypes.byref(nk), "resolved": None, "stream": None, "root_code": _p(_U64),
            "cluster_group_dev": _p(_U32), "corrected_values": _p(_OUT), "n_clusters_in": 1, "n_reads_dev": _p(_U32),
            "n_distinct_dev": _p(_U32), "rep_rows": _p(_I64), "rep_offsets": _p(_I64),
            "rep_values_len": ctypes.byref(ctypes.c_int64(0))}
    good.update({k: ctypes.byref(r) for k, r in results.items()})
    unknown = set(bad) - set(good) - {"col"}
    assert not unknown, unknown
    a = {**good, **bad}
    desc = _lib.StrCol(a["offsets"], a["ow"], a["values"], a["values_len"], a["validity"], a["voff"], a["n"])
    a["col"] = bad.get("col", ctypes.byref(desc))
    lib = _lib.hip()
    rc = getattr(lib, entry)(*[a[name] for name in SPEC[entry]])
    msg = lib.rogtk_last_error().decode() if rc else ""
    for k in ("corrected", "representatives"):
        lib.rogtk_str_result_free(ctypes.byref(results[k]))
    for k in ("n_reads", "n_distinct", "cluster_group"):
        lib.rogtk_u32_result_free(ctypes.byref(results[k]))
    return rc, nk.value, msg


def _cases():
    c = []  # (entry, bad arguments, expected code, substring of the message or None)
    for e in ROW_LIMIT:  # values stays non-NULL: the host check of a NULL values reads offsets[n]
        c.append((e, dict(n=BIG), U, None))
    c.append(("rogtk_umi_cluster_dev", dict(n=BIG, offsets=None, values=None, cluster_id=None), E, None))
    c.append(("rogtk_umi_correct_dev", dict(n=BIG, offsets=None, values=None, cluster_id=None, corrected_values=None),
              U, None))
    for e in ENTRIES:
        c.append((e, dict(n=-1), U if e in DEV and e != "rogtk_umi_cluster_dev" else E, None))
    # n > 0 with a NULL buffer
    for e in ENTRIES:
        names = ["offsets", "values", "cluster_id"]
        names += ["groups"] if e in GROUPED else []
        names += ["corrected_values"] if "corrected_values" in SPEC[e] else []
        for name in names:
            c.append((e, {name: None}, E, None))
    for e in HOST:
        c.append((e, dict(ow=2), E, "offset_width"))
    for e in COL_HOST:
        c.append((e, dict(col=None), E, None))
        for name in CORRECT_OUT:
            if name in SPEC[e]:
                c.append((e, {name: None}, E, None))
    for name in ("n_reads_dev", "n_distinct_dev", "rep_rows", "rep_offsets", "rep_values_len"):
        c.append(("rogtk_cluster_summary_dev", {name: None}, E, None))
    for e in DEV:
        c.append((e, dict(umi_len=0), E, "umi_len"))
        c.append((e, dict(umi_len=0, n=0), E, "umi_len"))
    for e in HAS_MAXD:
        c.append((e, dict(max_distance=2), U, "max_distance 2: only 0 and 1 are supported"))
        c.append((e, dict(max_distance=-1), U, "max_distance -1: only 0 and 1 are supported"))
    for e in GROUPED:
        c.append((e, dict(method=2), E, "method 2"))
        c.append((e, dict(method=-1), E, None))
        c.append((e, dict(method=2, max_distance=2), E, None))
        c.append((e, dict(method=0, max_distance=1), U, 'method="directional"'))
        c.append((e, dict(method=0, max_distance=2), U, "max_distance 2: only 0 and 1 are supported"))
    for e in ("rogtk_cluster_summary_host", "rogtk_cluster_summary_dev"):
        c.append((e, dict(n_clusters_in=-1), E, "n_clusters"))
        c.append((e, dict(n_clusters_in=(1 << 32) - 1), E, "n_clusters"))
    c.append(("rogtk_cluster_summary_host", dict(cluster_id=_p(_IDS_PAST_END)), E, "cluster_id[1]"))
    # n = 0 with every buffer NULL
    nulls = dict(n=0, values=None, validity=None, cluster_id=None, groups=None, corrected_values=None, root_code=None,
                 cluster_group_dev=None, values_len=0)
    for e in IDS:
        if e in DEV:
            c.append((e, dict(nulls, offsets=None), OK, None))
        else:
            c.append((e, dict(nulls, offsets=None), E, "offsets"))
            want = EMPTY if e in COL_HOST else OK
            c.append((e, dict(nulls), want, None))
            c.append((e, dict(nulls, max_distance=0), want, None))
            if e in GROUPED:
                c.append((e, dict(nulls, method=0, max_distance=0), want, None))
    c.append(("rogtk_cluster_summary_host", dict(nulls, n_clusters_in=0), EMPTY, None))
    c.append(("rogtk_cluster_summary_dev", dict(nulls, offsets=None, n_clusters_in=0, n_reads_dev=None,
                                                n_distinct_dev=None, rep_rows=None, rep_offsets=None), E, None))
    return c


CASES = _cases()


def _id(case):
    entry, bad, _, _ = case
    return entry[len("rogtk_"):] + "-" + ",".join(f"{k}={'NULL' if v is None else v if isinstance(v, int) else 'set'}"
                                                  for k, v in bad.items())


def test_the_table_covers_every_entry():
    assert len(IDS) == 12 and len(ENTRIES) == 14 and {e for e, *_ in CASES} == set(ENTRIES)
    lib = _lib.hip()
    for e in ENTRIES:
        assert len(_lib.SIGNATURES[e]) == len(SPEC[e]) and hasattr(lib, e), e


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_bad_call(case):
    entry, bad, want, text = case
    if want == EMPTY:
        want = OK if _lib.device_count() else NODEV
    rc, nk, msg = _call(entry, **bad)
    assert rc == want, (rc, msg)
    if text:
        assert text in msg, msg
    if rc == OK and "n_clusters" in SPEC[entry]:
        assert nk == 0
