"""The twelve UMI cluster / correct C entries on the GPU as one matrix: for every rule the same
column goes through the host cluster entry, the device cluster entry, the host correct entry
and the device correct entry, and the four answers (ids, n_clusters, cluster keys, corrected
bytes, and the host entry's summary table) equal the pure-Python restatements:
oracle.pyoracle.umi_cluster for method="cluster", directional_spec.restate, grouped_spec.restate
and correct_spec.summarize. No expected value comes from the library.

The columns are the smallest at which the plumbing between the entries and the engines can go
wrong: no rows, one row, only nulls, the known answer with irregular and null rows, 65 regular
rows (no irregular row, one row past a 64-row word of regular bits), and 20-base rows (the long
engine). Every host column goes in with 32-bit offsets, with 64-bit offsets and with its
validity bitmap starting at bit 3."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import directional_spec as D
import grouped_spec as G
from correct_spec import is_regular, summarize

pytestmark = pytest.mark.gpu

NULL_ID = 0xFFFFFFFF


def _long_rows():
    rng = np.random.default_rng(11)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    parents = [bytes(acgt[rng.integers(0, 4, 20)]) for _ in range(8)]
    rows = []
    for i in range(40):
        r = bytearray(parents[i % 8])
        if i % 3 == 0:
            q = int(rng.integers(0, 20))
            r[q] = int(rng.choice([b for b in b"ACGT" if b != r[q]]))
        rows.append(bytes(r))
    return rows + [b"N" * 20, b"ACG", None]


# name -> (rows, umi_len)
COLUMNS = {
    "empty": ([], 4),
    "one": ([b"ACGT"], 4),
    "nulls": ([None] * 5, 4),
    "known": (D.KNOWN_ROWS, 4),
    "regular65": (D.random_families()[:65], 8),
    "long": (_long_rows(), 20),
}
# name -> (kind, method of the grouped entries, max_distance)
RULES = {
    "cluster_d0": ("cluster", 0, 0),
    "cluster_d1": ("cluster", 0, 1),
    "directional_d1": ("directional", 1, 1),
    "grouped_cluster_d0": ("grouped", 0, 0),
    "grouped_directional_d0": ("grouped", 1, 0),
    "grouped_directional_d1": ("grouped", 1, 1),
}
ENTRY = {"cluster": "rogtk_umi_%s_%s", "directional": "rogtk_umi_%s_directional_%s", "grouped": "rogtk_umi_%s_grouped_%s"}
MATRIX = [(c, r) for c in COLUMNS for r in RULES if c != "long" or RULES[r][0] == "cluster"]
LAYOUTS = ("offsets32", "offsets64", "validity_offset3")


def _keys(column):
    rows, _ = COLUMNS[column]
    if column == "known":
        return list(G.KNOWN_KEYS)
    return [(7, 0, 0xFFFFFFFF)[i % 3] for i in range(len(rows))]


@pytest.fixture(scope="module")
def lib():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from rogtk_amd import _lib

    assert _lib.device_count() >= 1
    return _lib


@pytest.fixture(scope="module")
def expected():
    """(column, rule) -> (ids with None for nulls, n_clusters, [(representative, n_reads,
    n_distinct)], corrected, cluster keys or None), computed once."""
    from oracle import pyoracle as P

    out = {}
    for column, rule in MATRIX:
        rows, L = COLUMNS[column]
        kind, _, d = RULES[rule]
        keys = None
        if kind == "grouped":
            ids, k, table4, corrected = G.restate(rows, _keys(column), L, d)
            table, keys = [t[:3] for t in table4], [t[3] for t in table4]
        elif kind == "directional":
            ids, k, table, corrected = D.restate(rows, L)
        else:
            ids, k = [], 0
            if rows:
                cid, valid, k, _ = P.umi_cluster(P.StrCol.from_list(rows), L, d)
                ids = [int(c) if v else None for c, v in zip(cid, valid)]
            table, corrected = summarize(rows, ids, k, L)
        out[column, rule] = (ids, k, table, corrected, keys)
    return out


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


class HostColumn:
    """The rows as Arrow buffers (a null row has no bytes) in one of LAYOUTS."""

    def __init__(self, rows, layout):
        dense = [b"" if x is None else x for x in rows]
        self.n = len(rows)
        self.offsets = np.concatenate([[0], np.cumsum([len(x) for x in dense])]).astype(
            np.int32 if layout == "offsets32" else np.int64)
        self.values = np.frombuffer(b"".join(dense) or b"\0", np.uint8).copy()
        valid = [x is not None for x in rows]
        self.voff, self.validity = 0, None
        if layout == "validity_offset3":  # three bits of another column's rows first
            self.voff = 3
            self.validity = np.packbits(np.array([False, True, False] + valid), bitorder="little")
        elif not all(valid):
            self.validity = np.packbits(np.array(valid), bitorder="little")

    def loose(self):
        return (_p(self.offsets), self.offsets.dtype.itemsize, _p(self.values), int(self.offsets[-1]),
                None if self.validity is None else _p(self.validity), self.voff, self.n)

    def desc(self, _lib):
        return _lib.StrCol(*self.loose())


def _u32_result(r):
    n = int(r.n)
    if n == 0:
        return []
    return np.ctypeslib.as_array(ctypes.cast(r.data, ctypes.POINTER(ctypes.c_uint32)), (max(n, 1),))[:n].tolist()


def _str_result(res):
    """A rogtk_str_result as a list of bytes / None."""
    n = int(res.n)
    offs = np.ctypeslib.as_array(ctypes.cast(res.offsets, ctypes.POINTER(ctypes.c_int64)), (n + 1,))
    data = ctypes.string_at(res.values, int(res.values_len))
    bits = np.ctypeslib.as_array(ctypes.cast(res.validity, ctypes.POINTER(ctypes.c_uint8)), (max((n + 7) // 8, 1),))
    rows = [data[offs[i]:offs[i + 1]] if (bits[i >> 3] >> (i & 7)) & 1 else None for i in range(n)]
    assert int(res.null_count) == sum(x is None for x in rows)
    return rows


def _host_cluster(_lib, col, keys, L, rule):
    """(ids, n_clusters, cluster keys or None) of the host cluster entry."""
    kind, method, d = RULES[rule]
    cid = np.full(max(col.n, 1), 0xABABABAB, np.uint32)
    nk, rl = ctypes.c_int64(-1), ctypes.c_int(-1)
    name = ENTRY[kind] % ("cluster", "host")
    if kind == "grouped":
        cg = _lib.U32Result()
        _lib.call(name, *col.loose(), _p(keys) if col.n else None, L, method, d, _p(cid), ctypes.byref(nk),
                  ctypes.byref(rl), ctypes.byref(cg))
        group = _u32_result(cg)
        _lib.hip().rogtk_u32_result_free(ctypes.byref(cg))
    else:
        _lib.call(name, *col.loose(), L, d, _p(cid), ctypes.byref(nk), ctypes.byref(rl))
        group = None
    assert rl.value == L
    return cid[:col.n].tolist(), nk.value, group


def _host_correct(_lib, col, keys, L, rule):
    """(ids, n_clusters, cluster keys or None, table, corrected) of the host correct entry."""
    kind, method, d = RULES[rule]
    hip = _lib.hip()
    cid = np.full(max(col.n, 1), 0xABABABAB, np.uint32)
    nk, rl = ctypes.c_int64(-1), ctypes.c_int(-1)
    cor, rep = _lib.StrResult(), _lib.StrResult()
    nr, nd, cg = _lib.U32Result(), _lib.U32Result(), _lib.U32Result()
    outs = [ctypes.byref(cor), ctypes.byref(rep), ctypes.byref(nr), ctypes.byref(nd)]
    desc = col.desc(_lib)
    name = ENTRY[kind] % ("correct", "host")
    if kind == "grouped":
        _lib.call(name, ctypes.byref(desc), _p(keys) if col.n else None, L, method, d, _p(cid), *outs,
                  ctypes.byref(cg), ctypes.byref(nk), ctypes.byref(rl))
    else:
        _lib.call(name, ctypes.byref(desc), L, d, _p(cid), *outs, ctypes.byref(nk), ctypes.byref(rl))
    try:
        table = list(zip(_str_result(rep), _u32_result(nr), _u32_result(nd)))
        group = _u32_result(cg) if kind == "grouped" else None
        corrected = _str_result(cor)
    finally:
        hip.rogtk_str_result_free(ctypes.byref(cor))
        hip.rogtk_str_result_free(ctypes.byref(rep))
        for r in (nr, nd, cg):
            hip.rogtk_u32_result_free(ctypes.byref(r))
    assert rl.value == L
    return cid[:col.n].tolist(), nk.value, group, table, corrected


def _device(_lib, rows, keys, L, rule, what):
    """(ids, n_clusters, cluster keys or None, corrected or None) of a device entry."""
    import torch

    kind, method, d = RULES[rule]
    n = len(rows)
    col = HostColumn(rows, "offsets64")
    t = lambda a: torch.from_numpy(a).cuda()
    off, val = t(col.offsets), t(col.values)
    vbits = t(np.packbits(np.array([x is not None for x in rows] + [False] * 7), bitorder="little"))
    dkeys = t(keys.view(np.int32)) if n else None
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    cid = torch.full((max(n, 1),), -3, dtype=torch.int32, device="cuda")
    cgroup = torch.full((max(n, 1),), -2, dtype=torch.int32, device="cuda")
    out = torch.zeros(col.values.size, dtype=torch.uint8, device="cuda")
    nk = ctypes.c_int64(-1)
    tail = [p(out)] if what == "correct" else []
    args = [p(off) if n else None, p(val) if n else None, p(vbits) if n else None, n]
    ids_out = [p(cid) if n else None, ctypes.byref(nk)]
    name = ENTRY[kind] % (what, "dev")
    if kind == "grouped":
        root = [None] if what == "cluster" else []
        _lib.call(name, *args, p(dkeys), L, method, d, *ids_out, *root, *tail, p(cgroup) if n else None, s)
    elif kind == "directional":
        root = [None] if what == "cluster" else []
        _lib.call(name, *args, L, *ids_out, *root, *tail, s)
    else:
        _lib.call(name, *args, L, d, *ids_out, *tail, s)
    torch.cuda.synchronize()
    k = nk.value
    group = cgroup.cpu().numpy().view(np.uint32)[:k].tolist() if kind == "grouped" else None
    corrected = None
    if what == "correct":
        data = out.cpu().numpy().tobytes()
        corrected = [None if x is None else data[col.offsets[i]:col.offsets[i + 1]] for i, x in enumerate(rows)]
    return cid.cpu().numpy().view(np.uint32)[:n].tolist(), k, group, corrected


def _rounds(_lib):
    r = ctypes.c_int64(-1)
    _lib.call("rogtk_directional_last_rounds", ctypes.byref(r))
    return r.value


@pytest.mark.parametrize("column,rule", MATRIX, ids=[f"{c}-{r}" for c, r in MATRIX])
def test_four_entries_one_answer(lib, expected, column, rule):
    rows, L = COLUMNS[column]
    ids, k, table, corrected, group = expected[column, rule]
    want_ids = [NULL_ID if i is None else i for i in ids]
    keys = np.asarray(_keys(column), dtype=np.uint32)
    kind, _, d = RULES[rule]
    edges = kind != "cluster" and d == 1 and any(x is not None and is_regular(x, L) for x in rows)

    def rounds_ok():  # the relaxation ran under the directional rule, and only there
        if kind != "cluster":
            assert (_rounds(lib) >= 1) if edges else (_rounds(lib) == 0)

    for layout in LAYOUTS:
        col = HostColumn(rows, layout)
        assert _host_cluster(lib, col, keys, L, rule) == (want_ids, k, group), layout
        rounds_ok()
        assert _host_correct(lib, col, keys, L, rule) == (want_ids, k, group, table, corrected), layout
        rounds_ok()
    assert _device(lib, rows, keys, L, rule, "cluster") == (want_ids, k, group, None)
    rounds_ok()
    assert _device(lib, rows, keys, L, rule, "correct") == (want_ids, k, group, corrected)
    rounds_ok()


def test_cluster_method_leaves_last_rounds_alone(lib):
    """rogtk_directional_last_rounds is the last directional or grouped call's: the entries of
    method="cluster" (and the directional host entries at max_distance 0, which are that
    method) do not write it."""
    rows, L = COLUMNS["known"]
    keys = np.asarray(_keys("known"), dtype=np.uint32)
    _device(lib, rows, keys, L, "directional_d1", "cluster")
    r = _rounds(lib)
    assert r >= 1
    col = HostColumn(rows, "offsets64")
    for rule in ("cluster_d0", "cluster_d1"):
        _host_cluster(lib, col, keys, L, rule)
        assert _rounds(lib) == r
        _host_correct(lib, col, keys, L, rule)
        assert _rounds(lib) == r
        _device(lib, rows, keys, L, rule, "cluster")
        assert _rounds(lib) == r
        _device(lib, rows, keys, L, rule, "correct")
        assert _rounds(lib) == r
    nk, rl = ctypes.c_int64(-1), ctypes.c_int(-1)
    cid = np.zeros(col.n, np.uint32)
    lib.call("rogtk_umi_cluster_directional_host", *col.loose(), L, 0, _p(cid), ctypes.byref(nk), ctypes.byref(rl))
    assert _rounds(lib) == r
    _host_cluster(lib, col, keys, L, "grouped_directional_d0")
    assert _rounds(lib) == 0


def test_last_rounds_after_an_empty_column(lib):
    """The entries differ in what an empty column leaves in rogtk_directional_last_rounds, and
    the difference is kept: rogtk_umi_correct_directional_host leaves the last call's rounds,
    its directional and grouped siblings write 0."""
    rows, L = COLUMNS["known"]
    keys = np.asarray(_keys("known"), dtype=np.uint32)
    empty = HostColumn([], "offsets64")

    def relax():
        _device(lib, rows, keys, L, "directional_d1", "cluster")
        r = _rounds(lib)
        assert r >= 1
        return r

    r = relax()
    _host_correct(lib, empty, keys, L, "directional_d1")
    assert _rounds(lib) == r
    for call in (lambda rule: _host_cluster(lib, empty, keys, L, rule),
                 lambda rule: _device(lib, [], keys, L, rule, "cluster"),
                 lambda rule: _device(lib, [], keys, L, rule, "correct")):
        relax()
        call("directional_d1")
        assert _rounds(lib) == 0
    for call in (lambda: _host_cluster(lib, empty, keys, L, "grouped_directional_d1"),
                 lambda: _host_correct(lib, empty, keys, L, "grouped_directional_d1")):
        relax()
        call()
        assert _rounds(lib) == 0
