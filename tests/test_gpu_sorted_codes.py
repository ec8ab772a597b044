"""The front end and the back end that the sort engines share (rogtk_amd/csrc/sorted_codes.hip,
cc_labels in dist_cluster.hip): every column goes through rogtk_umi_cluster_dev
(max_distance 0 and 1; umi_len 17..32 is the long engine) and through
rogtk_umi_cluster_directional_dev, and the ids and cluster counts equal the oracles the suite
already uses: oracle.pyoracle for the transitive method, tests/directional_spec.py for directional.

Shapes sit where the pack kernel can break: row counts around its 1024-row tile and the 64-lane
wave, umi_len 16 / 17 (u32 / u64 sort keys) and 32 (the top code bits in use), and the degenerate
columns (all null, all irregular, one code, every row distinct). The device entries take a
validity bitmap at bit offset 0 only, so the bitmap with a non-zero bit offset goes through the
host entries, which also cover 4-byte offsets."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

from directional_spec import restate

pytestmark = pytest.mark.gpu

NULL_ID = 0xFFFFFFFF


@pytest.fixture(scope="module")
def lib():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import rogtk_amd
    from rogtk_amd import _lib

    assert rogtk_amd.device_count() >= 1
    return _lib


def _random(rng, n, L):
    return [bytes(r) for r in np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=(n, L))]]


@functools.lru_cache(maxsize=None)
def _column(kind: str, n: int, L: int):
    """Rows of one test column (None = null)."""
    rng = np.random.default_rng(1000 * L + n)
    if kind == "null":
        return (None,) * n
    if kind == "irregular":  # wrong lengths and an N, with repeats
        pool = [b"ACGT" * (L // 4) + b"N" * (L % 4 or 4), b"A" * (L - 1), b"A" * (L + 1), b"", b"C" * (L - 1) + b"N",
                b"N" + b"C" * (L - 1)]
        return tuple(pool[int(k)] for k in rng.integers(0, len(pool), size=n))
    if kind == "same":
        return (b"T" * L,) * n
    if kind == "distinct":
        rows = set()
        while len(rows) < n:
            rows.update(_random(rng, n - len(rows), L))
        return tuple(sorted(rows, key=lambda r: rng.random()))
    assert kind == "mixed"
    # families of one-substitution neighbours with skewed counts, a few irregular and null rows;
    # the all-T code (every key bit set) and the all-A code are present
    parents = _random(rng, max(n // 12, 1), L) + [b"T" * L, b"A" * L]
    rows = []
    for _ in range(n):
        u = bytearray(parents[int(rng.integers(len(parents)))])
        if rng.random() < 0.35:
            j = int(rng.integers(L))
            u[j] = b"ACGT"[int(rng.integers(4))]
        r = rng.random()
        if r < 0.02:
            rows.append(None)
        elif r < 0.04:
            u[int(rng.integers(L))] = ord("N")
            rows.append(bytes(u))
        elif r < 0.05:
            rows.append(bytes(u[:-1]))
        else:
            rows.append(bytes(u))
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def _expected(kind: str, n: int, L: int):
    """{method: (ids as u32 with NULL_ID for nulls, n_clusters)}, computed once per column."""
    from oracle import pyoracle as P

    items = list(_column(kind, n, L))
    out = {}
    for md in (0, 1):
        cid, valid, k, _ = P.umi_cluster(P.StrCol.from_list(items), L, md)
        out[md] = (np.where(valid.astype(bool), cid, NULL_ID).astype(np.uint32), k)
    ids, k, _, _ = restate(items, L)
    out["directional"] = (np.array([NULL_ID if i is None else i for i in ids], dtype=np.uint32), k)
    return out


def _buffers(items, offset_dtype, voff=0):
    dense = [b"" if u is None else u for u in items]
    off = np.concatenate([[0], np.cumsum([len(u) for u in dense])]).astype(offset_dtype)
    val = np.frombuffer(b"".join(dense) + b"\0", np.uint8).copy()
    bits = np.array([True] * voff + [u is not None for u in items] + [False] * 7)
    return off, val, np.packbits(bits, bitorder="little")


def _run_dev(lib, items, L):
    """{method: (ids, n_clusters)} of the three device entries on one device column."""
    import torch

    n = len(items)
    off, val, vbits = (torch.from_numpy(a).cuda() for a in _buffers(items, np.int64))
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    out = {}
    for method in (0, 1, "directional"):
        cid = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        k = ctypes.c_int64(-1)
        if method == "directional":
            lib.call("rogtk_umi_cluster_directional_dev", p(off), p(val), p(vbits), n, L, p(cid), ctypes.byref(k),
                     None, s)
        else:
            lib.call("rogtk_umi_cluster_dev", p(off), p(val), p(vbits), n, L, method, p(cid), ctypes.byref(k), s)
        torch.cuda.synchronize()
        out[method] = (cid.cpu().numpy().view(np.uint32), k.value)
    return out


def _run_host(lib, items, L, offset_dtype, voff):
    """The same through the host entries: offsets of the given width, validity at bit `voff`."""
    n = len(items)
    off, val, vbits = _buffers(items, offset_dtype, voff)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = {}
    for method in (0, 1, "directional"):
        cid = np.full(n, 0x5A5A5A5A, dtype=np.uint32)
        k, rl = ctypes.c_int64(-1), ctypes.c_int(-1)
        entry = "rogtk_umi_cluster_directional_host" if method == "directional" else "rogtk_umi_cluster_host"
        lib.call(entry, vp(off), off.itemsize, vp(val), int(off[-1]), vp(vbits), voff, n, L,
                 1 if method == "directional" else method, vp(cid), ctypes.byref(k), ctypes.byref(rl))
        assert rl.value == L
        out[method] = (cid, k.value)
    return out


def _assert_equal(got, want):
    for method, (ids, k) in want.items():
        gi, gk = got[method]
        assert gk == k, f"{method}: n_clusters {gk} != {k}"
        bad = np.nonzero(gi != ids)[0]
        assert bad.size == 0, f"{method}: {bad.size} ids differ, first rows {bad[:5]}"


@pytest.mark.parametrize("L", [16, 17])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
def test_tile_and_wave_boundaries(lib, n, L):
    _assert_equal(_run_dev(lib, _column("mixed", n, L), L), _expected("mixed", n, L))


def test_top_code_bits_survive(lib):
    """umi_len 32: all 64 key bits are code. Rows that differ only in their first base (the top
    two bits) must stay apart at max_distance 0 and sort after the all-A code."""
    items = _column("mixed", 1025, 32)
    want = _expected("mixed", 1025, 32)
    _assert_equal(_run_dev(lib, items, 32), want)
    first = {u[0] for u in items if u is not None and len(u) == 32}
    assert first == set(b"ACGT") and b"T" * 32 in items and b"A" * 32 in items
    ids0 = want[0][0]
    assert ids0[items.index(b"A" * 32)] == 0
    assert ids0[items.index(b"T" * 32)] == len({u for u in items if u is not None and len(u) == 32
                                                and set(u) <= set(b"ACGT")}) - 1


@pytest.mark.parametrize("L", [16, 17])
@pytest.mark.parametrize("kind", ["null", "irregular", "same", "distinct"])
def test_degenerate_columns(lib, kind, L):
    n = 1025
    want = _expected(kind, n, L)
    _assert_equal(_run_dev(lib, _column(kind, n, L), L), want)
    k = {"null": 0, "same": 1, "distinct": n}.get(kind)
    if k is not None:
        assert want[0][1] == k


@pytest.mark.parametrize("L", [16, 17])
def test_validity_bit_offset_and_narrow_offsets(lib, L):
    """The 1025-row mixed column through the host entries: 4-byte and 8-byte offsets, the
    validity bitmap starting at bit 3."""
    items = _column("mixed", 1025, L)
    assert any(u is None for u in items)
    want = _expected("mixed", 1025, L)
    _assert_equal(_run_host(lib, items, L, np.int32, 0), want)
    _assert_equal(_run_host(lib, items, L, np.int32, 3), want)
    _assert_equal(_run_host(lib, items, L, np.int64, 3), want)


@pytest.mark.parametrize("nv,edges", [
    (5, []),                                                    # no edges
    (5, [(0, 1), (1, 2), (2, 3), (3, 4)]),                       # a path of 5
    (6, [(4, 0), (0, 2), (2, 4), (5, 1), (3, 5)]),              # two components; (2, 4) is a back edge
], ids=["no-edges", "path", "two-components"])
def test_cc_labels_small_graphs(lib, nv, edges):
    import torch

    from test_dist_sharded import NumpyOps

    E = torch.tensor(edges, dtype=torch.int32).reshape(len(edges), 2)
    want, want_k = NumpyOps().cc_labels(nv, E)
    Ed = E.cuda()
    labels = torch.full((nv,), -1, dtype=torch.int32, device="cuda")
    k = ctypes.c_int64(-1)
    lib.call("rogtk_cc_labels", nv, ctypes.c_void_p(Ed.data_ptr()) if len(edges) else None, len(edges),
             ctypes.c_void_p(labels.data_ptr()), ctypes.byref(k),
             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert k.value == want_k
    assert labels.cpu().tolist() == want.tolist()
