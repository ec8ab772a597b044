"""cc_labels of dist_cluster.hip (hook-to-min + compress rounds, shared by the long, irregular
merge and sharded engines) called directly on graphs larger than one wave: labels and the count
equal the union-find reference of tests/test_dist_sharded.py (NumpyOps.cc_labels), components
numbered by their smallest vertex. Graphs come from tests/backend_cases.py."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

import backend_cases as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import rogtk_amd
    from rogtk_amd import _lib

    assert rogtk_amd.device_count() >= 1
    return _lib


def _run(lib, nv, E):
    """(labels, n_clusters) of rogtk_cc_labels; a call that does not converge raises."""
    import torch

    m = len(E)
    assert m == 0 or (E.min() >= 0 and E.max() < nv)  # the kernels trust the endpoints
    Ed = torch.from_numpy(np.array(E, dtype=np.int32)).cuda() if m else None
    labels = torch.full((max(nv, 1),), -1, dtype=torch.int32, device="cuda")
    k = ctypes.c_int64(-1)
    lib.call("rogtk_cc_labels", nv, ctypes.c_void_p(Ed.data_ptr()) if m else None, m,
             ctypes.c_void_p(labels.data_ptr()) if nv else None, ctypes.byref(k),
             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return labels.cpu().numpy()[:nv], k.value


@functools.lru_cache(maxsize=None)
def _union_find(name):
    """The reference's (labels, count) of a named graph, computed once."""
    import torch

    from test_dist_sharded import NumpyOps

    nv, E = {"path": B.cc_path, "star": B.cc_star, "small": B.cc_small_components}[name]()[:2]
    want, k = NumpyOps().cc_labels(nv, torch.from_numpy(np.array(E, dtype=np.int32)))
    return want.numpy(), k


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_path_of_100000_shuffled_vertices(lib, order):
    nv, E = B.cc_path()
    if order == "descending":
        E = E[::-1]
    elif order == "shuffled":
        E = E[np.random.default_rng(7).permutation(len(E))]
    want, want_k = _union_find("path")
    assert want_k == 1 and not want.any()
    labels, k = _run(lib, nv, E)  # raises on "rounds did not converge"
    assert k == want_k
    assert np.array_equal(labels, want)


def test_star_with_the_largest_index_at_the_centre(lib):
    nv, E = B.cc_star()
    want, want_k = _union_find("star")
    assert want_k == 1
    labels, k = _run(lib, nv, E)
    assert k == want_k and np.array_equal(labels, want)


def test_many_small_components(lib):
    """70 001 vertices in components of 1 to 5, every edge twice, self loops; neither the vertex
    nor the edge count is a multiple of the wave or the block."""
    nv, E, planted, planted_k = B.cc_small_components()
    want, want_k = _union_find("small")
    assert want_k == planted_k and np.array_equal(want, planted)  # the reference agrees with the partition
    labels, k = _run(lib, nv, E)
    assert k == want_k and np.array_equal(labels, want)


def test_trivial_sizes(lib):
    labels, k = _run(lib, 1, np.zeros((0, 2), np.int32))
    assert k == 1 and labels.tolist() == [0]
    labels, k = _run(lib, 0, np.zeros((0, 2), np.int32))
    assert k == 0 and len(labels) == 0


def test_one_grid_stride_trip_more(lib):
    """nv = 16384 * 256 + 3 vertices and more edges than that: every grid-stride kernel of
    cc_labels takes a second trip. Sized by the launch cap, not by the smallest breaking shape;
    the expected labels follow from the planted partition."""
    nv, E, want, want_k = B.cc_grid_stride()
    assert nv == B.CC_LAUNCH_CAP + 3 and len(E) >= nv
    labels, k = _run(lib, nv, E)
    assert k == want_k
    assert np.array_equal(labels, want)
