"""GPU: the presence mark by 2^16-code slices with 16-bit entries (umi_len 9..12, n >= 2^20).

The bitmap of ClusterEngine.mark_bitmap is compared word for word with a host bitmap built
with numpy from the valid codes, as one call (phase 0) and as the bucket pass and the slice
pass on two streams (phase 1 then 2). The shapes sit just past the 2^20-row threshold of
the path: a ragged last uint4 and a ragged last bucket, bucket-multiple n, every row in
one run, runs on both sides of a slice boundary, invalid rows and codes outside 4^L.
"""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = (1 << 20) + 3  # ragged last uint4, ragged last bucket
BUCKET = 16384     # a multiple of the bucket pass's rows per workgroup, whichever it is built with


def host_bitmap(codes_h, L, reg=None):
    ok = codes_h < np.uint32(4 ** L)
    if reg is not None:
        ok &= reg
    bits = np.zeros(4 ** L, np.uint8)
    bits[codes_h[ok]] = 1
    return np.packbits(bits, bitorder="little").view(np.uint64)


def pack_reg(reg):
    """bool[n] -> the regular_bits words (bit r & 63 of word r >> 6)."""
    n = len(reg)
    padded = np.zeros((n + 63) // 64 * 64, np.uint8)
    padded[:n] = reg
    return np.packbits(padded, bitorder="little").view(np.int64)


_engines = {}


def engine(L):
    from rogtk_amd import device as D

    if L not in _engines:
        _engines[L] = D.ClusterEngine(L, min(N + 2 * BUCKET, 4 ** L), "cuda")
    return _engines[L]


def gpu_bitmaps(codes_h, L, reg=None):
    """(bitmap of phase 0, bitmap of phase 1 on one stream then phase 2 on another)."""
    import torch

    from rogtk_amd import device as D

    eng = engine(L)
    codes = torch.from_numpy(codes_h.view(np.int32)).cuda()
    regbits = None if reg is None else torch.from_numpy(pack_reg(reg)).cuda()
    batch = D.PackedBatch(codes, L, regbits)
    eng.local_bitmap.fill_(-1)
    whole = eng.mark_bitmap(batch).clone()
    eng.local_bitmap.fill_(-1)
    eng.mark_temp(batch.n).fill_(0xA5)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ev = torch.cuda.Event()
    eng.mark_bitmap(batch, stream=s1, phase=1)
    ev.record(s1)
    s2.wait_event(ev)
    split = eng.mark_bitmap(batch, stream=s2, phase=2)
    torch.cuda.synchronize()
    return whole.cpu().numpy().view(np.uint64), split.cpu().numpy().view(np.uint64)


def check(codes_h, L, reg=None):
    ref = host_bitmap(codes_h, L, reg)
    whole, split = gpu_bitmaps(codes_h, L, reg)
    assert np.array_equal(whole, ref), "phase 0"
    assert np.array_equal(split, ref), "phase 1 then 2"
    return ref


def random_codes(n, L, seed=5):
    return np.random.default_rng(seed).integers(0, 4 ** L, n, dtype=np.uint32)


@pytest.mark.parametrize("L", [12, 11, 9])
def test_random_codes(L):
    """256, 64 and 4 slices."""
    check(random_codes(N, L), L)


@pytest.mark.parametrize("L", [12, 9])
def test_all_one_code(L):
    """Every bucket is one run of all its rows."""
    ref = check(np.full(N, 4 ** L // 3 + 77, np.uint32), L)
    assert int(np.unpackbits(ref.view(np.uint8)).sum()) == 1


@pytest.mark.parametrize("L,k", [(12, 1), (12, 255), (11, 37), (9, 3)])
def test_two_codes_across_a_slice_boundary(L, k):
    codes_h = np.where(np.arange(N) % 3 == 0, k * 65536 - 1, k * 65536).astype(np.uint32)
    check(codes_h, L)


@pytest.mark.parametrize("L", [12, 11, 9])
def test_first_and_last_code(L):
    rng = np.random.default_rng(9)
    codes_h = np.where(rng.random(N) < 0.5, 0, 4 ** L - 1).astype(np.uint32)
    check(codes_h, L)


def test_region_bits_whole_bucket_invalid():
    reg = np.ones(N, bool)
    reg[BUCKET:2 * BUCKET] = False
    lone = 4 ** 12 - 5  # the invalid rows' code, which no valid row carries
    codes_h = np.random.default_rng(5).integers(0, lone, N, dtype=np.uint32)
    codes_h[BUCKET:2 * BUCKET] = lone
    ref = check(codes_h, 12, reg)
    assert not (int(ref[lone >> 6]) >> (lone & 63)) & 1


@pytest.mark.parametrize("L", [12, 11])
def test_region_bits_random_half(L):
    reg = np.random.default_rng(3).random(N) < 0.5
    check(random_codes(N, L), L, reg)


@pytest.mark.parametrize("L", [11, 9])
@pytest.mark.parametrize("with_reg", [False, True])
def test_codes_outside_the_code_space_set_nothing(L, with_reg):
    rng = np.random.default_rng(21)
    codes_h = random_codes(N, L)
    big = rng.random(N) < 0.3
    codes_h[big] = rng.integers(4 ** L, 2 ** 32, int(big.sum()), dtype=np.uint64).astype(np.uint32)
    codes_h[::1001] = 0xFFFFFFFF
    codes_h[1::1001] = 4 ** L
    codes_h[-1] = 4 ** L + 65535
    check(codes_h, L, np.ones(N, bool) if with_reg else None)


def test_only_codes_outside_the_code_space():
    whole, split = gpu_bitmaps(np.full(N, 4 ** 11, np.uint32), 11)
    assert not whole.any() and not split.any()


@pytest.mark.parametrize("n", [1 << 20, (1 << 20) + BUCKET])
def test_bucket_multiple_rows(n):
    check(random_codes(n, 12, seed=n & 0xFFFF), 12)
    reg = np.random.default_rng(4).random(n) < 0.5
    check(random_codes(n, 11, seed=8), 11, reg)


CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, {root!r})
from rogtk_amd import device as D
z = np.load({src!r})
out = {{}}
for L in (12, 11):
    codes = torch.from_numpy(z[f"codes{{L}}"].view(np.int32)).cuda()
    batch = D.PackedBatch(codes, L, torch.from_numpy(z["reg"]).cuda())
    eng = D.ClusterEngine(L, min(batch.n, 4 ** L), "cuda")
    out[f"bm{{L}}"] = eng.mark_bitmap(batch).cpu().numpy()
torch.cuda.synchronize()
np.savez({path!r}, **out)
"""


def test_old_path_gives_the_identical_bitmap(tmp_path):
    """The kernels kept from before the 16-bit path write the same bitmap: the 2^20-code
    slices over all rows with chunk partials and the OR pass, ROGTK_SLICE_BUCKETS=0 (read
    once per process, so in a child). While the A/B switch ROGTK_SLICE16=0 existed this test
    ran with it, against the 32-bit segment mode (green: profiles/r07_mark16_switch_gpu_tests.txt);
    the switch left with that mode once the 16-bit path had won."""
    reg = np.random.default_rng(6).random(N) < 0.7
    codes = {L: random_codes(N, L, seed=L) for L in (12, 11)}
    src, path = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, reg=pack_reg(reg), **{f"codes{L}": c for L, c in codes.items()})
    env = dict(os.environ, ROGTK_SLICE_BUCKETS="0")
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, src=src, path=path)], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(path)
    for L in (12, 11):
        whole, _ = gpu_bitmaps(codes[L], L, reg)
        assert np.array_equal(z[f"bm{L}"].view(np.uint64), whole), L
        assert np.array_equal(whole, host_bitmap(codes[L], L, reg)), L


def test_pipeline_cluster_ids_match_the_sequential_path():
    """A C2-shaped batch through UmiPipeline with the arguments the benchmark passes (two
    submits, so both slots run) against cluster_batch on one stream."""
    import torch

    from rogtk_amd import device as D
    from rogtk_amd import synth
    from rogtk_amd.pipeline import UmiPipeline

    L = 12
    codes_h = synth.umi_codes(N, L)
    codes = torch.from_numpy(codes_h.view(np.int32)).cuda()
    batch = D.PackedBatch(codes, L)
    eng = D.ClusterEngine(L, min(N, 4 ** L), "cuda")
    want = torch.empty(N, dtype=torch.int32, device="cuda")
    D.cluster_batch(eng, batch, want, 1)
    torch.cuda.synchronize()
    pipe = UmiPipeline(L, min(N, 4 ** L), N, "cuda", depth=2, target=b"ACGTACGTACGT", max_distance=1,
                       score_alone=True)
    for _ in range(2):
        pipe.submit(batch)
    pipe.drain()
    torch.cuda.synchronize()
    for slot in pipe.slots:
        assert torch.equal(slot.cid[:N], want)
