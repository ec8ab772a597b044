"""GPU: the assign's dominant-cluster bitmap (k_assign<0, G, true>).

The roots scan samples the roots of 256 evenly spaced words (word k * words / 256) and takes
their mode as the dominant cluster; k_word_label sets one bit per 64-code word whose present
codes all belong to it; the assign copies the bits into LDS and gives such rows the dominant
label without a gather. Every case here compares the ids of cluster_batch and of UmiPipeline
with the oracle's and with the ids of a child process that runs ROGTK_ASSIGN_DOM=0 (the
instance without the bitmap; the switch is read once per process).

The code sets are built so that the sample meets them. In a code of L bases, base position 0
is the two lowest bits. A word is 64 codes (positions 0..2); the sampled words are those
with positions 3..L-5 zero, one per combination of the top four positions. The family
`giant(L)` fills bits 0..7 of each of them (position 2 = A, position 1 in {A, C}): 2048
codes, connected, present in every sampled word. Codes elsewhere in a word (bit 31, 47, 63:
positions 1 and 0 = T) are two edits from every family code of the word.
"""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = (1 << 18) + 3  # ragged last uint4


def P():
    from oracle import pyoracle

    return pyoracle


# ------------------------------------------------------------------ code sets (host, numpy)
def hamming(codes, c):
    x = codes.astype(np.uint64) ^ np.uint64(c)
    x = np.ascontiguousarray((x | (x >> np.uint64(1))) & np.uint64(0x5555555555555555))
    return np.unpackbits(x.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1)


def drop_near(codes, c):
    """codes without those within one edit of c."""
    return codes[hamming(codes, c) > 1]


def giant(L, tops=range(256), bits=range(8)):
    """The family: top four positions `tops`, positions 3..L-5 zero, word bits `bits`."""
    t = np.array(list(tops), np.uint32)[:, None] << np.uint32(2 * (L - 4))
    return (t | np.array(list(bits), np.uint32)[None, :]).reshape(-1)


def isolated(L, k, seed):
    """k codes pairwise two edits apart (position 0 is a checksum of the others) with at least
    two non-zero positions among 3..L-5 (two edits from every family code), plus code 0 and
    4^L - 1 and nothing within one edit of those two."""
    rng = np.random.default_rng(seed)
    hi = np.unique(rng.integers(0, 4 ** (L - 1), 4 * k, dtype=np.uint32))
    digits = (hi[:, None] >> (2 * np.arange(L - 1, dtype=np.uint32))[None, :]) & 3
    codes = (hi << np.uint32(2)) | (digits.sum(axis=1) & 3).astype(np.uint32)
    mid = (codes[:, None] >> (2 * np.arange(3, L - 4, dtype=np.uint32))[None, :]) & 3
    codes = codes[(mid != 0).sum(axis=1) >= 2]
    codes = drop_near(drop_near(codes, 0), 4 ** L - 1)
    codes = codes[rng.permutation(len(codes))[:k]]
    assert len(codes) == k
    return np.concatenate([codes, np.array([0, 4 ** L - 1], np.uint32)])


def rows_of(distinct, n, seed, heavy=None):
    """n rows: every distinct code once, the rest drawn from `heavy` (default: all of them)."""
    rng = np.random.default_rng(seed)
    distinct = np.unique(distinct)
    pool = distinct if heavy is None else heavy
    rows = np.concatenate([distinct, rng.choice(pool, n - len(distinct))]).astype(np.uint32)
    return rows[rng.permutation(n)]


def family_rows(L, seed, extra=()):
    fam = drop_near(giant(L), 0)  # code 0 stays on its own
    iso = isolated(L, 20000 if L > 9 else 4000, seed)
    parts = [fam, iso] + [np.asarray(e, np.uint32) for e in extra]
    return rows_of(np.concatenate(parts), N, seed, heavy=np.concatenate([np.tile(fam, 20), iso]))


def edge_words(L=12):
    """Words next to sampled ones (position 3 = C: word t * 4^(L-7) + 1), so their codes at
    bits 0..7 are one edit from the family. Top-position combinations t two edits apart keep
    the planted codes of different words apart. Returns (codes, probes): probes name the code
    whose id must differ from the family's, or equal it."""
    word = lambda t: np.uint32((t << (2 * (L - 4))) | 64)
    low = np.arange(8, dtype=np.uint32)
    out, other, same = [], [], []
    # one code of another cluster in the upper half of the word; in the lower half (twice);
    # one in each half (adjacent to each other: a cluster of two)
    for t, exc in ((5, [63]), (10, [26]), (15, [31]), (18, [63, 31])):
        out += [word(t) | low, word(t) | np.array(exc, np.uint32)]
        other += [int(word(t) | e) for e in exc]
        same += [int(word(t))]
    # two adjacent exceptions (one cluster of two), three exceptions (the mask form)
    out += [word(33) | low, word(33) | np.array([63, 47], np.uint32)]
    out += [word(36) | low, word(36) | np.array([63, 47, 31], np.uint32)]
    other += [int(word(33) | 63), int(word(36) | 31)]
    # the family code is the exception of a word that belongs to another cluster
    out += [word(43) | np.array([0], np.uint32), word(43) | np.array([63, 47, 31, 62], np.uint32)]
    other += [int(word(43) | 62)]
    same += [int(word(43))]
    # a word of family codes only, away from the sample
    out += [word(54) | low]
    same += [int(word(54) | 3)]
    return np.concatenate(out), (other, same)


def chain(rng, L, start_top, low, length):
    """Self-avoiding walk over the top four positions from start_top, the rest = low."""
    cur, seen, path = start_top, {start_top}, [start_top]
    while len(path) < length:
        for _ in range(64):
            nxt = cur ^ (int(rng.integers(1, 4)) << (2 * int(rng.integers(4))))
            if nxt not in seen:
                break
        else:
            break
        seen.add(nxt)
        path.append(nxt)
        cur = nxt
    return np.array([(t << (2 * (L - 4))) | low for t in path], np.uint32)


def build_case(name):
    """name -> (L, codes u32[n], valid bool[n] or None)."""
    if name.startswith("giant"):
        L = int(name[5:])
        return L, family_rows(L, L), None
    if name == "edges":
        extra, _ = edge_words()
        return 12, family_rows(12, 3, [extra]), None
    if name == "none":
        return 12, rows_of(isolated(12, 60000, 7), N, 7), None
    if name == "two_equal":
        a = giant(12, range(0, 128), range(0, 8))
        b = giant(12, range(128, 256), range(56, 64))
        return 12, rows_of(np.concatenate([drop_near(a, 0), b, isolated(12, 20000, 8)]), N, 8), None
    if name == "invalid":
        rows = family_rows(12, 4)
        rng = np.random.default_rng(4)
        valid = rng.random(N) < 0.8
        junk = rng.integers(0, 4 ** 12, N, dtype=np.uint32)
        junk[::3] = giant(12)[5]  # an invalid row with a family code still gets no id
        return 12, np.where(valid, rows, junk), valid
    if name == "L13":
        return 13, family_rows(13, 13), None
    if name == "chains":
        # walks over the top positions hang off the family: through bit 63 -> 15 -> 3 of word
        # 0's neighbourhood the first walk joins it, so the family's cluster is final (and its
        # label, which counts the roots before it) only after many rounds
        rng = np.random.default_rng(12)
        top0 = 64  # top positions (1, 0, 0, 0): away from code 0's neighbourhood
        base = top0 << 16
        walks = [chain(rng, 12, top0, 63, 200)] + [chain(rng, 12, int(rng.integers(256)), int(m) << 6 | 63, 200)
                                                   for m in (1 + 4, 2 + 8, 3 + 12)]
        link = np.array([base | 15, base | 3], np.uint32)
        return 12, family_rows(12, 5, walks + [link]), None
    raise KeyError(name)


CASES = ["giant12", "giant11", "giant9", "edges", "none", "two_equal", "invalid", "L13", "chains"]


# ------------------------------------------------------------------ device
def pack_reg(reg):
    n = len(reg)
    padded = np.zeros((n + 63) // 64 * 64, np.uint8)
    padded[:n] = reg
    return np.packbits(padded, bitorder="little").view(np.int64)


def device_batch(L, codes_h, valid):
    import torch

    from rogtk_amd import device as D

    codes = torch.from_numpy(codes_h.view(np.int32)).cuda()
    reg = None if valid is None else torch.from_numpy(pack_reg(valid)).cuda()
    return D.PackedBatch(codes, L, reg)


def gpu_ids(name):
    """{"batch": ids of cluster_batch, "deferred": ids of a deferred assign after one
    speculative round, "pipe": ids of both slots of a 2-deep UmiPipeline}."""
    import torch

    from rogtk_amd import device as D
    from rogtk_amd.pipeline import UmiPipeline

    L, codes_h, valid = build_case(name)
    n = len(codes_h)
    batch = device_batch(L, codes_h, valid)
    eng = D.ClusterEngine(L, min(n, 4 ** L), "cuda")
    cid = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    D.cluster_batch(eng, batch, cid, 1)
    torch.cuda.synchronize()
    out = {"batch": cid.cpu().numpy().view(np.uint32), "n_clusters": np.int64(eng.stats()["n_clusters"])}
    cid.fill_(-7)
    try:
        D.set_spec_rounds(1)
        eng.resolve(eng.mark_bitmap(batch), 1, 1)
        eng.assign(batch, cid, deferred=True)
        redone = eng.sync()
    finally:
        D.set_spec_rounds(0)
    torch.cuda.synchronize()
    out["deferred"] = cid.cpu().numpy().view(np.uint32)
    out["redone"] = np.int64(redone)
    pipe = UmiPipeline(L, min(n, 4 ** L), n, "cuda", depth=2, target=b"ACGTACGTACGTA"[:L], max_distance=1,
                       score_alone=True)
    for _ in range(2):
        pipe.submit(batch)
    pipe.drain()
    torch.cuda.synchronize()
    for k, slot in enumerate(pipe.slots):
        out[f"pipe{k}"] = slot.cid[:n].cpu().numpy().view(np.uint32)
    return out


_oracle = {}


def oracle_ids(name):
    """(ids with 0xFFFFFFFF on the invalid rows, n_clusters), once per case."""
    from rogtk_amd import synth

    if name not in _oracle:
        L, codes_h, valid = build_case(name)
        keep = np.ones(len(codes_h), bool) if valid is None else valid
        col = P().StrCol.from_fixed(synth.codes_to_ascii(codes_h[keep], L))
        rc, rv, rk, _ = P().umi_cluster(col, L, 1, threads=min(16, os.cpu_count() or 1))
        assert rv.all()
        ids = np.full(len(codes_h), 0xFFFFFFFF, np.uint32)
        ids[keep] = rc
        _oracle[name] = (ids, rk)
    return _oracle[name]


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import test_gpu_assign_dom as T
out = {{}}
for name in T.CASES:
    for k, v in T.gpu_ids(name).items():
        out[name + "." + k] = v
for k, v in enumerate(T.rotating_pipeline()):
    out["rotate." + str(k)] = v
np.savez({path!r}, **out)
"""


@pytest.fixture(scope="module")
def without_bitmap(tmp_path_factory):
    """Every case's ids from a child process with ROGTK_ASSIGN_DOM=0."""
    path = str(tmp_path_factory.mktemp("dom") / "off.npz")
    env = dict(os.environ, ROGTK_ASSIGN_DOM="0")
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), path=path)],
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return np.load(path)


def check_case(name, off):
    want, k = oracle_ids(name)
    got = gpu_ids(name)
    assert int(got["n_clusters"]) == k
    for key in ("batch", "deferred", "pipe0", "pipe1"):
        bad = np.nonzero(got[key] != want)[0]
        assert len(bad) == 0, f"{name}.{key}: {len(bad)} rows differ from the oracle, first {bad[:5]}"
        assert np.array_equal(got[key], off[f"{name}.{key}"]), f"{name}.{key}: differs from ROGTK_ASSIGN_DOM=0"
    return got, want


@pytest.mark.parametrize("L", [12, 11, 9])
def test_giant_and_isolated_codes(L, without_bitmap):
    """The family (2047 codes in one cluster, about two thirds of the rows) and isolated codes
    two edits apart, code 0 and 4^L - 1 among them."""
    name = f"giant{L}"
    _, want = check_case(name, without_bitmap)
    _, codes_h, _ = build_case(name)
    fam = want[codes_h == giant(L)[9]][0]
    assert (want == fam).sum() > N // 2
    for c in (0, 4 ** L - 1):
        assert want[codes_h == c][0] != fam


def test_word_edges(without_bitmap):
    """Words of family codes with one, two (apart and adjacent) and three codes of other
    clusters, in either half of the word; a word of another cluster with one family code; a
    family-only word the sample does not meet."""
    _, want = check_case("edges", without_bitmap)
    _, codes_h, _ = build_case("edges")
    _, (other, same) = edge_words()
    fam = want[codes_h == giant(12)[9]][0]
    for c in other:
        assert want[codes_h == c][0] != fam, hex(c)
    for c in same:
        assert want[codes_h == c][0] == fam, hex(c)


def test_no_dominant_cluster(without_bitmap):
    """Every code isolated: no root holds a quarter of the sample, the marker says none."""
    _, want = check_case("none", without_bitmap)
    assert np.bincount(want).max() < N // 100


def test_two_components_of_equal_size(without_bitmap):
    """Half the sampled words belong to each; whichever is picked, the ids are the oracle's."""
    check_case("two_equal", without_bitmap)


def test_invalid_rows(without_bitmap):
    """A fifth of the rows have their region bit clear (and some other code): id 0xFFFFFFFF."""
    got, _ = check_case("invalid", without_bitmap)
    _, _, valid = build_case("invalid")
    assert (got["batch"][~valid] == 0xFFFFFFFF).all() and (got["batch"][valid] != 0xFFFFFFFF).all()


def test_umi_len_13_takes_the_instance_without_bitmap(without_bitmap):
    check_case("L13", without_bitmap)


def test_more_rounds_than_the_speculative_ones(without_bitmap):
    """Walks of 200 steps hang off the family: one speculative round does not finish them, so
    the deferred assign runs on labels and a bitmap that are not final, and sync() / drain()
    rebuild both."""
    got, _ = check_case("chains", without_bitmap)
    assert int(got["redone"]) == 1


def rotating_pipeline():
    """Three batches with different dominant clusters through two slots; the ids of each."""
    import torch

    from rogtk_amd.pipeline import UmiPipeline

    sets = rotating_sets()
    pipe = UmiPipeline(12, N, N, "cuda", depth=2, target=b"ACGTACGTACGT", max_distance=1, score_alone=True)
    batches = [device_batch(12, rows, None) for rows in sets]
    first = pipe.submit(batches[0])
    pipe.submit(batches[1])
    out = [pipe.settle(first)[:N].clone()]
    pipe.submit(batches[2])
    pipe.drain()
    torch.cuda.synchronize()
    out += [pipe.slots[1].cid[:N], pipe.slots[0].cid[:N]]
    return [o.cpu().numpy().view(np.uint32) for o in out]


def rotating_sets():
    fams = [giant(12, range(256), range(0, 8)), giant(12, range(256), range(56, 64)), giant(12, range(256), range(24, 32))]
    return [rows_of(np.concatenate([f, isolated(12, 20000, 20 + k)]), N, 20 + k, heavy=f) for k, f in enumerate(fams)]


def test_pipeline_slots_keep_their_own_bitmap(without_bitmap):
    from rogtk_amd import synth

    got = rotating_pipeline()
    for k, rows in enumerate(rotating_sets()):
        rc, _, _, _ = P().umi_cluster(P().StrCol.from_fixed(synth.codes_to_ascii(rows, 12)), 12, 1,
                                      threads=min(16, os.cpu_count() or 1))
        assert np.array_equal(got[k], rc), f"batch {k}"
        assert np.array_equal(got[k], without_bitmap[f"rotate.{k}"]), f"batch {k} against ROGTK_ASSIGN_DOM=0"
