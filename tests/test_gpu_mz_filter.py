"""GPU: the minimizer filter's per-group decision (kmer_kernels.hip k_minimizer_filter,
read through rogtk_kmer_debug_filter: 1 emptied, 2 kept, 3 gave up, 0 untouched) held to the
plain model of tests/mz_spec.py, on families built to reach the list cap, the claim cap,
several 64-row passes, the split path, the batch boundaries, keys of several groups in one
table, a batch across two chunks of one wave and the row-length edges.

Every family runs through the block column (certificate from rogtk_pack_reads) and the
fused staging (certificate from k_pack_gather). Outputs are compared with the CPU oracle in
full; every candidate group must carry a decision and it must be the model's; no other
group may carry one; with the filter off the outputs are the same and nothing is decided."""
from __future__ import annotations

import numpy as np
import pytest

import mz_spec as S

pytestmark = pytest.mark.gpu
K = 17  # effective 32, the only K the filter runs at
_dev = {}


def _column(name):
    """The family's column, group offsets and block column on the device, once."""
    if name not in _dev:
        import torch

        from rogtk_amd import device as D

        fam = S.family(name)
        off = torch.from_numpy(fam.offsets).cuda()
        vals = torch.from_numpy(fam.values).cuda()
        go = torch.from_numpy(fam.go).cuda()
        pk = D.PackedReads(off, vals)
        assert pk.max_len == fam.max_len and pk.block_words == 8
        _dev[name] = (off, vals, go, pk)
    return _dev[name]


def _run(name, fused, filt):
    """One spectrum call with the decision buffer registered: (outputs, decisions)."""
    import torch

    from rogtk_amd import _lib
    from rogtk_amd import device as D

    fam = S.family(name)
    off, vals, go, pk = _column(name)
    G = fam.n_groups
    dec = torch.zeros(G, dtype=torch.uint8, device="cuda")
    _lib.call("rogtk_kmer_set_path", 1)
    _lib.call("rogtk_kmer_set_filter", filt)
    _lib.call("rogtk_kmer_debug_filter", D._p(dec), G)
    try:
        if fused:
            got = D.kmer_spectrum_fused(off, vals, go, K, fam.mc, fam.capacity(), -1)
        else:
            got = D.kmer_spectrum_blocks(pk, off, vals, go, K, fam.mc, fam.capacity())
        torch.cuda.synchronize()
    finally:
        _lib.call("rogtk_kmer_debug_filter", None, 0)
        _lib.call("rogtk_kmer_set_filter", 1)
    km = got["kmers"].cpu().numpy().view(np.uint64).reshape(-1, 2)
    out = {"group_offsets": got["entry_offsets"].cpu().numpy(), "stats": got["stats"].cpu().numpy(),
           "kmer_hi": km[:, 0], "kmer_lo": km[:, 1], "exts": got["exts"].cpu().numpy(),
           "counts": got["counts"].cpu().numpy().view(np.uint16)}
    return out, dec.cpu().numpy()


def _uncertified(name, g):
    """For the message of a candidate left undecided: its rows without the repeat
    certificate (block meta bit 33), which the builder would then have to avoid."""
    fam = S.family(name)
    meta = _column(name)[3].blocks.view(-1, 8)[:, 0].cpu().numpy().view(np.uint64)
    return [r for r in range(int(fam.go[g]), int(fam.go[g + 1])) if not (int(meta[r]) >> 33) & 1]


def _assert_oracle(name, out):
    ref = S.oracle_ref(name, K)
    for f in ("group_offsets", "stats", "kmer_hi", "kmer_lo", "exts", "counts"):
        assert np.array_equal(out[f], ref[f]), (name, f)


CASES = [(n, f) for n in S.BUILDERS for f in (False, True)]
IDS = [f"{n}-{'fused' if f else 'blocks'}" for n, f in CASES]


@pytest.mark.parametrize("name,fused", CASES, ids=IDS)
def test_filter_decisions_match_the_model(name, fused):
    fam = S.family(name)
    out, dec = _run(name, fused, 1)
    print(name, "fused" if fused else "blocks", "decisions:", np.bincount(dec, minlength=4).tolist())
    _assert_oracle(name, out)
    # every candidate has a decision, nothing else has one
    cand = np.array(fam.candidates())
    mask = np.zeros(fam.n_groups, bool)
    mask[cand] = True
    missing = cand[dec[cand] == 0]
    assert len(missing) == 0, [(int(g), fam.groups[int(g)].role, _uncertified(name, int(g))) for g in missing]
    touched = np.flatnonzero((dec != 0) & ~mask)
    assert len(touched) == 0, [(int(g), int(dec[g])) for g in touched[:10]]
    # the decision is the model's
    for g in cand.tolist():
        info = fam.groups[g]
        d = S.decision(fam.rows_of(g), fam.mc)
        want = (1,) if d.verdict == "emptied" else (3,) if info.gave_up else (2, 3)
        assert int(dec[g]) in want, (g, info.role, int(dec[g]), d)


@pytest.mark.parametrize("name,fused", CASES, ids=IDS)
def test_filter_off_same_outputs_nothing_decided(name, fused):
    out, dec = _run(name, fused, 0)
    _assert_oracle(name, out)
    assert not dec.any()
