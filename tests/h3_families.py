"""Structured UMI code sets for the Hamming<=1 clustering (H3) tests, and a second
reference for them (numpy only; a plain module, no fixtures).

Uniform random codes percolate: a Hamming-1 graph has 3 L neighbours per code, so past a
few percent density the answer is one giant component. The families here are dense AND
fall into many clusters, because a parity rule forbids every edge that would join two of
them. Notation: d_p = (code >> 2p) & 3 is the digit at position p (p = 0 the last base),
c_p = d_p >> 1 its class ({A,C} / {G,T}); a 64-code word is the codes that share the
digits p >= 3, its index is code >> 6.

Every generator returns sorted distinct uint32 codes and is a pure function of its
arguments (seed included).
"""
from __future__ import annotations

import numpy as np

# the in-word mask {d_2 < 2 and d_1 < 2} | {d_2 >= 2 and d_1 >= 2}: 32 codes, two components
# (a substitution at d_1 or d_2 alone leaves the mask), 80 in-word edges
_b = np.arange(64)
TWOBOX_MASK = ((_b >> 4) < 2) == (((_b >> 2) & 3) < 2)
del _b


def codes_to_ascii(codes: np.ndarray, L: int) -> np.ndarray:
    """(n, L) uint8 ACGT rows of the codes (first base = the highest digit)."""
    shifts = np.arange(L - 1, -1, -1, dtype=np.uint32) * 2
    return np.frombuffer(b"ACGT", dtype=np.uint8)[(codes[:, None].astype(np.uint32) >> shifts[None, :]) & 3]


def _digit_sum(x: np.ndarray, lo: int, hi: int, cls: bool = False) -> np.ndarray:
    """Sum over positions lo <= p < hi of d_p (or of c_p) of the values x."""
    s = np.zeros(x.shape, dtype=np.uint32)
    for p in range(lo, hi):
        d = (x >> np.uint32(2 * p)) & np.uint32(3)
        s += (d >> np.uint32(1)) if cls else d
    return s


def _from_present(present: np.ndarray) -> np.ndarray:
    return np.flatnonzero(present.reshape(-1)).astype(np.uint32)


def _word_masks_to_codes(masks: np.ndarray) -> np.ndarray:
    """masks: (n_words, 64) bool, code = word * 64 + bit."""
    return _from_present(masks)


def n_words(L: int) -> int:
    if L < 3:
        raise ValueError("the word families need L >= 3")
    return 4 ** (L - 3)


def parity_cubes(L: int, lo: int = 8, keep: float = 1.0, seed: int = 0) -> np.ndarray:
    """Codes whose class sum over p < min(lo, L) is even and whose digit sum over p >= lo is
    0 mod 4, each kept with probability `keep`. One substitution always changes one of the
    two sums, so the components are the 2^min(lo, L)-code class cubes (one per even class
    vector and admissible high part), never linked across the high digits. For lo >= 6 every
    64-code word holds four 8-code components and every populated tile is 50% * keep dense."""
    x = np.arange(4 ** L, dtype=np.uint32)
    present = (_digit_sum(x, 0, min(lo, L), cls=True) & 1) == 0
    if L > lo:
        present &= (_digit_sum(x, lo, L) & 3) == 0
    if keep < 1.0:
        present &= np.random.default_rng([seed, L, lo, 1]).random(x.size) < keep
    return _from_present(present)


def mod4(L: int, extra: float = 0.0, seed: int = 0) -> np.ndarray:
    """Digit sum 0 mod 4 (25% of the codes, no two adjacent: every one a singleton, every
    word 16 scattered codes), plus each other code with probability `extra`."""
    x = np.arange(4 ** L, dtype=np.uint32)
    present = (_digit_sum(x, 0, L) & 3) == 0
    if extra > 0.0:
        present |= np.random.default_rng([seed, L, 2]).random(x.size) < extra
    return _from_present(present)


def _random_boxes(rng, n: int) -> np.ndarray:
    """n random axis-aligned boxes of the 4x4x4 in-word cube as (n, 64) bool masks."""
    b = np.arange(64)
    out = np.ones((n, 64), dtype=bool)
    for q in range(3):
        a0 = rng.integers(0, 4, n)
        a1 = rng.integers(0, 4, n)
        lo_, hi_ = np.minimum(a0, a1), np.maximum(a0, a1)
        dq = (b >> (2 * q)) & 3
        out &= (dq[None, :] >= lo_[:, None]) & (dq[None, :] <= hi_[:, None])
    return out


def boxes(L: int, p_empty: float = 0.1, two: bool = False, seed: int = 0) -> np.ndarray:
    """Each word is empty (probability p_empty) or one random box (two: the union of two)
    of its 4x4x4 cube: words of one or two in-word components."""
    rng = np.random.default_rng([seed, L, 3, int(two)])
    nw = n_words(L)
    masks = _random_boxes(rng, nw)
    if two:
        masks |= _random_boxes(rng, nw)
    masks &= (rng.random(nw) >= p_empty)[:, None]
    return _word_masks_to_codes(masks)


def mixed(L: int, seed: int = 0) -> np.ndarray:
    """Per word, uniformly one of: empty, full, 7 scattered codes, one box, the two-box
    mask thinned at 0.9, 30% random: every kind of word next to every other."""
    rng = np.random.default_rng([seed, L, 4])
    nw = n_words(L)
    kind = rng.integers(0, 6, nw)
    masks = np.zeros((nw, 64), dtype=bool)
    masks[kind == 1] = True
    scattered = np.argsort(rng.random((nw, 64)), axis=1) < 7
    masks[kind == 2] = scattered[kind == 2]
    box = _random_boxes(rng, nw)
    masks[kind == 3] = box[kind == 3]
    thin = TWOBOX_MASK[None, :] & (rng.random((nw, 64)) < 0.9)
    masks[kind == 4] = thin[kind == 4]
    rnd = rng.random((nw, 64)) < 0.3
    masks[kind == 5] = rnd[kind == 5]
    return _word_masks_to_codes(masks)


def twobox(L: int, frac: float = 1.0, seed: int = 0) -> np.ndarray:
    """A fraction `frac` of the words hold TWOBOX_MASK, the others are empty."""
    nw = n_words(L)
    on = np.ones(nw, dtype=bool) if frac >= 1.0 else np.random.default_rng([seed, L, 5]).random(nw) < frac
    return _word_masks_to_codes(on[:, None] & TWOBOX_MASK[None, :])


def chains(L: int, seed: int = 0) -> np.ndarray:
    """Groups of 4 words along one word position (chosen by the seed), the words of a group
    linked in a path in a random order: three codes a, b, c on one in-word line, the words
    {a}, {a, b}, {b, c}, {c} (each one component) dealt over the group by a random
    permutation. The groups present have a digit sum 0 mod 4 over the other word positions,
    so no two are adjacent: every group is one cluster of 6 codes, which the 4-word closure
    of one-component words must find whatever the order of the path (L = 3: the one word
    {a, b, c})."""
    rng = np.random.default_rng([seed, L, 6])
    ndig = L - 3
    nw = n_words(L)
    masks = np.zeros((nw, 64), dtype=bool)

    def line3():
        q = int(rng.integers(0, 3))
        base = int(rng.integers(0, 64)) & ~(3 << (2 * q))
        a, b, c = (base | (int(v) << (2 * q)) for v in rng.permutation(4)[:3])
        return a, b, c

    if ndig == 0:
        masks[0, list(line3())] = True
        return _word_masks_to_codes(masks)
    pw = seed % ndig
    w = np.arange(nw, dtype=np.uint32)
    rest = _digit_sum(w, 0, ndig) - ((w >> np.uint32(2 * pw)) & np.uint32(3))
    for w0 in np.flatnonzero((((w >> np.uint32(2 * pw)) & np.uint32(3)) == 0) & ((rest & 3) == 0)):
        a, b, c = line3()
        order = rng.permutation(4)
        for v, members in zip(order, ([a], [a, b], [b, c], [c])):
            masks[int(w0) + (int(v) << (2 * pw)), members] = True
    return _word_masks_to_codes(masks)


# two 2-code components of a word: {0, 1} and {42, 43} (3 digits apart), two edges, both bridges
DOMINO_CODES = (0, 1, 42, 43)


def bridge_overflow(L: int, n_twobox: int, n_domino: int) -> np.ndarray:
    """Per 4^8-code tile (L >= 8), over its 256 words of digit sum 0 mod 4 (no two adjacent, so
    every component lies inside one word) in ascending order: n_twobox words of TWOBOX_MASK
    (80 in-word edges each, none a bridge), then n_domino words of DOMINO_CODES (2 edges each,
    both bridges), the rest full (one component: no listed edge). A kernel that lists the
    in-word edges in word order has its edges 80 * n_twobox .. 80 * n_twobox + 2 * n_domino - 1
    all bridges: put an edge-list boundary among them and an edge lost or doubled at the
    boundary splits a domino. Clusters per tile: 2 * n_twobox + 2 * n_domino + the full words."""
    if L < 8 or n_twobox + n_domino > 256:
        raise ValueError("bridge_overflow: L >= 8, at most 256 words per tile")
    nw = n_words(L)
    w = np.arange(nw, dtype=np.uint32)
    present = np.flatnonzero((_digit_sum(w, 0, L - 3) & 3) == 0)
    # rank of each present word inside its tile of 1024 words
    rank = np.arange(present.size) - np.searchsorted(present, (present >> 10) << 10)
    masks = np.zeros((nw, 64), dtype=bool)
    domino = np.zeros(64, dtype=bool)
    domino[list(DOMINO_CODES)] = True
    masks[present[rank < n_twobox]] = TWOBOX_MASK
    masks[present[(rank >= n_twobox) & (rank < n_twobox + n_domino)]] = domino
    masks[present[rank >= n_twobox + n_domino]] = True
    return _word_masks_to_codes(masks)


def masked(codes: np.ndarray, L: int, how: str) -> np.ndarray:
    """The codes whose word-index digits (p >= 3) pass `how`. "parity": even class sum, so the
    present words form disjoint class cubes; "mod4": digit sum 0 mod 4, so no two present
    words are adjacent and every component lies inside one word."""
    w = (np.asarray(codes, dtype=np.uint32) >> np.uint32(6))
    if how == "parity":
        ok = (_digit_sum(w, 0, L - 3, cls=True) & 1) == 0
    elif how == "mod4":
        ok = (_digit_sum(w, 0, L - 3) & 3) == 0
    else:
        raise ValueError(how)
    return np.asarray(codes, dtype=np.uint32)[ok]


def with_ballast(codes: np.ndarray, L: int) -> np.ndarray:
    """codes without those whose top digit is 3, plus parity_cubes(L - 1, 8, 1.0) under top
    digit 3 (L >= 9): one 4^8-code tile then holds 32768 codes, more than any 8-position
    instance takes, so the 7-position tiling runs over the whole space."""
    if L < 9:
        raise ValueError("ballast needs L >= 9")
    top = np.uint32(2 * (L - 1))
    codes = np.asarray(codes, dtype=np.uint32)
    kept = codes[(codes >> top) != 3]
    return np.concatenate([kept, parity_cubes(L - 1, 8, 1.0) | (np.uint32(3) << top)])


def densest_tile(codes: np.ndarray, positions: int) -> int:
    """Most distinct codes in one tile of 4^positions codes."""
    u = np.unique(np.asarray(codes, dtype=np.uint32))
    return int(np.bincount(u >> np.uint32(2 * positions)).max()) if u.size else 0


def grid_components(codes: np.ndarray, L: int):
    """Hamming<=1 components of regular codes by label propagation over the 4^L grid
    (L <= 12): every present cell holds its own code, absent cells all-ones; until nothing
    changes, every present cell takes the minimum over each of its L lines of 4. No
    union-find and no edge list: a structurally different check of the oracle. Returns
    (ids, n_clusters): dense ids by each component's smallest code, one per entry of
    `codes` (duplicates allowed, any order)."""
    if not 1 <= L <= 12:
        raise ValueError("grid_components: 1 <= L <= 12")
    codes = np.asarray(codes, dtype=np.uint32)
    absent = np.uint32(0xFFFFFFFF)
    lab = np.full(4 ** L, absent, dtype=np.uint32)
    lab[codes] = codes
    present = lab != absent
    lab = lab.reshape((4,) * L)
    present = present.reshape((4,) * L)
    while True:
        before = lab.copy()
        for ax in range(L):
            line = lab.min(axis=ax, keepdims=True)
            np.minimum(lab, line, out=lab, where=present)
        if np.array_equal(before, lab):
            break
    roots = lab.reshape(-1)[codes]
    uniq, ids = np.unique(roots, return_inverse=True)
    return ids.astype(np.uint32), int(uniq.size)


def cluster_sizes(ids: np.ndarray) -> np.ndarray:
    """Codes per cluster, from the ids of DISTINCT codes."""
    return np.bincount(ids)


def _nonempty(make):
    """make(L, seed) with the seed moved on (by 1000s) until the code set is not empty: at
    L = 3, 4 the word families have a handful of words, which a draw can leave all empty."""
    def build(L, s):
        codes = make(L, s)
        while codes.size == 0:
            s += 1000
            codes = make(L, s)
        return codes
    return build


# (name, builder(L, seed)): the families as the tests use them at any L >= 3. The word
# families are masked, otherwise they percolate into one cluster.
FAMILIES = [
    ("parity_cubes", lambda L, s: parity_cubes(L, 8, 1.0 if s == 0 else 0.85 if s % 2 else 0.6, seed=s)),
    ("mod4", lambda L, s: mod4(L, 0.0 if s == 0 else 0.03, seed=s)),
    ("boxes_parity", _nonempty(lambda L, s: masked(boxes(L, 0.1, two=bool(s & 1), seed=s), L, "parity"))),
    ("boxes_mod4", _nonempty(lambda L, s: masked(boxes(L, 0.1, two=bool(s & 1), seed=s), L, "mod4"))),
    ("mixed_parity", _nonempty(lambda L, s: masked(mixed(L, seed=s), L, "parity"))),
    ("mixed_mod4", _nonempty(lambda L, s: masked(mixed(L, seed=s), L, "mod4"))),
    ("twobox_parity", _nonempty(lambda L, s: masked(twobox(L, 1.0 if s == 0 else 0.7, seed=s), L, "parity"))),
    ("chains", lambda L, s: chains(L, seed=s)),
    ("twobox_mod4", _nonempty(lambda L, s: masked(twobox(L, 1.0 if s == 0 else 0.7, seed=s), L, "mod4"))),
]
