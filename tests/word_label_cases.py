"""Planted code sets that pin the word-label forms of the max-distance-1 assign.

The assign labels rows through one u32 per 64-code word (decode_word_label in
rogtk_internal.h; DESIGN.md "Word-label forms and their limits"). Which form a word takes
depends on how many of its codes lie outside the word's majority cluster and on how large
the majority's label is. This module builds code sets whose cluster ids are known by
construction, so a test can put a chosen word shape at a chosen label:

* F fillers, singleton clusters with ids 0..F-1, that sit below every gadget;
* a few dozen gadget words (kinds a..j, see WORDS) whose ids follow the fillers.

Codes are 2 bits per base, first base in the highest digit (A=0, C=1, G=2, T=3), held as
int64 here; to_int32 gives the bit pattern the device entry points take. Only numpy is
needed; fillers() also runs on a torch device so that millions of them never exist on the
host.
"""
from __future__ import annotations

import numpy as np

_ACGT = np.frombuffer(b"ACGT", np.uint8)


def _s3(s: str) -> int:
    """The 6-bit in-word code (= bit in the word) of a 3-letter suffix."""
    v = 0
    for ch in s:
        v = v * 4 + "ACGT".index(ch)
    return v


def _sfx(*names):
    return [_s3(s) for s in names]


# ---------------------------------------------------------------------------- fillers
def filler_capacity(L: int, sparse: bool = False) -> int:
    """Fillers available: 9 * 4^(L-3), or 9 * 4^(L-5) with one filler per word."""
    return 9 * 4 ** (L - 5 if sparse else L - 3)


def fillers(L: int, F: int, sparse: bool = False, device=None):
    """The F lowest fillers in ascending code order (int64; numpy, or torch on `device`), so
    a filler's cluster id is its index.

    Fillers are the codewords of the length-L parity code (last digit = minus the sum of
    the others mod 4) whose first two digits lie in {A, C, G}: pairwise distance >= 2, so
    each is its own cluster, and at least 2 digits from every gadget (those start with TT).
    Dense: every filler word holds 16 of them (digits L-3 and L-2 free). sparse: only the
    codewords with A at both of those digits, one per word."""
    if not 0 <= F <= filler_capacity(L, sparse):
        raise ValueError(f"F={F} outside 0..{filler_capacity(L, sparse)} (L={L}, sparse={sparse})")
    if device is None:
        k = np.arange(F, dtype=np.int64)
    else:
        import torch

        k = torch.arange(F, dtype=torch.int64, device=device)
    free = L - 5 if sparse else L - 3  # free digits after the first two
    M = 4 ** free
    q = k // M
    pre = ((q // 3) * 4 + q % 3) * M + (k - q * M)  # every digit but the parity digit
    s = k * 0
    for i in range(free + 2):
        s = s + ((pre >> (2 * i)) & 3)
    if sparse:
        pre = pre * 16
    return pre * 4 + ((-s) & 3)


def to_int32(codes):
    """int64 codes -> the int32 bit pattern of their uint32 value (numpy or torch). At L = 16
    the gadget codes (first bases TT) have the top bit set and come out negative."""
    if isinstance(codes, np.ndarray):
        return codes.astype(np.uint32).view(np.int32)
    import torch

    return ((codes + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32)


def codes_to_ascii(codes: np.ndarray, L: int) -> np.ndarray:
    """(n, L) uint8 ASCII of int64 / uint32 codes."""
    shifts = np.arange(L - 1, -1, -1, dtype=np.int64) * 2
    return _ACGT[(np.asarray(codes, dtype=np.int64)[:, None] >> shifts[None, :]) & 3]


# ---------------------------------------------------------------------------- gadgets
# One entry per gadget: kind -> the words it plants, each (link, majority suffixes, other
# suffixes). link is the word's link digit (below); words of one gadget share the rest of
# their prefix, so their prefixes differ in one digit. Inside a word, codes that differ
# only in the last digit are adjacent; the "other" suffixes differ from every majority
# suffix and from each other in >= 2 digits, so each is a cluster of its own (kinds g and
# i excepted, which have no majority / no exception).
_M3 = _sfx("AAA", "AAC", "AAG")
_M6 = _sfx("AAA", "AAC", "AAG", "ACA", "ACC", "ACG")
_C3 = _sfx("CCA", "CCC", "CCG")
_G3 = _sfx("GGA", "GGC", "GGG")
WORDS = {
    "a_uniform": [(0, _M3, [])],
    "b_exc1": [(0, _M3, _sfx("CCA"))],
    "c_exc2": [(0, _M3, _sfx("CCA", "GGC"))],
    "d_exc3": [(0, _M6, _sfx("CAT", "CGC", "CTA"))],
    "d_exc5": [(0, _M6, _sfx("CAT", "CGC", "CTA", "GGA", "GTT"))],
    "e_exc1_bit0": [(0, _C3, _sfx("AAA"))],
    "e_exc1_bit63": [(0, _C3, _sfx("TTT"))],
    "e_exc2_bit0_bit63": [(0, _C3, _sfx("AAA", "TTT"))],
    "f_exc1_lower": [(0, _G3, _sfx("AAC"))],
    "f_exc2_lower": [(0, _G3, _sfx("AAC", "CCA"))],
    "g_none_4": [(0, [], _sfx("AAA", "CCC", "GGG", "TTT"))],
    "g_none_2v2": [(0, [], _sfx("AAA", "AAC", "CCA", "CCC"))],
    # one cluster over two words whose prefixes differ in one digit (p.AAA - p'.AAA)
    "h_span": [(0, _sfx("AAA", "AAC"), _sfx("CCA")), (1, _sfx("AAA", "AAG"), _sfx("GGC"))],
    # p holds AAA and CCC, not adjacent; p' joins them: AAA - CAA - CCA - CCC
    "i_global": [(0, _sfx("AAA", "CCC"), []), (1, _sfx("AAA", "CAA", "CCA", "CCC"), [])],
    "j_single": [(0, _sfx("GAT"), [])],
}
_SET = list(WORDS)
# The boundary block: two clusters, X and Y, each the majority of three linked words of
# kinds b, c and d. X's word of kind b has its exception below the majority and Y's word of
# kind b follows it directly in code order, so X and Y get consecutive ids.
_G6 = _sfx("GGA", "GGC", "GGG", "GTA", "GTC", "GTG")
_BLOCK_X = [("b_exc1", 0, _G3, _sfx("AAA")), ("c_exc2", 1, _G3, _sfx("CCT", "TTA")),
            ("d_exc3", 2, _G6, _sfx("AAC", "CAT", "TCA"))]
_BLOCK_Y = [("b_exc1", 0, _M3, _sfx("CCA")), ("c_exc2", 1, _M3, _sfx("CTG", "TCC")),
            ("d_exc3", 2, _M6, _sfx("GGA", "GTT", "TGT"))]


def _prefix(L: int, link: int, j: int) -> int:
    """Gadget word prefix (the top L-3 digits): T, T, the link digit, then the j-th codeword
    of the parity code on L-6 digits. Prefixes with different j differ in >= 2 digits
    whatever their link digits; with the same j they differ in the link digit alone."""
    if not 0 <= j < 4 ** (L - 7):
        raise ValueError(f"gadget slot {j} outside the {4 ** (L - 7)} of L={L}")
    par = -sum((j >> (2 * i)) & 3 for i in range(L - 7)) & 3
    return ((15 * 4 + link) << (2 * (L - 6))) | (j * 4 + par)


def _distance(a: np.ndarray, b: np.ndarray, L: int) -> np.ndarray:
    """Hamming distance in digits between int64 codes (broadcasting)."""
    x = a ^ b
    d = np.zeros(np.broadcast(a, b).shape, np.int64)
    for i in range(L):
        d += ((x >> (2 * i)) & 3) != 0
    return d


def _components(codes: np.ndarray, L: int) -> np.ndarray:
    """Union-find over the Hamming-1 graph of a few hundred sorted codes: the rank of each
    code's component, components ordered by their smallest code."""
    n = len(codes)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    adj = _distance(codes[:, None], codes[None, :], L) == 1
    for i, k in zip(*np.nonzero(np.triu(adj))):
        a, b = find(int(i)), find(int(k))
        if a != b:
            parent[max(a, b)] = min(a, b)  # the root is the component's smallest code
    roots = np.array([find(i) for i in range(n)])
    return np.searchsorted(np.unique(roots), roots)


class Planted:
    """A planted code set. gadget_codes (ascending int64), gadget_ids (max_distance 1) and
    gadget_exact (max_distance 0) are per gadget code; the fillers come from fillers() with
    ids (both distances) equal to their index. words: one dict per gadget word with kind,
    prefix, codes, majority_label (None for a word without majority) and majority_size."""

    def __init__(self, L, F, sparse, gadget_codes, comp, words):
        self.L, self.F, self.sparse = L, F, sparse
        self.gadget_codes = gadget_codes
        self.gadget_ids = F + comp
        self.gadget_exact = F + np.arange(len(gadget_codes), dtype=np.int64)
        self.n_clusters = F + (int(comp.max()) + 1 if len(comp) else 0)
        self.n_distinct = F + len(gadget_codes)
        self.words = words

    def fillers(self, device=None):
        return fillers(self.L, self.F, self.sparse, device)

    def codes(self) -> np.ndarray:
        """Every distinct code, ascending (host; for small F)."""
        return np.concatenate([self.fillers(), self.gadget_codes])

    def ids(self) -> np.ndarray:
        return np.concatenate([np.arange(self.F, dtype=np.int64), self.gadget_ids])

    def exact_ids(self) -> np.ndarray:
        return np.arange(self.n_distinct, dtype=np.int64)

    def majority_labels(self, letter: str) -> set:
        """Majority labels of the words whose kind starts with `letter` (b, c, d, ...)."""
        return {w["majority_label"] for w in self.words if w["kind"][0] == letter} - {None}

    def on_boundary(self, T: int) -> bool:
        """Both T-1 and T are the majority label of a one-exception word (b), of a
        two-exception word (c) and of a word with more exceptions (d)."""
        return all({T - 1, T} <= self.majority_labels(k) for k in "bcd")


def _layout(L: int):
    """(kind, prefix, majority suffixes, other suffixes) of every gadget word: one set of
    all kinds below the boundary block (link digit 0, partners at 1), the block, one set
    above it (link digit 2, partners at 3)."""
    out = []
    n = len(_SET)
    for base, j0 in ((0, 0), (2, n + 2)):
        for g, kind in enumerate(_SET):
            for link, maj, other in WORDS[kind]:
                out.append((kind, _prefix(L, base + link, j0 + g), maj, other))
    for j, block in ((n, _BLOCK_X), (n + 1, _BLOCK_Y)):
        for kind, link, maj, other in block:
            out.append((kind, _prefix(L, link, j), maj, other))
    return out


def build(L: int, F: int | None = None, T: int | None = None, sparse: bool = False) -> Planted:
    """The planted set at length L (10..16). Give F, the number of fillers, or a threshold T:
    F is then chosen so that the boundary block's two majority clusters get the ids T-1
    and T (Planted.on_boundary(T); the caller asserts it)."""
    if not 10 <= L <= 16:
        raise ValueError("L outside 10..16")
    if (F is None) == (T is None):
        raise ValueError("give exactly one of F and T")
    layout = _layout(L)
    pairs = sorted({(p << 6) | s for _, p, maj, other in layout for s in maj + other})
    gcodes = np.array(pairs, dtype=np.int64)
    comp = _components(gcodes, L)
    # gadget prefixes: pairwise >= 2 digits apart unless linked on purpose (same slot)
    pre = np.array(sorted({p for _, p, _, _ in layout}), dtype=np.int64)
    dist = _distance(pre[:, None], pre[None, :], L - 3)
    slot = pre & (4 ** (L - 6) - 1)
    assert np.all((dist >= 2) | (slot[:, None] == slot[None, :]))
    if T is not None:
        _, p, maj, _ = layout[-6]  # X's word of kind b
        F = T - 1 - int(comp[np.searchsorted(gcodes, (p << 6) | maj[0])])
    words = []
    for kind, p, maj, other in layout:
        at = lambda s: int(comp[np.searchsorted(gcodes, (p << 6) | s)])
        mc = {at(s) for s in maj}
        oc = [at(s) for s in other]
        if kind[0] == "g":  # no majority: no component holds more than half of the codes
            counts = np.bincount(oc)
            assert not maj and counts.max() * 2 <= len(oc), kind
            label, size = None, 0
        else:  # one majority component, every other code in a component of its own
            assert len(mc) == 1 and len(set(oc)) == len(oc) and not (mc & set(oc)), kind
            assert len(maj) > len(other), kind
            label, size = F + mc.pop(), len(maj)
        words.append({"kind": kind, "prefix": p, "codes": np.array([(p << 6) | s for s in sorted(maj + other)]),
                      "majority_label": label, "majority_size": size, "n_other": len(other)})
    return Planted(L, F, sparse, gcodes, comp, words)


def device_rows(pl: Planted, seed: int, device, n_dup: int = 3000):
    """Rows for the device entry points, built with torch on `device`: every planted code
    once, every gadget code once more, about n_dup random duplicates (so many that the row
    count is 3 mod 4: the tails of the 4-row, 256-row and 1024-row loops run), shuffled.
    Returns (codes int32 [n], ids int64 [n], rank int64 [n], is_gadget bool [n]); rank, the
    row's index among the distinct codes, is its id at max_distance 0."""
    import torch

    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    nd, ng = pl.n_distinct, len(pl.gadget_codes)
    distinct = torch.cat([pl.fillers(device), torch.from_numpy(pl.gadget_codes).to(device)])
    ids = torch.cat([torch.arange(pl.F, dtype=torch.int64, device=device), torch.from_numpy(pl.gadget_ids).to(device)])
    n = nd + ng + n_dup
    n += (3 - n) % 4
    extra = torch.randint(0, nd, (n - nd - ng,), generator=gen, device=device)
    rank = torch.cat([torch.arange(nd, device=device), torch.arange(pl.F, nd, device=device), extra])
    rank = rank[torch.randperm(n, generator=gen, device=device)]
    return to_int32(distinct[rank]).contiguous(), ids[rank], rank, rank >= pl.F


def check_separation(pl: Planted, sample: np.ndarray) -> None:
    """Brute force on a sample of fillers: pairwise >= 2 digits apart, and >= 2 digits from
    every gadget code."""
    L = pl.L
    d = _distance(sample[:, None], sample[None, :], L)
    np.fill_diagonal(d, L)
    assert d.min() >= 2
    assert _distance(sample[:, None], pl.gadget_codes[None, :], L).min() >= 2
