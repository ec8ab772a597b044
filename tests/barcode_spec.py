"""Cell-barcode correction against a whitelist restated twice in plain Python,
independently of each other and of the library:

  (a) ``correct_dict``   generates the neighbour strings of each row and looks them up in a dict;
  (b) ``correct_brute``  compares each row against every whitelist entry, position by position.

Both return a ``Result``; ``KNOWN_*`` is the hand-derived known answer of the section.
Rows and whitelist entries are ``bytes`` (a row may be ``None``).
"""
from collections import namedtuple

EXACT, CORRECTED, AMBIGUOUS, NO_MATCH, NULL = 0, 1, 2, 3, 4
NO_INDEX = 0xFFFFFFFF
BASES = b"ACGT"

Result = namedtuple("Result", "index status corrected exact_counts counts totals")


def _b(x):
    return None if x is None else (x.encode() if isinstance(x, str) else bytes(x))


def _resolve(cands, prior, ambiguous):
    """(status, index) of a non-exact row with candidate entries `cands`."""
    cands = sorted(set(cands))
    if not cands:
        return NO_MATCH, NO_INDEX
    if len(cands) == 1:
        return CORRECTED, cands[0]
    if ambiguous == "reject":
        return AMBIGUOUS, NO_INDEX
    top = max(prior[w] for w in cands)
    best = [w for w in cands if prior[w] == top]
    return (CORRECTED, best[0]) if len(best) == 1 else (AMBIGUOUS, NO_INDEX)


def _finish(rows, whitelist, found, exact_counts, ambiguous, counts):
    """found[i]: None (null row), ("exact", w) or ("cands", [w...])."""
    assert ambiguous in ("counts", "reject")
    prior = list(counts) if counts is not None else exact_counts
    assert len(prior) == len(whitelist)
    index, status, corrected = [], [], []
    final = list(exact_counts)
    totals = [0] * 5
    for f in found:
        if f is None:
            st, w = NULL, NO_INDEX
        elif f[0] == "exact":
            st, w = EXACT, f[1]
        else:
            st, w = _resolve(f[1], prior, ambiguous)
            if st == CORRECTED:
                final[w] += 1
        index.append(w)
        status.append(st)
        corrected.append(whitelist[w] if st <= CORRECTED else None)
        totals[st] += 1
    return Result(index, status, corrected, list(exact_counts), final, totals)


def correct_dict(rows, whitelist, ambiguous="counts", counts=None):
    """(a): neighbour strings looked up in a dict."""
    rows = [_b(r) for r in rows]
    whitelist = [_b(w) for w in whitelist]
    L = len(whitelist[0])
    where = {w: k for k, w in enumerate(whitelist)}
    exact_counts = [0] * len(whitelist)
    found = []
    for r in rows:
        if r is None:
            found.append(None)
            continue
        unknown = [j for j, ch in enumerate(r) if ch not in BASES]
        if len(r) != L or len(unknown) >= 2:
            found.append(("cands", []))
        elif not unknown and r in where:
            exact_counts[where[r]] += 1
            found.append(("exact", where[r]))
        else:
            places = unknown if unknown else range(L)
            cands = []
            for j in places:
                for b in BASES:
                    if b == r[j]:
                        continue
                    q = r[:j] + bytes([b]) + r[j + 1:]
                    if q in where:
                        cands.append(where[q])
            found.append(("cands", cands))
    return _finish(rows, whitelist, found, exact_counts, ambiguous, counts)


def correct_brute(rows, whitelist, ambiguous="counts", counts=None):
    """(b): every row against every entry, position by position."""
    rows = [_b(r) for r in rows]
    whitelist = [_b(w) for w in whitelist]
    L = len(whitelist[0])
    exact_counts = [0] * len(whitelist)
    found = []
    for r in rows:
        if r is None:
            found.append(None)
            continue
        n_unknown = sum(1 for ch in r if ch not in BASES)
        if len(r) != L or n_unknown >= 2:
            found.append(("cands", []))
            continue
        hit, cands = None, []
        for k, w in enumerate(whitelist):
            known_mismatch = sum(1 for a, b in zip(r, w) if a in BASES and a != b)
            if n_unknown == 0 and known_mismatch == 0:
                hit = k
            elif known_mismatch + n_unknown == 1:
                cands.append(k)
        if hit is not None:
            exact_counts[hit] += 1
            found.append(("exact", hit))
        else:
            found.append(("cands", cands))
    return _finish(rows, whitelist, found, exact_counts, ambiguous, counts)


# ------------------------------------------------------------ the known answer
KNOWN_WHITELIST = [b"ACGT", b"AAAA", b"AAAT", b"TTTT", b"CCCC", b"CCCG", b"GGGG"]
KNOWN_ROWS = ([b"ACGT"] * 3 + [b"AAAA"] * 5 + [b"AAAT"] * 2 +
              [b"AAAC", b"ACGA", b"TTTN", b"AAAN", b"NCGN", b"GGCC", b"ACG", b"acgt", b"ACGt", b"CCCA", None])
_X = NO_INDEX
KNOWN_EXACT_COUNTS = [3, 5, 2, 0, 0, 0, 0]
#                      ACGTx3   AAAAx5         AAATx2 AAAC ACGA TTTN AAAN NCGN GGCC ACG acgt ACGt CCCA null
KNOWN_INDEX_COUNTS = [0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 1, 0, 3, 1, _X, _X, _X, _X, 0, _X, _X]
KNOWN_STATUS_COUNTS = [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 3, 3, 3, 3, 1, 2, 4]
KNOWN_TOTALS_COUNTS = [10, 5, 1, 4, 1]
KNOWN_COUNTS_COUNTS = [5, 7, 2, 1, 0, 0, 0]
KNOWN_INDEX_REJECT = [0, 0, 0, 1, 1, 1, 1, 1, 2, 2, _X, 0, 3, _X, _X, _X, _X, _X, 0, _X, _X]
KNOWN_STATUS_REJECT = [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 1, 1, 2, 3, 3, 3, 3, 1, 2, 4]
KNOWN_TOTALS_REJECT = [10, 3, 3, 4, 1]
KNOWN_COUNTS_REJECT = [5, 5, 2, 1, 0, 0, 0]
# with the caller's counts: CCCA -> 5; AAAC and AAAN tie 0 against 0
KNOWN_CALLER_COUNTS = [0, 0, 0, 0, 1, 4, 0]
KNOWN_INDEX_CALLER = [0, 0, 0, 1, 1, 1, 1, 1, 2, 2, _X, 0, 3, _X, _X, _X, _X, _X, 0, 5, _X]
KNOWN_STATUS_CALLER = [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 1, 1, 2, 3, 3, 3, 3, 1, 1, 4]
KNOWN_TOTALS_CALLER = [10, 4, 2, 4, 1]
KNOWN_COUNTS_CALLER = [5, 5, 2, 1, 0, 1, 0]

KNOWN = {
    ("counts", None): (KNOWN_INDEX_COUNTS, KNOWN_STATUS_COUNTS, KNOWN_TOTALS_COUNTS, KNOWN_COUNTS_COUNTS),
    ("reject", None): (KNOWN_INDEX_REJECT, KNOWN_STATUS_REJECT, KNOWN_TOTALS_REJECT, KNOWN_COUNTS_REJECT),
    ("counts", "caller"): (KNOWN_INDEX_CALLER, KNOWN_STATUS_CALLER, KNOWN_TOTALS_CALLER, KNOWN_COUNTS_CALLER),
}


def random_case(rng, L=None, W=None, n=None):
    """A seeded small case (numpy Generator): a whitelist of W distinct barcodes of length L and
    rows drawn from it, mutated, with N / lower case / wrong lengths / nulls mixed in."""
    L = int(rng.integers(1, 7)) if L is None else L
    W = int(rng.integers(1, 41)) if W is None else W
    W = min(W, 4 ** L)
    codes = rng.choice(4 ** L, size=W, replace=False)
    wl = [bytes(BASES[(int(c) >> (2 * (L - 1 - j))) & 3] for j in range(L)) for c in codes]
    n = int(rng.integers(0, 60)) if n is None else n
    rows = []
    for _ in range(n):
        k = int(rng.integers(0, 10))
        r = bytearray(wl[int(rng.integers(0, W))])
        if k == 0:
            rows.append(None)
            continue
        if k in (1, 2, 3):  # one substitution
            j = int(rng.integers(0, L))
            r[j] = BASES[int(rng.integers(0, 4))]
        elif k == 4:  # one or two unknown positions
            for _ in range(int(rng.integers(1, 3))):
                r[int(rng.integers(0, L))] = b"Nacgt"[int(rng.integers(0, 5))]
        elif k == 5:  # another length (the empty string included)
            r = r[:-1] if rng.integers(0, 2) else r + b"A"
        elif k == 6:  # random
            r = bytearray(BASES[int(x)] for x in rng.integers(0, 4, size=L))
        rows.append(bytes(r))
    return rows, wl
