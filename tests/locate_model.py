"""Brute-force model of rse_locate_flat's per-column definition, for the tests.

A byte column of a k+p stripe is *decodable* when exactly one codeword lies
within Hamming distance t = p // 2 of it (unique because the code's minimum
distance is p + 1 > 2t); its bad shards are where it differs from that
codeword.  Stated without any decoding algorithm: with the check matrix
Hc = [P | I] taken from the ORACLE's encoding matrix (Hc c = P data ^ parity),
a column c is within distance |A| of a codeword differing exactly inside A iff
Hc c lies in the span of the columns A of Hc.  The model tries every position
set of size 0 .. t in ascending size and tests that by rank; no
Berlekamp-Massey, no syndromes of the library's form.
"""
import itertools

import numpy as np

from oracle import oracle as O

CLEAN, LOCATED, UNCORRECTABLE = 0, 1, 2

_MUL = None
_INV = None


def _tables():
    global _MUL, _INV
    if _MUL is None:
        _MUL = O.gf8_tables()[2].astype(np.uint8)
        _INV = np.zeros(256, np.uint8)
        for a in range(1, 256):
            _INV[a] = int(np.nonzero(_MUL[a] == 1)[0][0])
    return _MUL, _INV


def gf_matvec(m, v):
    """m (r x c) times v (c) or (c x cols), over GF(2^8)."""
    mul, _ = _tables()
    m = np.asarray(m, np.uint8)
    v = np.asarray(v, np.uint8)
    if v.ndim == 1:
        return np.bitwise_xor.reduce(mul[m, v[None, :]], axis=1)
    out = np.zeros((m.shape[0], v.shape[1]), np.uint8)
    for i in range(m.shape[1]):
        out ^= mul[m[:, i][:, None], v[i][None, :]]
    return out


def check_matrix(k, p):
    """Hc = [P | I] from the oracle's matrix."""
    m = O.Codec(8, k, p).matrix()
    return np.concatenate([m[k:], np.eye(p, dtype=np.uint8)], axis=1)


def _rank(rows):
    mul, inv = _tables()
    a = [list(map(int, r)) for r in rows]
    rank = 0
    ncol = len(a[0]) if a else 0
    for c in range(ncol):
        piv = next((r for r in range(rank, len(a)) if a[r][c]), None)
        if piv is None:
            continue
        a[rank], a[piv] = a[piv], a[rank]
        s = int(inv[a[rank][c]])
        a[rank] = [int(mul[s, x]) for x in a[rank]]
        for r in range(len(a)):
            if r != rank and a[r][c]:
                f = a[r][c]
                a[r] = [x ^ int(mul[f, y]) for x, y in zip(a[r], a[rank])]
        rank += 1
    return rank


def column_bad_shards(hc, d, t):
    """The bad shards of a column whose check vector is d = Hc c: a sorted
    tuple (empty: clean), or None when the column is undecodable."""
    d = [int(x) for x in d]
    if not any(d):
        return ()
    n = hc.shape[1]
    for size in range(1, t + 1):
        for pos in itertools.combinations(range(n), size):
            # columns as rows: d in span(Hc[:, pos]) iff appending it keeps the rank
            rows = [hc[:, q] for q in pos]
            if _rank(rows + [d]) == size:
                return pos
    return None


def stripe_verdict(k, p, shards):
    """(status, present) of one stripe given as (k+p) x shard_len bytes."""
    hc = check_matrix(k, p)
    shards = np.asarray(shards, np.uint8)
    d = gf_matvec(hc, shards)  # p x shard_len
    n, t = k + p, p // 2
    union = set()
    seen = {}
    for col in np.nonzero(d.any(axis=0))[0]:
        key = d[:, col].tobytes()
        if key not in seen:
            seen[key] = column_bad_shards(hc, d[:, col], t)
        bad = seen[key]
        if bad is None:
            return UNCORRECTABLE, np.ones(n, np.uint8)
        union.update(bad)
    if len(union) > p:
        return UNCORRECTABLE, np.ones(n, np.uint8)
    present = np.ones(n, np.uint8)
    present[sorted(union)] = 0
    return (LOCATED if union else CLEAN), present
