"""Brute-force model of rse_correct_flat's per-column definition, for the tests.

With the erased shards E (|E| = f) a byte column c of a k+p stripe is
*decodable* when some codeword differs from it in nu positions outside E (and
anywhere inside E) with 2 nu + f <= p; that codeword is unique because the
code's minimum distance is p + 1.  Stated without any decoding algorithm, as
tests/locate_model.py does: with Hc = [P | I] from the ORACLE's encoding matrix
and d = Hc c, such a codeword exists iff d lies in the span of the columns
E u B of Hc for some set B of nu positions outside E, and the error vector is
the solution of that linear system.  The model tries every B for
nu = 0 .. (p - f) // 2 and solves by Gaussian elimination; no syndromes, no
Berlekamp-Massey, no Forney.
"""
import itertools

import numpy as np

from locate_model import _tables, check_matrix, gf_matvec  # noqa: F401

CLEAN, CORRECTED, UNCORRECTABLE = 0, 1, 2


def _solve(cols, d, mul, inv):
    """x with sum_i x[i] cols[i] = d over GF(2^8), or None; the columns are
    independent whenever there are at most p of them (any p columns of Hc are)."""
    m, rows = len(cols), len(d)
    a = [[cols[j][i] for j in range(m)] + [d[i]] for i in range(rows)]
    rank = 0
    for c in range(m):
        piv = next((r for r in range(rank, rows) if a[r][c]), None)
        if piv is None:
            return None  # dependent columns: not a set the definition allows
        a[rank], a[piv] = a[piv], a[rank]
        s = inv[a[rank][c]]
        a[rank] = [mul[s][x] for x in a[rank]]
        for r in range(rows):
            if r != rank and a[r][c]:
                g = mul[a[r][c]]
                a[r] = [x ^ g[y] for x, y in zip(a[r], a[rank])]
        rank += 1
    if any(a[r][m] for r in range(rank, rows)):
        return None  # d is not in the span
    return [a[i][m] for i in range(m)]


def correct_column(hc, col, erased, p):
    """The corrected column (a list of n bytes), or None when it is undecodable.
    hc: check_matrix(k, p); col: n bytes; erased: shard indices."""
    mul_np, inv_np = _tables()
    mul = _py_tables(mul_np)
    inv = [int(x) for x in inv_np]
    n = hc.shape[1]
    col = [int(x) for x in col]
    erased = sorted(set(int(q) for q in erased))
    f = len(erased)
    if f > p:
        return None
    d = [int(x) for x in gf_matvec(hc, np.array(col, np.uint8))]
    hcols = _py_cols(hc)
    rest = [q for q in range(n) if q not in erased]
    for nu in range(0, (p - f) // 2 + 1):
        for extra in itertools.combinations(rest, nu):
            where = erased + list(extra)
            x = _solve([hcols[q] for q in where], d, mul, inv)
            if x is not None:
                out = list(col)
                for q, e in zip(where, x):
                    out[q] ^= e
                return out
    return None


_PY = {}


def _py_tables(mul_np):
    if "mul" not in _PY:
        _PY["mul"] = [[int(x) for x in row] for row in mul_np]
    return _PY["mul"]


def _py_cols(hc):
    key = (hc.shape, hc.tobytes())
    if key not in _PY:
        _PY[key] = [[int(x) for x in hc[:, q]] for q in range(hc.shape[1])]
    return _PY[key]


def correct_stripe(k, p, shards, erased):
    """(status, corrected shards, undecodable columns) of one stripe given as
    (k+p) x shard_len bytes; undecodable columns are left as they were."""
    hc = check_matrix(k, p)
    shards = np.array(shards, np.uint8)
    if len(set(erased)) > p:
        return UNCORRECTABLE, shards, 0
    d = gf_matvec(hc, shards)
    out = shards.copy()
    bad = 0
    for c in np.nonzero(d.any(axis=0))[0]:
        fixed = correct_column(hc, shards[:, c], erased, p)
        if fixed is None:
            bad += 1
        else:
            out[:, c] = fixed
    if bad:
        return UNCORRECTABLE, out, bad
    return (CORRECTED if (out != shards).any() else CLEAN), out, 0
