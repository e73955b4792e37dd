"""CPU check of the algebra behind rse_fft16.hip (GF(2^16) codecs past 256
shards with u = 2^m - k <= 32), a pure-Python restatement compared with the
oracle's matrix encode and reconstruct (core.rs:430-436, 481-509, 733-923):

- with c = ifft(values on the k valid points S, zero elsewhere) on the n = 2^m
  points (the Lin-Chung-Han inverse transform of test_fft_math.py, beta = 0,
  GF(2^16) arithmetic) and H[q] = coefficients k .. n-1 of ifft(e_q), the values
  on the other u points U are A_U^-1 c[k .. n-1], A_U = (H[q])_{q in U}: encode
  is S = {0 .. k-1}, reconstruct S = the first k present shards;
- pruning: coefficients n-32 .. n-1 of ifft are the XOR over the n/32 blocks of
  each block's own 5-level transform (twiddles s^_i(32 blk ^ j)).

Test infrastructure; the kernels' own tables are checked by test_fft16_plan.py."""
import functools

import numpy as np
import pytest

from oracle import oracle as O

SHAPES = [(500, 12), (490, 12), (480, 24)]  # u = 12, 22 (padding points), 32
B = 32


@functools.lru_cache(maxsize=None)
def _gf8():
    exp, log = [0] * 512, [0] * 256
    b = 1
    for i in range(255):
        exp[i] = exp[i + 255] = b
        log[b] = i
        b <<= 1
        if b & 0x100:
            b ^= 0x11D  # build.rs:11
    return exp, log


def g8(a, b):
    if not a or not b:
        return 0
    exp, log = _gf8()
    return exp[log[a] + log[b]]


def gmul(a, b):  # GF(2^8)[x] / (x^2 + 2x + 128), element (x coefficient << 8) | constant
    a1, a0, b1, b0 = a >> 8, a & 255, b >> 8, b & 255
    hh = g8(a1, b1)
    return ((g8(a1, b0) ^ g8(a0, b1) ^ g8(2, hh)) << 8) | (g8(a0, b0) ^ g8(128, hh))


def ginv(a):
    r, e, b = 1, 65534, a
    while e:
        if e & 1:
            r = gmul(r, b)
        b = gmul(b, b)
        e >>= 1
    return r


@functools.lru_cache(maxsize=None)
def vanish(i, x):  # s_i(x) = prod over a in span(1, 2, .. 2^(i-1)) of (x + a)
    r = 1
    for a in range(1 << i):
        r = gmul(r, x ^ a)
    return r


@functools.lru_cache(maxsize=None)
def skew(i, x):  # s^_i(x) = s_i(x) / s_i(2^i)
    return gmul(vanish(i, x), ginv(vanish(i, 1 << i)))


def ifft(v, beta=0, levels=None):  # values at beta ^ j -> novel-basis coefficients
    d = list(v)
    n = len(d)
    for i in range(n.bit_length() - 1 if levels is None else levels):
        h = 1 << i
        for j in range(0, n, 2 * h):
            s = skew(i, beta ^ j)
            for t in range(j, j + h):
                d[t + h] ^= d[t]
                d[t] ^= gmul(s, d[t + h])
    return d


def invert(m):
    n = len(m)
    w = [list(r) + [int(i == j) for j in range(n)] for i, r in enumerate(m)]
    for c in range(n):
        piv = next(r for r in range(c, n) if w[r][c])
        w[c], w[piv] = w[piv], w[c]
        s = ginv(w[c][c])
        w[c] = [gmul(s, x) for x in w[c]]
        for r in range(n):
            f = w[r][c]
            if r != c and f:
                w[r] = [x ^ gmul(f, y) for x, y in zip(w[r], w[c])]
    return [r[n:] for r in w]


def size(k, p):
    n = 512
    while n < k + p:
        n *= 2
    return n


@functools.lru_cache(maxsize=None)
def hcols(k, p):
    """H[q]: coefficients k .. n-1 of ifft(e_q).  e_q touches only q's block of
    32, and the levels >= 5 only XOR that block's outputs upwards."""
    n = size(k, p)
    u = n - k
    out = []
    for q in range(n):
        blk = q // B
        e = [0] * B
        e[q % B] = 1
        out.append(ifft(e, B * blk)[B - u:])
    return out


def solve(k, p, valid, vals):
    """The values on the points outside `valid` from the values on it."""
    n = size(k, p)
    u = n - k
    full = [0] * n
    for q, v in zip(valid, vals):
        full[q] = v
    c = ifft(full)[k:]
    other = [q for q in range(n) if q not in set(valid)]
    h = hcols(k, p)
    a = [[h[q][r] for q in other] for r in range(u)]
    ainv = invert(a)
    return {q: functools.reduce(lambda x, y: x ^ y, (gmul(ainv[j][r], c[r]) for r in range(u)))
            for j, q in enumerate(other)}


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"{s[0]}+{s[1]}")
def case(request):
    """One oracle codec per shape, and one encoded stripe of two elements."""
    k, p = request.param
    oc = O.Codec(16, k, p)
    rng = np.random.default_rng(k * 100 + p)
    sh = [rng.integers(0, 256, 4, dtype=np.uint8) for _ in range(k)] + \
         [np.zeros(4, np.uint8) for _ in range(p)]
    oc.encode(sh)
    vals = [[(int(s[2 * e]) << 8) | int(s[2 * e + 1]) for s in sh] for e in range(2)]
    return k, p, oc, sh, vals


def test_h_of_a_point_is_its_blocks_transform():
    k, p = 490, 12
    n = size(k, p)
    for q in (0, 37, 489, 501, 511):
        e = [0] * n
        e[q] = 1
        assert ifft(e)[k:] == hcols(k, p)[q]


def test_encode_is_the_pruned_solve(case):
    k, p, _, _, vals = case
    for col in vals:
        got = solve(k, p, list(range(k)), col[:k])
        assert [got[k + j] for j in range(p)] == col[k:]


def test_pruning_identity(case):
    k, p, _, _, vals = case
    n = size(k, p)
    full = vals[0][:k] + [0] * (n - k)
    acc = [0] * B
    for blk in range(n // B):
        d = ifft(full[B * blk:B * blk + B], B * blk)
        acc = [x ^ y for x, y in zip(acc, d)]
    assert acc == ifft(full)[n - B:]


def patterns(k, p):
    mixed = [1, k // 2, k - 1, k + 0, k + p - 1]
    return {"mixed": mixed, "all-parity": list(range(k, k + p)), "p-data": list(range(5, 5 + p))}


@pytest.mark.parametrize("name", ["mixed", "all-parity", "p-data"])
def test_reconstruct_is_the_pruned_solve(case, name):
    k, p, oc, sh, vals = case
    lost = patterns(k, p)[name]
    valid = [q for q in range(k + p) if q not in lost][:k]
    # the oracle rebuilds the same bytes
    broken = [s.copy() for s in sh]
    for q in lost:
        broken[q][:] = 0
    oc.reconstruct(broken, [q not in lost for q in range(k + p)])
    for q in lost:
        assert (broken[q] == sh[q]).all()
    for col in vals:
        got = solve(k, p, valid, [col[q] for q in valid])
        assert [got[q] for q in lost] == [col[q] for q in lost]
