"""rse_correct_flat and rse_locate_flat with every byte column different, at
parity counts between the ones tests/test_gpu_locate.py started with.

Neighbouring columns -- the 16 of one lane, the 64 lanes of one wave -- draw
their own number of wrong shards, their own positions and values, so the
rolled column loop of the slow path, the selects that pick a column out of the
accumulators and Berlekamp-Massey runs of different lengths all meet in one
wave.  Codecs: p = 6 and 8 (NO = 8 of the kernels partly and fully used),
9, 12, 15 (NO = 16 partly filled), 16 with k = 128 (one chunk of tables) and
k = 129 (MULTI, a last chunk of one input), and 10+4 and 239+16 from the
existing list.  Lengths: 17 (byte-wise) and 4096 + 16 (16-byte vectors, a
partly filled second span).

Expected bytes are the clean stripes -- random data with the ORACLE's parity
(tests/test_gpu_locate.py reference()) -- wherever a column stays within
2 nu + f <= p; flags and counts follow from before -> clean.  Past capacity
the header's definition is checked column by column with the oracle's check
matrix: a column of the output is either byte-identical to the input and still
not a codeword, or a codeword that differs from the input in at most
(p - f) // 2 positions outside the erased set.  The library is never compared
with itself.  Batches are 5 stripes and a guard stripe; outputs carry one
spare row of 0xA5.

Untested: saturation of counts at 2^32 - 1.  It needs more than 4 GiB of wrong
bytes in one stripe.
"""

import numpy as np
import pytest
import torch

import reed_solomon_erasure as R

import locate_model as LM
from test_gpu_correct import correct, expect
from test_gpu_locate import NS, locate, reference
from test_gpu_locate import expect as expect_located

pytestmark = pytest.mark.gpu

CLEAN, CORRECTED, UNCORRECTABLE = 0, 1, 2
CODECS = [(11, 6), (20, 8), (6, 9), (12, 12), (30, 15), (128, 16), (129, 16), (10, 4), (239, 16)]
LENGTHS = [17, 4096 + 16]
CASES = [(k, p, n) for k, p in CODECS for n in LENGTHS]


def dense_errors(rng, buf, stripe, shards, nu, forced=0):
    """XOR a nonzero value into nu[c] shards of byte column c, drawn from
    `shards` independently per column.  forced: column j < forced has at least
    one wrong shard and shards[j] is among them.  Returns the hit mask,
    len(shards) x length."""
    shards = np.asarray(shards)
    m, length = len(shards), buf.shape[2]
    nu = np.array(nu)
    order = rng.random((m, length)).argsort(axis=0)  # a permutation per column
    for j in range(forced):
        i = int(np.nonzero(order[:, j] == j)[0][0])
        order[[0, i], j] = order[[i, 0], j]
        nu[j] = max(nu[j], 1)
    hit = np.zeros((m, length), bool)
    rows = np.arange(m)[:, None]
    hit[order, np.arange(length)[None, :]] = rows < nu[None, :]
    assert (hit.sum(axis=0) == nu).all()
    buf[stripe, shards] ^= rng.integers(1, 256, (m, length), dtype=np.uint8) * hit
    return hit


@pytest.mark.parametrize("k,p,length", CASES)
def test_correct_every_column_different(k, p, length):
    """Stripe s has f erased shards, f = 0, 1, p - 2, p, 3 (filled with 0xEE
    in stripes 1 and 3, with random bytes in the others); every column draws
    nu in 0 .. (p - f) // 2 and nu shards outside the erased set."""
    n = k + p
    rng = np.random.default_rng(1000 * k + p + length)
    ref = reference(k, p, length)
    buf = ref.copy()
    present = np.ones((NS, n), np.uint8)
    stored = []
    for s, f in enumerate((0, 1, p - 2, p, 3)):
        perm = rng.permutation(n)
        era, rest = perm[:f], perm[f:]
        if f >= 2:  # both ends of the point shift among the erasures
            era = np.array([0, n - 1] + [q for q in perm if q not in (0, n - 1)][:f - 2])
            rest = np.array([q for q in perm if q not in era])
        fill = np.full((f, length), 0xEE, np.uint8) if s in (1, 3) else \
            rng.integers(0, 256, (f, length), dtype=np.uint8)
        buf[s, era] = fill
        present[s, era] = 0
        cap = (p - f) // 2
        hit = dense_errors(rng, buf, s, rest, rng.integers(0, cap + 1, length))
        stored.append(int(hit.sum()) + int((fill != ref[s, era]).sum()))
    result = correct(R.galois_8.ReedSolomon(k, p), buf, length, present)
    expect(buf, result, ref[:NS])
    assert result[3][:, 0].tolist() == stored


@pytest.mark.parametrize("k,p,length", CASES)
def test_locate_every_column_different(k, p, length):
    """Per stripe a set U of shards, |U| = t, p, p, p + 1 (stripe 4 is clean);
    every column has at most t wrong shards out of U, every member of U is
    wrong in some column.  Then reconstruct_batch with the device's flags."""
    n, t = k + p, p // 2
    rng = np.random.default_rng(2000 * k + p + length)
    ref = reference(k, p, length)
    buf = ref.copy()
    sets = []
    for s, size in enumerate((t, p, p, p + 1)):
        u = rng.permutation(n)[:size]
        if s == 1:
            u = np.array([0, n - 1] + [q for q in u if q not in (0, n - 1)][:size - 2])
        dense_errors(rng, buf, s, u, rng.integers(0, t + 1, length), forced=size)
        assert set(np.nonzero((buf[s] != ref[s]).any(axis=1))[0].tolist()) == set(u.tolist())
        assert (buf[s] != ref[s]).sum(axis=0).max() <= t
        sets.append(set(int(q) for q in u))
    r = R.galois_8.ReedSolomon(k, p)
    present, status = locate(r, buf, length)
    expect_located(present, status, sets[:3] + ["bad", None])

    dev = torch.from_numpy(buf).cuda()
    flags, _ = r.locate_flat(dev, length, NS)
    r.reconstruct_batch(dev, length, NS, flags)  # the device tensor, unchanged
    torch.cuda.synchronize()
    assert (flags.cpu().numpy() == present).all()
    got = dev.cpu().numpy()
    assert (got[:3] == ref[:3]).all(), "located stripes equal the oracle's encode"
    assert (got[3] == buf[3]).all(), "an uncorrectable stripe is left as it was"
    assert (got[4:] == ref[4:]).all(), "clean stripe, guard stripe"


def check_definition(hc, p, before, got, erased, status, changed, counts):
    """One stripe past capacity against the header: every column of the output
    is the input, still no codeword, or a codeword within (p - f) // 2 of the
    input outside the erased set; status, changed and counts follow."""
    n = before.shape[0]
    outside = np.ones(n, bool)
    outside[list(erased)] = False
    diff = before != got
    codeword = ~LM.gf_matvec(hc, got).any(axis=0)
    left = ~diff.any(axis=0) & ~codeword
    decoded = codeword & (diff[outside].sum(axis=0) <= (p - len(erased)) // 2)
    assert (left | decoded).all(), np.nonzero(~(left | decoded))[0][:8].tolist()
    assert counts[1] == left.sum(), (counts.tolist(), int(left.sum()))
    assert counts[0] == diff.sum(), (counts.tolist(), int(diff.sum()))
    assert (changed == diff.any(axis=1)).all()
    assert status == (UNCORRECTABLE if left.any() else CORRECTED if diff.any() else CLEAN)
    return int(left.sum())


@pytest.mark.parametrize("k,p,length", [(k, p, n) for k, p in ((20, 8), (6, 9), (30, 15))
                                        for n in LENGTHS])
def test_one_error_too_many_in_every_column(k, p, length):
    """Stripe 1: no erasure, t + 1 wrong shards in every column.  Stripe 3: one
    erased shard, (p - 1) // 2 + 1 wrong shards in every column."""
    n, t = k + p, p // 2
    rng = np.random.default_rng(3000 * k + p + length)
    ref = reference(k, p, length)
    buf = ref.copy()
    present = np.ones((NS, n), np.uint8)
    dense_errors(rng, buf, 1, np.arange(n), np.full(length, t + 1))
    perm = rng.permutation(n)
    buf[3, perm[0]] = rng.integers(0, 256, length, dtype=np.uint8)
    present[3, perm[0]] = 0
    dense_errors(rng, buf, 3, perm[1:], np.full(length, (p - 1) // 2 + 1))
    r = R.galois_8.ReedSolomon(k, p)
    got, status, changed, counts = correct(r, buf, length, present)
    hc = LM.check_matrix(k, p)
    left = [check_definition(hc, p, buf[s], got[s], era, status[s], changed[s], counts[s])
            for s, era in ((1, []), (3, [int(perm[0])]))]
    # The share of columns within reach of ANOTHER codeword is at most the words
    # within (p - f) // 2 of a codeword over all words with that check vector
    # length: C(28, 4) 255^4 / 256^8 < 5e-6 for 20+8 and less for the others,
    # under 0.03 columns of 4112.  One is allowed; the rest must be left.
    assert min(left) >= length - 1
    for s in (0, 2, 4):
        assert (got[s] == ref[s]).all() and status[s] == CLEAN
        assert not changed[s].any() and not counts[s].any()
    _, located = locate(r, buf, length)
    assert located[1] != CLEAN and located[3] != CLEAN
    assert located[[0, 2, 4]].tolist() == [CLEAN] * 3
