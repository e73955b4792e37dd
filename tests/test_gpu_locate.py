"""rse_locate_flat on the GPU: which shards of a stripe are wrong.

Expected flags come from the injection itself (at most t = p // 2 wrong shards
in a column are located exactly: the code's minimum distance is p + 1) and,
past t, from the brute-force model of tests/locate_model.py (position sets and
ranks over the ORACLE's matrix; no Berlekamp-Massey).  Expected repaired bytes
are the oracle's encode.  The library is never compared with itself.

Every batch is 5 stripes followed by a guard stripe that must stay
byte-identical (the call only reads: so must the batch); present and status
are allocated with one spare row past the batch, filled with 0xA5, which must
keep it.  Shard lengths: 1, 15, 17 and 4096 + 37 (byte-wise path: the shards
of a flat stripe of odd length start at odd addresses), 4096 (16-byte
vectors, whole spans) and 4096 + 16 (a partly filled span); 65537 for 10+4.
20+8, 6+9, 30+15, 128+16 and 129+16 run at 17 and 4096 + 16 only.
"""

import numpy as np
import pytest
import torch

import reed_solomon_erasure as R
from oracle import oracle as O
from reed_solomon_erasure._lib import load

import locate_model as LM

pytestmark = pytest.mark.gpu

LIB = load()
CODECS = [(10, 4), (3, 2), (4, 5), (17, 3), (1, 1), (100, 16), (239, 16)]
LENGTHS = [1, 15, 17, 4096, 4096 + 16, 4096 + 37]
# parity counts 8, 9 and 15, and k on both sides of one chunk of the kernels'
# tables at p = 16: a byte-wise and a vector length each
WIDE_CODECS = [(20, 8), (6, 9), (30, 15), (128, 16), (129, 16)]
WIDE_LENGTHS = [17, 4096 + 16]
CASES = [(k, p, n) for k, p in CODECS for n in LENGTHS] + [(10, 4, 65537)] + \
        [(k, p, n) for k, p in WIDE_CODECS for n in WIDE_LENGTHS]
NS = 5
CLEAN, LOCATED, UNCORRECTABLE = 0, 1, 2

_REF = {}


def reference(k, p, length):
    """NS clean stripes and a guard stripe, (NS + 1, k + p, length) bytes: random
    data with the ORACLE's parity.  Computed once per shape; never modified."""
    key = (k, p, length)
    if key not in _REF:
        rng = np.random.default_rng(1000 * k + 10 * p + length)
        buf = rng.integers(0, 256, (NS + 1, k + p, length), dtype=np.uint8)
        codec = O.Codec(8, k, p)
        for s in range(NS):
            codec.encode([buf[s, i] for i in range(k + p)])
        buf.setflags(write=False)
        _REF[key] = buf
    return _REF[key]


def corrupt_shards(buf, rng, stripe, shards, cols=None):
    """XOR a nonzero value into every byte (or the bytes `cols`) of the shards."""
    length = buf.shape[2]
    for q in shards:
        if cols is None:
            buf[stripe, q] ^= rng.integers(1, 256, length, dtype=np.uint8)
        else:
            for c in cols:
                buf[stripe, q, c] ^= np.uint8(rng.integers(1, 256))


def locate(r, host, length, n_stripes=NS):
    """rse_locate_flat through the C entry on a copy of `host` (n_stripes + 1
    stripes) in HBM; returns (present, status) of the batch after checking
    what must not have been written."""
    n = r.total_shard_count()
    dev = torch.from_numpy(np.array(host)).cuda()
    present = torch.full((n_stripes + 1, n), 0xA5, dtype=torch.uint8, device="cuda")
    status = torch.full((n_stripes + 1,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = LIB.rse_locate_flat(r._h, dev.data_ptr(), length, n_stripes, present.data_ptr(),
                             status.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert (dev.cpu().numpy() == host).all(), "the call only reads the stripes (and the guard)"
    present, status = present.cpu().numpy(), status.cpu().numpy()
    assert (present[n_stripes] == 0xA5).all() and status[n_stripes] == 0xA5
    return present[:n_stripes], status[:n_stripes]


def expect(present, status, want):
    """want: per stripe None (clean), a set of shards (located) or 'bad'."""
    n = present.shape[1]
    for s, w in enumerate(want):
        flags = np.ones(n, np.uint8)
        if w is None:
            code = CLEAN
        elif isinstance(w, str):
            code = UNCORRECTABLE
        else:
            code = LOCATED
            flags[sorted(w)] = 0
        assert status[s] == code, (s, int(status[s]), w)
        assert (present[s] == flags).all(), (s, present[s].tolist(), w)


@pytest.mark.parametrize("k,p,length", CASES)
def test_all_clean(k, p, length):
    r = R.galois_8.ReedSolomon(k, p)
    present, status = locate(r, reference(k, p, length), length)
    expect(present, status, [None] * NS)


@pytest.mark.parametrize("k,p,length", CASES)
def test_whole_shard_corruption(k, p, length):
    n, t = k + p, p // 2
    rng = np.random.default_rng(7)
    buf = reference(k, p, length).copy()
    want = [None] * NS
    if t == 0:  # 1+1: nothing can be located, any corruption is uncorrectable
        corrupt_shards(buf, rng, 0, [0])
        corrupt_shards(buf, rng, 2, [1])
        want[0] = want[2] = "bad"
    else:
        want[0] = {min(1, n - 1)}
        many = {0, n - 1} if t >= 2 else {n - 1}
        while len(many) < t:
            many.add(int(rng.integers(1, n - 1)))
        want[1] = many
        want[2] = set(range(k, k + t))  # parity shards only
        for s in range(3):
            corrupt_shards(buf, rng, s, sorted(want[s]))
    present, status = locate(R.galois_8.ReedSolomon(k, p), buf, length)
    expect(present, status, want)


@pytest.mark.parametrize("k,p,length", [c for c in CASES if c[1] >= 2])
def test_single_wrong_bytes(k, p, length):
    n = k + p
    rng = np.random.default_rng(11)
    buf = reference(k, p, length).copy()
    tail = (length // 16) * 16 if length % 16 else length - 1  # first byte of a ragged tail
    a, b, c = 0, n - 1, k // 2
    corrupt_shards(buf, rng, 0, [a], cols=[0])
    corrupt_shards(buf, rng, 1, [b], cols=[length - 1])
    corrupt_shards(buf, rng, 2, [c], cols=[min(tail, length - 1)])
    # all three at once, each in its own column where the shard is long enough
    cols = sorted({0, length - 1, min(tail, length - 1)})
    want3 = set()
    for q, col in zip((a, b, c), cols if len(cols) == 3 else cols[:1]):
        corrupt_shards(buf, rng, 3, [q], cols=[col])
        want3.add(q)
    present, status = locate(R.galois_8.ReedSolomon(k, p), buf, length)
    expect(present, status, [{a}, {b}, {c}, want3 if len(want3) <= p else "bad", None])


def disjoint_columns(k, p, length, rng, size):
    """`size` shards split into sets of at most t, one byte column each."""
    n, t = k + p, p // 2
    shards = [int(q) for q in rng.permutation(n)[:size]]
    sets = [shards[i:i + t] for i in range(0, size, t)]
    cols = np.linspace(0, length - 1, len(sets)).astype(int).tolist()
    assert len(set(cols)) == len(sets)
    return sets, cols


@pytest.mark.parametrize("k,p,length", [c for c in CASES if c[1] >= 2 and c[2] >= 15])
def test_disjoint_sets_in_different_columns(k, p, length):
    rng = np.random.default_rng(13)
    buf = reference(k, p, length).copy()
    sets, cols = disjoint_columns(k, p, length, rng, p)
    assert len(sets) == 2 or p % 2  # even p: exactly two columns of t each
    for shards, col in zip(sets, cols):
        corrupt_shards(buf, rng, 1, shards, cols=[col])
    want = [None, set(sum(sets, [])), None, None, None]
    assert len(want[1]) == p
    if (k, p) in ((10, 4), (100, 16)):  # p + 1 shards implicated: more than can be rebuilt
        sets, cols = disjoint_columns(k, p, length, rng, p + 1)
        for shards, col in zip(sets, cols):
            corrupt_shards(buf, rng, 3, shards, cols=[col])
        want[3] = "bad"
    present, status = locate(R.galois_8.ReedSolomon(k, p), buf, length)
    expect(present, status, want)


# t + 1 wrong shards in EVERY column: each column is undecodable or lies within
# t of another codeword, never located right.  Seeds fixed on the CPU so that
# the model's verdict for the stripe is UNCORRECTABLE.
@pytest.mark.parametrize("k,p,length,seed", [(3, 2, 17, 1), (10, 4, 17, 1), (10, 4, 4096 + 16, 1)])
def test_one_more_than_t_wrong_shards_in_every_column(k, p, length, seed):
    n, t = k + p, p // 2
    rng = np.random.default_rng(seed)
    buf = reference(k, p, length).copy()
    shards = [int(q) for q in rng.permutation(n)[:t + 1]]
    corrupt_shards(buf, rng, 2, shards)
    model = min(length, 64)  # the model walks the first columns; the rest only add to them
    code, flags = LM.stripe_verdict(k, p, buf[2][:, :model])
    assert code == UNCORRECTABLE and flags.all()
    present, status = locate(R.galois_8.ReedSolomon(k, p), buf, length)
    assert status[2] != CLEAN
    expect(present, status, [None, None, "bad", None, None])


@pytest.mark.parametrize("length", LENGTHS)
def test_one_plus_one_locates_nothing(length):
    rng = np.random.default_rng(17)
    buf = reference(1, 1, length).copy()
    corrupt_shards(buf, rng, 1, [0], cols=[length - 1])
    corrupt_shards(buf, rng, 4, [1], cols=[0])
    present, status = locate(R.galois_8.ReedSolomon(1, 1), buf, length)
    expect(present, status, [None, "bad", None, None, "bad"])


@pytest.mark.parametrize("k,p", [(10, 4), (100, 16)])
def test_round_trip_locate_reconstruct_verify(k, p):
    length = 4096 + 37
    n, t = k + p, p // 2
    rng = np.random.default_rng(19)
    clean = reference(k, p, length)
    r = R.galois_8.ReedSolomon(k, p)

    # encode_flat of the data equals the oracle's encode
    dev = torch.from_numpy(clean.copy()).cuda()
    dev[:NS, k:] = 0
    r.encode_flat(dev, length, NS)
    torch.cuda.synchronize()
    assert (dev.cpu().numpy() == clean).all()

    buf = clean.copy()
    corrupt_shards(buf, rng, 1, [3])
    corrupt_shards(buf, rng, 2, [0, n - 1] + list(range(k - t + 2, k)))
    sets, cols = disjoint_columns(k, p, length, rng, p)
    for shards, col in zip(sets, cols):
        corrupt_shards(buf, rng, 3, shards, cols=[col])
    sets, cols = disjoint_columns(k, p, length, rng, p + 1)
    for shards, col in zip(sets, cols):
        corrupt_shards(buf, rng, 4, shards, cols=[col])

    dev = torch.from_numpy(buf).cuda()
    present, status = r.locate_flat(dev, length, NS)
    assert present.is_cuda and present.dtype == torch.uint8 and tuple(present.shape) == (NS, n)
    assert status.is_cuda and status.dtype == torch.uint8 and tuple(status.shape) == (NS,)
    r.reconstruct_batch(dev, length, NS, present)  # the device tensor, unchanged
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [CLEAN, LOCATED, LOCATED, LOCATED, UNCORRECTABLE]
    assert (present.cpu().numpy().sum(axis=1) == [n, n - 1, n - t, n - p, n]).all()
    got = dev.cpu().numpy()
    assert (got[:4] == clean[:4]).all(), "repaired stripes equal the oracle's encode"
    assert (got[4] == buf[4]).all(), "an uncorrectable stripe is left as it was"
    assert (got[NS] == clean[NS]).all(), "guard stripe"
    assert r.verify_flat(dev, length, NS).tolist() == [True, True, True, True, False]


def test_non_default_stream_and_last_kernel():
    k, p, length = 10, 4, 4096
    rng = np.random.default_rng(23)
    buf = reference(k, p, length).copy()
    corrupt_shards(buf, rng, 3, [5, 12])
    r = R.galois_8.ReedSolomon(k, p)
    dev = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        present, status = r.locate_flat(dev, length, NS)
    stream.synchronize()
    assert R.core.last_kernel().startswith("locate gf8")
    assert R.core.last_kernel() == "locate gf8 10+4"
    expect(present.cpu().numpy(), status.cpu().numpy(), [None, None, None, {5, 12}, None])


def test_out_of_scope_codecs_raise():
    buf = torch.zeros(256 * 16 * 2, dtype=torch.uint8, device="cuda")
    for r in (R.galois_16.ReedSolomon(10, 4), R.galois_8.ReedSolomon(10, 17),
              R.galois_8.ReedSolomon(200, 56)):
        with pytest.raises(R.DeviceError):
            r.locate_flat(buf, 16, 1)
    with pytest.raises(R.RSError):
        R.galois_8.ReedSolomon(10, 4).locate_flat(buf, 0, 1)
    present, status = R.galois_8.ReedSolomon(10, 4).locate_flat(buf, 16, 0)
    assert tuple(present.shape) == (0, 14) and tuple(status.shape) == (0,)
