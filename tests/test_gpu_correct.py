"""rse_correct_flat on the GPU: wrong bytes repaired in place, erasures too.

Expected bytes are the oracle's encode (the clean reference a batch was
corrupted from) wherever the injection is within a column's capacity
2 nu + f <= p, and past it the brute-force model of tests/correct_model.py
(position sets and Gaussian elimination over the ORACLE's matrix; no
syndromes).  The library is never compared with itself.

Shapes and batches are those of tests/test_gpu_locate.py (whose cached clean
stripes are shared): 5 stripes followed by a guard stripe that must stay
byte-identical; status, changed and counts are allocated with one spare row
past the batch, filled with 0xA5, which must keep it.  Erased shards are
filled with 0xEE before the call.
"""

import numpy as np
import pytest
import torch

import reed_solomon_erasure as R
from reed_solomon_erasure._lib import load

import correct_model as CM
from test_gpu_locate import CASES, LENGTHS, NS, corrupt_shards, disjoint_columns, reference

pytestmark = pytest.mark.gpu

LIB = load()
CLEAN, CORRECTED, UNCORRECTABLE = 0, 1, 2
MODEL_COLS = 64


def correct(r, host, length, present=None, n_stripes=NS):
    """rse_correct_flat through the C entry on a copy of `host` (n_stripes + 1
    stripes) in HBM; returns (stripes, status, changed, counts) of the batch
    after checking what must not have been written."""
    n = r.total_shard_count()
    dev = torch.from_numpy(np.array(host)).cuda()
    status = torch.full((n_stripes + 1,), 0xA5, dtype=torch.uint8, device="cuda")
    changed = torch.full((n_stripes + 1, n), 0xA5, dtype=torch.uint8, device="cuda")
    counts = torch.full((n_stripes + 1, 2), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32,
                        device="cuda")
    pres = None
    if present is not None:
        pres = torch.from_numpy(np.ascontiguousarray(present, dtype=np.uint8)).cuda()
        assert tuple(pres.shape) == (n_stripes, n)
    rc = LIB.rse_correct_flat(r._h, dev.data_ptr(), length, n_stripes,
                              pres.data_ptr() if pres is not None else None, status.data_ptr(),
                              changed.data_ptr(), counts.data_ptr(),
                              torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    got = dev.cpu().numpy()
    assert (got[n_stripes] == host[n_stripes]).all(), "guard stripe"
    status, changed = status.cpu().numpy(), changed.cpu().numpy()
    counts = counts.cpu().numpy().view(np.uint32)
    assert status[n_stripes] == 0xA5 and (changed[n_stripes] == 0xA5).all()
    assert (counts[n_stripes] == 0xA5A5A5A5).all()
    if pres is not None:
        assert (pres.cpu().numpy() == np.asarray(present, np.uint8)).all(), "present is only read"
    return got[:n_stripes], status[:n_stripes], changed[:n_stripes], counts[:n_stripes]


def expect(before, result, want, undecodable=None):
    """Every stripe of the batch against `want` (the bytes it must hold now):
    the bytes, the changed flags and the stored-byte count follow from
    before -> want; the status from those and from `undecodable` (per stripe,
    a minimum of columns left as they were; None: none anywhere)."""
    got, status, changed, counts = result
    for s in range(len(want)):
        bad = undecodable[s] if undecodable else 0
        diff = before[s] != want[s]
        assert (got[s] == want[s]).all(), (s, np.argwhere(got[s] != want[s])[:4].tolist())
        assert (changed[s] == diff.any(axis=1)).all(), (s, changed[s].tolist())
        assert counts[s][0] == diff.sum(), (s, counts[s].tolist(), int(diff.sum()))
        if bad:
            assert status[s] == UNCORRECTABLE and counts[s][1] >= bad, (s, counts[s].tolist())
        else:
            assert status[s] == (CORRECTED if diff.any() else CLEAN), (s, int(status[s]))
            assert counts[s][1] == 0


def erase(buf, present, stripe, shards):
    for q in shards:
        buf[stripe, q] = 0xEE
        present[stripe, q] = 0


@pytest.mark.parametrize("k,p,length", CASES)
def test_all_clean(k, p, length):
    ref = reference(k, p, length)
    result = correct(R.galois_8.ReedSolomon(k, p), ref, length)
    expect(ref, result, ref[:NS])
    assert not result[1].any() and not result[2].any() and not result[3].any()


@pytest.mark.parametrize("k,p,length", CASES)
def test_whole_shard_corruption(k, p, length):
    n, t = k + p, p // 2
    rng = np.random.default_rng(7)
    ref = reference(k, p, length)
    buf = ref.copy()
    if t == 0:  # 1+1: no error can be corrected; every column is left as it was
        corrupt_shards(buf, rng, 0, [0])
        corrupt_shards(buf, rng, 2, [1])
        result = correct(R.galois_8.ReedSolomon(k, p), buf, length)
        expect(buf, result, buf[:NS], undecodable=[length, 0, length, 0, 0])
        assert result[3][0][1] == length and result[3][2][1] == length
        return
    many = {0, n - 1} if t >= 2 else {n - 1}
    while len(many) < t:
        many.add(int(rng.integers(1, n - 1)))
    shards = [{min(1, n - 1)}, many, set(range(k, k + t))]  # one, t, t parity shards only
    for s in range(3):
        corrupt_shards(buf, rng, s, sorted(shards[s]))
    result = correct(R.galois_8.ReedSolomon(k, p), buf, length)
    expect(buf, result, ref[:NS])
    for s in range(3):
        assert set(np.nonzero(result[2][s])[0].tolist()) == shards[s]
        assert result[3][s][0] == len(shards[s]) * length


@pytest.mark.parametrize("k,p,length", [c for c in CASES if c[1] >= 2])
def test_single_wrong_bytes(k, p, length):
    n = k + p
    rng = np.random.default_rng(11)
    ref = reference(k, p, length)
    buf = ref.copy()
    tail = (length // 16) * 16 if length % 16 else length - 1  # first byte of a ragged tail
    a, b, c = 0, n - 1, k // 2
    corrupt_shards(buf, rng, 0, [a], cols=[0])
    corrupt_shards(buf, rng, 1, [b], cols=[length - 1])
    corrupt_shards(buf, rng, 2, [c], cols=[min(tail, length - 1)])
    result = correct(R.galois_8.ReedSolomon(k, p), buf, length)
    expect(buf, result, ref[:NS])
    assert result[3][:, 0].tolist() == [1, 1, 1, 0, 0]  # exactly those bytes
    assert [np.nonzero(result[2][s])[0].tolist() for s in range(3)] == [[a], [b], [c]]


@pytest.mark.parametrize("k,p,length", [c for c in CASES if c[1] >= 2 and c[2] >= 15])
def test_disjoint_sets_in_different_columns(k, p, length):
    rng = np.random.default_rng(13)
    ref = reference(k, p, length)
    buf = ref.copy()
    for stripe, size in ((1, p), (3, p + 1)):
        sets, cols = disjoint_columns(k, p, length, rng, size)
        for shards, col in zip(sets, cols):
            corrupt_shards(buf, rng, stripe, shards, cols=[col])
        assert len(set(sum(sets, []))) == size
    r = R.galois_8.ReedSolomon(k, p)
    # what the feature adds: p + 1 shards implicated, no column past t -- locate gives up
    _, located = r.locate_flat(torch.from_numpy(buf).cuda(), length, NS)
    assert located.cpu().tolist() == [CLEAN, 1, CLEAN, UNCORRECTABLE, CLEAN]
    result = correct(r, buf, length)
    expect(buf, result, ref[:NS])
    assert result[1].tolist() == [CLEAN, CORRECTED, CLEAN, CORRECTED, CLEAN]
    assert result[2][1].sum() == p and result[2][3].sum() == p + 1


# t + 1 wrong shards in EVERY column: each column is undecodable or lies within
# t of another codeword.  Seeds fixed on the CPU with the model, so that the
# modelled columns hold an undecodable one.
@pytest.mark.parametrize("k,p,length,seed", [(3, 2, 17, 1), (10, 4, 17, 1), (10, 4, 4096 + 16, 1)])
def test_one_more_than_t_wrong_shards_in_every_column(k, p, length, seed):
    n, t = k + p, p // 2
    rng = np.random.default_rng(seed)
    ref = reference(k, p, length)
    buf = ref.copy()
    corrupt_shards(buf, rng, 2, [int(q) for q in rng.permutation(n)[:t + 1]])
    cols = min(length, MODEL_COLS)
    code, want, bad = CM.correct_stripe(k, p, buf[2][:, :cols], [])
    assert code == UNCORRECTABLE and bad >= 1
    got, status, changed, counts = correct(R.galois_8.ReedSolomon(k, p), buf, length)
    assert status.tolist() == [CLEAN, CLEAN, UNCORRECTABLE, CLEAN, CLEAN]
    assert (got[2][:, :cols] == want).all(), "left as it was, or the model's other codeword"
    assert counts[2][1] >= bad and counts[2][1] <= length
    if cols == length:
        assert counts[2][1] == bad and counts[2][0] == (want != buf[2]).sum()
        assert (changed[2] == (want != buf[2]).any(axis=1)).all()
    for s in (0, 1, 3, 4):
        assert (got[s] == ref[s]).all() and not changed[s].any() and not counts[s].any()


@pytest.mark.parametrize("k,p,length", CASES)
def test_erasures(k, p, length):
    n = k + p
    rng = np.random.default_rng(29)
    ref = reference(k, p, length)
    buf = ref.copy()
    present = np.ones((NS, n), np.uint8)
    # stripe 0: p erasures, no error -- both ends of the point shift among them
    shards = [int(q) for q in rng.permutation(np.arange(1, n - 1))[:max(0, p - 2)]]
    erase(buf, present, 0, ([0, n - 1] + shards)[:p])
    # stripe 1: p - 2 erasures and one wholly corrupted shard
    if p >= 3:
        perm = [int(q) for q in rng.permutation(n)]
        erase(buf, present, 1, perm[:p - 2])
        corrupt_shards(buf, rng, 1, perm[p - 2:p - 1])
    # stripe 2: one erasure and (p - 1) // 2 wrong shards
    perm = [int(q) for q in rng.permutation(n)]
    erase(buf, present, 2, perm[:1])
    corrupt_shards(buf, rng, 2, perm[1:1 + (p - 1) // 2])
    # stripe 3: p + 1 erasures -- not touched; stripe 4: nothing erased, clean
    erase(buf, present, 3, [int(q) for q in rng.permutation(n)[:p + 1]])
    want = ref[:NS].copy()
    want[3] = buf[3]
    got, status, changed, counts = correct(R.galois_8.ReedSolomon(k, p), buf, length, present)
    assert status[3] == UNCORRECTABLE and (got[3] == buf[3]).all()
    assert not changed[3].any() and counts[3].tolist() == [0, 0]
    keep = [0, 1, 2, 4]
    expect(buf[keep], (got[keep], status[keep], changed[keep], counts[keep]), want[keep])


@pytest.mark.parametrize("k,p,length", [c for c in CASES if c[1] >= 2])
def test_one_error_too_many_beside_erasures(k, p, length):
    """p - 1 erasures and one error: 2 + (p - 1) > p.  The error sits in the
    first columns only, which are checked against the model; the columns past
    them have the erasures alone and must come out as the oracle's encode."""
    n = k + p
    rng = np.random.default_rng(31)
    ref = reference(k, p, length)
    buf = ref.copy()
    present = np.ones((NS, n), np.uint8)
    perm = [int(q) for q in rng.permutation(n)]
    era = perm[:p - 1]
    erase(buf, present, 1, era)
    cols = min(length, MODEL_COLS)
    corrupt_shards(buf, rng, 1, perm[p - 1:p], cols=range(cols))
    want = ref[:NS].copy()
    code, want[1][:, :cols], bad = CM.correct_stripe(k, p, buf[1][:, :cols], era)
    result = correct(R.galois_8.ReedSolomon(k, p), buf, length, present)
    expect(buf, result, want, undecodable=[0, bad, 0, 0, 0])
    assert result[3][1][1] == bad


@pytest.mark.parametrize("length", LENGTHS)
def test_one_plus_one_restores_an_erased_shard(length):
    rng = np.random.default_rng(17)
    ref = reference(1, 1, length)
    buf = ref.copy()
    present = np.ones((NS, 2), np.uint8)
    corrupt_shards(buf, rng, 1, [0])
    present[1, 0] = 0  # the corrupted shard, flagged: restored although 1+1 locates nothing
    corrupt_shards(buf, rng, 4, [1])
    present[4, 1] = 0
    corrupt_shards(buf, rng, 2, [0], cols=[length - 1])  # not flagged: left as it was
    want = ref[:NS].copy()
    want[2] = buf[2]
    result = correct(R.galois_8.ReedSolomon(1, 1), buf, length, present)
    expect(buf, result, want, undecodable=[0, 0, 1, 0, 0])
    assert result[1].tolist() == [CLEAN, CORRECTED, UNCORRECTABLE, CLEAN, CORRECTED]


@pytest.mark.parametrize("k,p", [(10, 4), (100, 16)])
def test_round_trip_with_locates_present(k, p):
    length = 4096 + 37
    n, t = k + p, p // 2
    rng = np.random.default_rng(19)
    ref = reference(k, p, length)
    r = R.galois_8.ReedSolomon(k, p)
    buf = ref.copy()
    corrupt_shards(buf, rng, 1, [0, n - 1] + list(range(k - t + 2, k)))  # t shards: LOCATED
    sets, cols = disjoint_columns(k, p, length, rng, p + 1)
    for shards, col in zip(sets, cols):
        corrupt_shards(buf, rng, 2, shards, cols=[col])
    corrupt_shards(buf, rng, 3, [int(q) for q in rng.permutation(n)[:t + 1]])  # past capacity
    corrupt_shards(buf, rng, 4, [2], cols=[length - 1])

    dev = torch.from_numpy(buf).cuda()
    present, located = r.locate_flat(dev, length, NS)
    assert located.cpu().tolist() == [0, 1, 2, 2, 1]
    # locate's flags, the device tensor unchanged: the bad shards of stripes 1 and 4
    # count as erasures now (f = t: errors nowhere else), the others have none
    status, changed, counts = r.correct_flat(dev, length, NS, present)
    assert status.is_cuda and status.dtype == torch.uint8 and tuple(status.shape) == (NS,)
    assert changed.is_cuda and changed.dtype == torch.uint8 and tuple(changed.shape) == (NS, n)
    assert counts.is_cuda and counts.dtype == torch.int32 and tuple(counts.shape) == (NS, 2)
    torch.cuda.synchronize()
    got = dev.cpu().numpy()
    status = status.cpu().numpy()
    assert status.tolist() == [CLEAN, CORRECTED, CORRECTED, UNCORRECTABLE, CORRECTED]
    for s in (0, 1, 2, 4):
        assert (got[s] == ref[s]).all(), "repaired stripes equal the oracle's encode"
    assert (got[NS] == ref[NS]).all(), "guard stripe"
    assert (changed.cpu().numpy() == (got[:NS] != buf[:NS]).any(axis=2)).all()
    assert (counts.cpu().numpy()[:, 0] == (got[:NS] != buf[:NS]).sum(axis=(1, 2))).all()
    assert counts.cpu().numpy()[3, 1] >= 1
    ok = r.verify_flat(dev, length, NS)
    assert ok.tolist() == [bool(c != UNCORRECTABLE) for c in status]

    # a host array of flags is uploaded: the same result
    dev2 = torch.from_numpy(buf).cuda()
    status2, _, _ = r.correct_flat(dev2, length, NS, present.cpu().numpy())
    torch.cuda.synchronize()
    assert (status2.cpu().numpy() == status).all() and (dev2.cpu().numpy() == got).all()


def test_non_default_stream_and_last_kernel():
    k, p, length = 10, 4, 4096
    rng = np.random.default_rng(23)
    ref = reference(k, p, length)
    buf = ref.copy()
    corrupt_shards(buf, rng, 3, [5, 12])
    r = R.galois_8.ReedSolomon(k, p)
    dev = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        status, changed, counts = r.correct_flat(dev, length, NS)
    stream.synchronize()
    assert R.core.last_kernel() == "correct gf8 10+4"
    assert status.cpu().tolist() == [CLEAN, CLEAN, CLEAN, CORRECTED, CLEAN]
    assert np.nonzero(changed.cpu().numpy()[3])[0].tolist() == [5, 12]
    assert counts.cpu().tolist()[3] == [2 * length, 0]
    assert (dev.cpu().numpy() == ref).all()


def test_out_of_scope_codecs_raise():
    buf = torch.zeros(256 * 16 * 2, dtype=torch.uint8, device="cuda")
    for r in (R.galois_16.ReedSolomon(10, 4), R.galois_8.ReedSolomon(10, 17),
              R.galois_8.ReedSolomon(200, 56)):
        with pytest.raises(R.DeviceError):
            r.correct_flat(buf, 16, 1)
    with pytest.raises(R.RSError):
        R.galois_8.ReedSolomon(10, 4).correct_flat(buf, 0, 1)
    status, changed, counts = R.galois_8.ReedSolomon(10, 4).correct_flat(buf, 16, 0)
    assert tuple(status.shape) == (0,) and tuple(changed.shape) == (0, 14)
    assert tuple(counts.shape) == (0, 2)
    with pytest.raises(R.RSError):  # flags of the wrong shape
        R.galois_8.ReedSolomon(10, 4).correct_flat(buf, 16, 2, np.ones((2, 13), np.uint8))
