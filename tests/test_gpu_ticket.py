"""The bit-sliced kernels that claim their 16 KiB chunks from a device counter
(RSE_OPT_KERNEL_VARIANT 10: one counter, 11: one per label blockIdx.x % 8 with
stealing; csrc/rse_bitslice_ticket.hpp), byte for byte against the CPU oracle.

Every output is filled with a poison byte first, so a chunk that no workgroup
claimed shows; a chunk claimed twice would be coded twice into the same bytes
and cannot show here, but the per-label bounds that rule it out are exercised
by the grids below (0, 1, 2 and all chunks per workgroup, labels without a
workgroup, labels that must steal).
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

CHUNK = 16384
POISON = 0xA5
# The variant that store-mode GF(2^8) launches of more than MIN_ROUNDS rounds of
# resident workgroups take by default (rse_bitslice.hip kBsTicketDefault), None:
# they keep variant 5.
DEFAULT_TICKET = 11
MIN_ROUNDS = 85  # rse_bitslice.hip kBsTicketMinRounds

# (field, k, p, RSE_OPT_SUBFIELD)
CODECS = [(8, 10, 4, 1), (8, 10, 2, 1), (16, 20, 8, 1), (16, 20, 8, 0)]
CODEC_IDS = ["gf8-10+4", "gf8-10+2", "gf16-20+8-sub", "gf16-20+8"]


@pytest.fixture(scope="module")
def R():
    import reed_solomon_erasure as R
    return R


@pytest.fixture
def opts(R):
    """set(key, value) for this test; every key is restored afterwards."""
    lib = R._lib.load()
    old = {}

    def set_(key, value):
        old.setdefault(key, lib.rse_get_option(key))
        assert lib.rse_set_option(key, value) == 0

    yield set_
    for key, value in old.items():
        lib.rse_set_option(key, value)


def codec(R, opts, field, k, p, sub):
    opts(34, sub)  # read when the codec is created
    return R.core.ReedSolomon(k, p, field)


@functools.lru_cache(maxsize=None)
def stripes_ref(field, k, p, nbytes, stripes):
    """`stripes` encoded stripes of k + p shards of nbytes each, flat, from
    the oracle.  Shared by the tests: never written to."""
    rng = np.random.default_rng(field * 1000 + k * 10 + p + nbytes)
    oc = O.Codec(field, k, p)
    out = []
    for _ in range(stripes):
        st = [rng.integers(0, 256, nbytes, dtype=np.uint8) for _ in range(k)] + \
             [np.zeros(nbytes, np.uint8) for _ in range(p)]
        oc.encode(st)
        out.append(np.concatenate(st))
    ref = np.concatenate(out)
    ref.setflags(write=False)
    return ref


def poisoned(ref, k, p, nbytes, stripes):
    """The reference's data shards on the device, its parity shards poisoned."""
    v = ref.reshape(stripes, k + p, nbytes).copy()
    v[:, k:, :] = POISON
    return torch.from_numpy(v.reshape(-1)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def kernel_id(field, k, p, variant):
    return f"bitslice gf{field} {k}+{p} v{variant} nt1"


@pytest.mark.parametrize("grid", [1, 7, 8, 16, 4096])
@pytest.mark.parametrize("variant", [10, 11])
@pytest.mark.parametrize("field,k,p,sub", CODECS, ids=CODEC_IDS)
def test_encode_variants_grids_codecs(R, opts, field, k, p, sub, variant, grid):
    """3 stripes of 5 x 16 KiB: 15 chunks, so the workgroups get all, 2 or 3,
    1 or 2, 0 or 1 chunks, and with 8 labels over 15 chunks (1 or 2 each) the
    grids below 8 leave labels without a workgroup: their chunks are stolen."""
    stripes, nbytes = 3, 5 * CHUNK
    ref = stripes_ref(field, k, p, nbytes, stripes)
    r = codec(R, opts, field, k, p, sub)
    opts(4, variant)
    opts(2, grid)
    d = poisoned(ref, k, p, nbytes, stripes)
    r.encode_flat(d, nbytes // (field // 8), stripes)
    got = host(d)
    kf = 8 if sub else field
    assert R.core.last_kernel() == kernel_id(kf, k, p, variant)
    assert (got == ref).all()


@pytest.mark.parametrize("variant", [10, 11])
def test_one_stripe_of_one_chunk(R, opts, variant):
    ref = stripes_ref(8, 10, 4, CHUNK, 1)
    r = codec(R, opts, 8, 10, 4, 1)
    opts(4, variant)
    d = poisoned(ref, 10, 4, CHUNK, 1)
    r.encode_flat(d, CHUNK, 1)
    assert R.core.last_kernel() == kernel_id(8, 10, 4, variant)
    assert (host(d) == ref).all()


@pytest.mark.parametrize("variant", [10, 11])
def test_ragged_shard(R, opts, variant):
    """2 x 16 KiB + 4 KiB + 48 B: the 4 KiB chunk and the ragged end go to the
    existing kernels; the whole shard must be right."""
    k, p, nbytes = 10, 4, 2 * CHUNK + 4096 + 48
    ref = stripes_ref(8, k, p, nbytes, 1)
    r = codec(R, opts, 8, k, p, 1)
    opts(4, variant)
    d = poisoned(ref, k, p, nbytes, 1)
    dv = d.view(k + p, nbytes)
    r.encode([dv[i] for i in range(k + p)])
    assert R.core.last_kernel() == kernel_id(8, k, p, variant)  # the 16 KiB chunks' launch
    assert (host(d) == ref).all()


@pytest.mark.parametrize("variant", [10, 11])
@pytest.mark.parametrize("field,k,p,sub", CODECS, ids=CODEC_IDS)
def test_check_modes(R, opts, field, k, p, sub, variant):
    stripes, nbytes = 3, 5 * CHUNK
    es = field // 8
    ref = stripes_ref(field, k, p, nbytes, stripes)
    r = codec(R, opts, field, k, p, sub)
    opts(4, variant)
    T = k + p
    shape = (nbytes,) if field == 8 else (nbytes // 2, 2)
    d = torch.from_numpy(ref.copy()).cuda()
    mid = [d.view(stripes, T, nbytes)[1, i].view(*shape) for i in range(T)]
    # check: clean, then one flipped byte in the last chunk of the middle stripe
    kid = kernel_id(8 if sub else field, k, p, variant)
    assert r.verify(mid)
    assert R.core.last_kernel() == kid
    assert r.verify_flat(d, nbytes // es, stripes).tolist() == [True, True, True]
    assert R.core.last_kernel() == kid
    # check + store: the buffer takes the parity
    buf = [torch.full(shape, POISON, dtype=torch.uint8, device="cuda") for _ in range(p)]
    assert r.verify_with_buffer(mid, buf)
    assert R.core.last_kernel() == kid
    want = ref.reshape(stripes, T, nbytes)
    for i in range(p):
        assert (host(buf[i]).reshape(-1) == want[1, k + i]).all()
    bad = ref.copy()
    bad.reshape(stripes, T, nbytes)[1, 3, 4 * CHUNK + 77] ^= 0x40
    d = torch.from_numpy(bad).cuda()
    mid = [d.view(stripes, T, nbytes)[1, i].view(*shape) for i in range(T)]
    assert not r.verify(mid)
    assert not r.verify_with_buffer(mid, buf)
    assert r.verify_flat(d, nbytes // es, stripes).tolist() == [True, False, True]
    assert (host(d) == bad).all()  # the check modes of the shards write nothing


@pytest.mark.parametrize("variant", [10, 11])
def test_counter_lifetime_one_stream(R, opts, variant):
    """The same call three times back to back: launches queued on one stream
    never share a counter block, and each finds its block zeroed."""
    k, p, stripes, nbytes = 10, 4, 3, 5 * CHUNK
    ref = stripes_ref(8, k, p, nbytes, stripes)
    r = codec(R, opts, 8, k, p, 1)
    opts(4, variant)
    opts(2, 7)
    d = poisoned(ref, k, p, nbytes, stripes)
    par = d.view(stripes, k + p, nbytes)[:, k:, :]
    for _ in range(3):
        par.fill_(POISON)  # stream-ordered between the calls
        r.encode_flat(d, nbytes, stripes)
    assert (host(d) == ref).all()


@pytest.mark.parametrize("variant", [10, 11])
def test_counter_lifetime_two_streams(R, opts, variant):
    """Two codecs launched alternately on two streams without a synchronise
    between them: launches on different streams never share a counter."""
    stripes, nbytes = 3, 5 * CHUNK
    refs = [stripes_ref(8, 10, 4, nbytes, stripes), stripes_ref(8, 10, 2, nbytes, stripes)]
    rs = [codec(R, opts, 8, 10, 4, 1), codec(R, opts, 8, 10, 2, 1)]
    opts(4, variant)
    opts(2, 7)
    bufs = [[poisoned(refs[c], 10, (4, 2)[c], nbytes, stripes) for _ in range(3)] for c in range(2)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for i in range(3):
        for c in range(2):
            with torch.cuda.stream(streams[c]):
                rs[c].encode_flat(bufs[c][i], nbytes, stripes)
    torch.cuda.synchronize()
    for c in range(2):
        for i in range(3):
            assert (bufs[c][i].cpu().numpy() == refs[c]).all()


def test_default_selection(R, opts):
    """Store-mode 10+4 launches of more than MIN_ROUNDS rounds of resident
    workgroups take the default ticket variant (DEFAULT_TICKET; None: variant
    5), checked against the oracle on the first, a middle and the last stripe
    and against variant 5 on every byte; one stripe just past two rounds and a
    1 MiB stripe keep variant 5."""
    k, p = 10, 4
    r = codec(R, opts, 8, k, p, 1)
    opts(4, -1)
    opts(2, 0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    resident = 3 * cus  # 3 workgroups per CU at most (launch bounds)
    nbytes = 1 << 20  # 64 chunks a stripe
    stripes = MIN_ROUNDS * resident // 64 + 1
    buf = torch.empty(stripes * (k + p) * nbytes, dtype=torch.uint8, device="cuda")
    R.core.fill_splitmix(buf, 1, 0)
    v = buf.view(stripes, k + p, nbytes)
    v[:, k:, :] = POISON
    other = buf.clone()
    r.encode_flat(buf, nbytes, stripes)
    assert R.core.last_kernel() == kernel_id(8, k, p, DEFAULT_TICKET or 5)
    oc = O.Codec(8, k, p)
    for s_ in (0, stripes // 2, stripes - 1):
        got = host(v[s_])
        want = [got[i].copy() for i in range(k)] + [np.zeros(nbytes, np.uint8) for _ in range(p)]
        oc.encode(want)
        assert (got[k:] == np.stack(want[k:])).all()
    opts(4, 5)
    r.encode_flat(other, nbytes, stripes)
    assert R.core.last_kernel() == kernel_id(8, k, p, 5)
    assert torch.equal(buf, other)
    opts(4, -1)
    for nbytes in ((2 * resident + 1) * CHUNK, 1 << 20):
        ref = stripes_ref(8, k, p, nbytes, 1)
        d = poisoned(ref, k, p, nbytes, 1)
        r.encode_flat(d, nbytes, 1)
        assert R.core.last_kernel() == kernel_id(8, k, p, 5)
        assert (host(d) == ref).all()
