"""The pruned additive-FFT kernel of GF(2^16) codecs past 256 shards with
2^m - k <= 32 (rse_fft16.hip, RSE_OPT_FFT16 = option 54 at 1; the default 0
leaves these codecs on their other kernels) against the oracle's
coefficient-matrix encode and reconstruct (core.rs:481-509, 680-923).

Covered: 500+12 (u = 12), 490+12 (u = 22: padding points) and 480+24 (u = 32)
on whole 4 KiB columns and with a ragged tail, 1 to 3 stripes with every stripe
against the oracle and a guard stripe after the batch; per-stripe verdicts;
three erasure patterns through the flat and the per-shard calls; workgroups
that loop over several columns (RSE_OPT_GRID_X 2); shapes the kernel does not
cover (a misaligned shard, shards under one column); 1000+24 with run-time
modules off; the option at 0.  Every case restores the options it sets."""
import contextlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(500, 12), (490, 12), (480, 24)]
SMAX = 3


@pytest.fixture(scope="module")
def R():
    import reed_solomon_erasure as R
    return R


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()  # a copy: the shared arrays are read-only


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@contextlib.contextmanager
def options(R, **kv):
    """Sets library options by key ("o54"=1), restores them afterwards."""
    lib = R._lib.load()
    old = {int(k_[1:]): lib.rse_get_option(int(k_[1:])) for k_ in kv}
    try:
        for k_, v in kv.items():
            assert lib.rse_set_option(int(k_[1:]), v) == 0
        yield lib
    finally:
        for key, v in old.items():
            lib.rse_set_option(key, v)


def last_kernel():
    from reed_solomon_erasure.core import last_kernel as lk
    return lk()


_WANT = {}


def stripes_of(k, p, nb, seed=0):
    """(buf, want): SMAX random stripes and a guard stripe of k+p shards of nb
    bytes, and the first SMAX with the oracle's parity.  Made once per case and
    never written to."""
    key = (k, p, nb, seed)
    if key not in _WANT:
        oc = O.Codec.shared(16, k, p)
        rng = np.random.default_rng(16000 + 7 * k + p + nb + seed)
        buf = rng.integers(0, 256, (SMAX + 1, k + p, nb), dtype=np.uint8)
        want = buf[:SMAX].copy()
        for s_ in range(SMAX):
            sh = [want[s_, i].copy() for i in range(k)] + [np.zeros(nb, np.uint8) for _ in range(p)]
            oc.encode(sh)
            want[s_] = np.stack(sh)
        buf.setflags(write=False)
        want.setflags(write=False)
        _WANT[key] = (buf, want)
    return _WANT[key]


def patterns(k, p):
    """Lost shards: a mix of data and parity, all parity, p data shards."""
    return {"mixed": [1, k // 2, k - 1, k, k + p - 1],
            "all-parity": list(range(k, k + p)),
            "p-data": list(range(5, 5 + p))}


@pytest.mark.parametrize("nb", [4096, 8192 + 32])
@pytest.mark.parametrize("k,p", SHAPES)
def test_fft16_flat_encode_verify(R, k, p, nb):
    T, ne = k + p, nb // 2
    buf, want = stripes_of(k, p, nb)
    rng = np.random.default_rng(k + nb)
    with options(R, o54=1):
        r = R.galois_16.ReedSolomon(k, p)
        assert r.kernel_kind() == "fft-compiled"
        for stripes in (1, 2, 3):
            d = dev(buf.reshape(-1))
            r.encode_flat(d, ne, stripes)
            assert last_kernel() == f"fft gf16 {k}+{p} code", last_kernel()
            got = host(d).reshape(SMAX + 1, T, nb)
            assert (got[stripes:] == buf[stripes:]).all()  # guard, and the stripes past the batch
            assert (got[:, :k] == buf[:, :k]).all()
            for s_ in range(stripes):  # every stripe
                bad = np.argwhere(got[s_, k:] != want[s_, k:])
                assert bad.size == 0, (stripes, s_, bad[:4])
            # per-stripe verdicts: a parity byte, and a data byte in another stripe
            v = got.copy()
            want_ok = np.ones(stripes, bool)
            hits = {stripes - 1: k + int(rng.integers(0, p))}
            if stripes > 1:
                hits[0] = int(rng.integers(0, k))
            for s_, i in hits.items():
                v[s_, i, int(rng.integers(0, nb))] ^= 0x5A
                want_ok[s_] = False
            dv = dev(v.reshape(-1))
            assert (r.verify_flat(dv, ne, stripes) == want_ok).all()
            assert last_kernel() == f"fft gf16 {k}+{p} check", last_kernel()
            assert r.verify_flat(d, ne, stripes).all()


@pytest.mark.parametrize("name", ["mixed", "all-parity", "p-data"])
@pytest.mark.parametrize("nb", [4096, 8192 + 32])
@pytest.mark.parametrize("k,p", SHAPES)
def test_fft16_reconstruct(R, k, p, nb, name):
    T, ne = k + p, nb // 2
    _, want = stripes_of(k, p, nb)
    lost = patterns(k, p)[name]
    present = [i not in lost for i in range(T)]
    lost_data = [i for i in lost if i < k]
    with options(R, o54=1):
        r = R.galois_16.ReedSolomon(k, p)
        for stripes in (1, 3):
            # flat: the data shards come back, the lost parity stays as it was
            broken = want.copy()
            broken[:stripes, lost] = 0xA5
            d = dev(broken.reshape(-1))
            r.reconstruct_data_flat(d, ne, stripes, present)
            expect = broken.copy()
            expect[:stripes, lost_data] = want[:stripes, lost_data]
            assert (host(d).reshape(SMAX, T, nb) == expect).all(), stripes
            if lost_data:
                assert last_kernel() == f"fft gf16 {k}+{p} rebuild", last_kernel()
        # per shard: every lost shard comes back
        broken = want[0].copy()
        broken[lost] = 0xA5
        d = dev(broken.reshape(-1)).view(T, ne, 2)
        r.reconstruct([(d[i], present[i]) for i in range(T)])
        assert last_kernel() == f"fft gf16 {k}+{p} rebuild", last_kernel()
        assert (host(d).reshape(T, nb) == want[0]).all()
        if lost_data:
            d = dev(broken.reshape(-1)).view(T, ne, 2)
            r.reconstruct_data([(d[i], present[i]) for i in range(T)])
            assert last_kernel() == f"fft gf16 {k}+{p} rebuild", last_kernel()
            expect = broken.copy()
            expect[lost_data] = want[0, lost_data]
            assert (host(d).reshape(T, nb) == expect).all()


def test_fft16_inconsistent_shards_rebuild_as_the_oracle(R):
    """Only the first k present shards are read (core.rs:801-841): a present
    shard past them may hold anything."""
    k, p, nb = 500, 12, 4096
    T = k + p
    _, want = stripes_of(k, p, nb)
    broken = want[0].copy()
    broken[[2, 9]] = 0
    broken[T - 1] ^= 0x3C  # present, but past the first k present shards
    present = [i not in (2, 9) for i in range(T)]
    sh = [broken[i].copy() for i in range(T)]
    O.Codec.shared(16, k, p).reconstruct(sh, present)
    with options(R, o54=1):
        r = R.galois_16.ReedSolomon(k, p)
        d = dev(broken.reshape(-1)).view(T, nb // 2, 2)
        r.reconstruct([(d[i], present[i]) for i in range(T)])
        assert last_kernel() == f"fft gf16 {k}+{p} rebuild", last_kernel()
        assert (host(d).reshape(T, nb) == np.stack(sh)).all()
        assert (host(d).reshape(T, nb)[[2, 9]] == want[0, [2, 9]]).all()


@pytest.mark.parametrize("k,p", SHAPES)
def test_fft16_workgroups_loop_over_columns(R, k, p):
    """Two workgroups for 3 stripes of 2 columns and a tail: each codes three
    columns, of more than one stripe."""
    nb, stripes = 8192 + 32, 3
    T, ne = k + p, nb // 2
    buf, want = stripes_of(k, p, nb)
    lost = patterns(k, p)["mixed"]
    with options(R, o54=1, o2=2):
        r = R.galois_16.ReedSolomon(k, p)
        d = dev(buf.reshape(-1))
        r.encode_flat(d, ne, stripes)
        assert last_kernel() == f"fft gf16 {k}+{p} code", last_kernel()
        got = host(d).reshape(SMAX + 1, T, nb)
        assert (got[stripes] == buf[stripes]).all()
        for s_ in range(stripes):
            assert (got[s_] == want[s_]).all(), s_
        assert r.verify_flat(d, ne, stripes).all()
        assert last_kernel() == f"fft gf16 {k}+{p} check", last_kernel()
        d.view(SMAX + 1, T, nb)[:stripes, lost] = 0
        r.reconstruct_data_flat(d, ne, stripes, [i not in lost for i in range(T)])
        assert last_kernel() == f"fft gf16 {k}+{p} rebuild", last_kernel()
        got = host(d).reshape(SMAX + 1, T, nb)
        for s_ in range(stripes):
            assert (got[s_, :k] == want[s_, :k]).all(), s_


def test_fft16_misaligned_shard_goes_to_the_other_kernels(R):
    k, p, nb = 500, 12, 4096
    T, ne = k + p, nb // 2
    _, want = stripes_of(k, p, nb)
    with options(R, o54=1):
        r = R.galois_16.ReedSolomon(k, p)
        d = dev(want[0, :k].reshape(-1)).view(k, ne, 2)
        big = torch.zeros(p * nb + 64, dtype=torch.uint8, device="cuda")
        par = [big[8 + i * nb:8 + (i + 1) * nb].view(ne, 2) for i in range(p)]
        assert par[3].data_ptr() % 16 == 8
        sh = [d[i] for i in range(k)] + par
        r.encode(sh)
        assert not last_kernel().startswith("fft gf16"), last_kernel()
        assert (host(big)[8:8 + p * nb].reshape(p, nb) == want[0, k:]).all()
        assert (host(big)[:8] == 0).all() and (host(big)[8 + p * nb:] == 0).all()
        assert r.verify(sh)
        assert not last_kernel().startswith(f"fft gf16 {k}+{p} check"), last_kernel()
        par[5].view(-1)[nb - 1] ^= 0x80
        assert not r.verify(sh)
        par[5].view(-1)[nb - 1] ^= 0x80
        d[7].fill_(0)
        par[0].fill_(0)
        r.reconstruct([(s, i not in (7, k)) for i, s in enumerate(sh)])
        assert not last_kernel().startswith("fft gf16"), last_kernel()
        assert (host(d).reshape(k, nb) == want[0, :k]).all()
        assert (host(big)[8:8 + p * nb].reshape(p, nb) == want[0, k:]).all()


def test_fft16_shards_under_one_column_go_to_the_other_kernels(R):
    k, p, nb, stripes = 500, 12, 2048 + 16, 2
    T, ne = k + p, nb // 2
    buf, want = stripes_of(k, p, nb)
    lost = patterns(k, p)["mixed"]
    with options(R, o54=1):
        r = R.galois_16.ReedSolomon(k, p)
        d = dev(buf.reshape(-1))
        r.encode_flat(d, ne, stripes)
        assert not last_kernel().startswith("fft gf16"), last_kernel()
        got = host(d).reshape(SMAX + 1, T, nb)
        assert (got[:stripes] == want[:stripes]).all() and (got[stripes:] == buf[stripes:]).all()
        assert r.verify_flat(d, ne, stripes).all()
        assert not last_kernel().startswith("fft gf16"), last_kernel()
        d.view(SMAX + 1, T, nb)[:stripes, lost] = 0
        r.reconstruct_data_flat(d, ne, stripes, [i not in lost for i in range(T)])
        assert not last_kernel().startswith("fft gf16"), last_kernel()
        assert (host(d).reshape(SMAX + 1, T, nb)[:stripes, :k] == want[:stripes, :k]).all()


def test_fft16_1000_24_needs_no_module(R):
    """1000+24 with run-time modules off: the FFT kind at once, no module built."""
    k, p, nb, stripes = 1000, 24, 4096, 2
    T, ne = k + p, nb // 2
    buf, want = stripes_of(k, p, nb)
    with options(R, o54=1, o9=0) as lib:
        built = lib.rse_get_option(10)
        r = R.galois_16.ReedSolomon(k, p)
        assert r.kernel_kind(wait=False) == "fft-compiled"
        d = dev(buf.reshape(-1))
        r.encode_flat(d, ne, stripes)
        assert last_kernel() == "fft gf16 1000+24 code", last_kernel()
        got = host(d).reshape(SMAX + 1, T, nb)
        assert (got[:stripes] == want[:stripes]).all() and (got[stripes:] == buf[stripes:]).all()
        assert r.verify_flat(d, ne, stripes).all()
        assert last_kernel() == "fft gf16 1000+24 check", last_kernel()
        lost = [0, 333, 999, 1001]
        d.view(SMAX + 1, T, nb)[:stripes, lost] = 0
        r.reconstruct_data_flat(d, ne, stripes, [i not in lost for i in range(T)])
        assert last_kernel() == "fft gf16 1000+24 rebuild", last_kernel()
        assert (host(d).reshape(SMAX + 1, T, nb)[:stripes, :k] == want[:stripes, :k]).all()
        assert lib.rse_get_option(10) == built


def test_fft16_option_off_is_the_default_and_gives_the_same_bytes(R):
    k, p, nb, stripes = 500, 12, 4096, 2
    T, ne = k + p, nb // 2
    buf, want = stripes_of(k, p, nb)
    lib = R._lib.load()
    assert lib.rse_get_option(54) == 0
    r = R.galois_16.ReedSolomon(k, p)
    assert r.kernel_kind() != "fft-compiled"
    d = dev(buf.reshape(-1))
    r.encode_flat(d, ne, stripes)
    assert not last_kernel().startswith("fft gf16"), last_kernel()
    assert (host(d).reshape(SMAX + 1, T, nb)[:stripes] == want[:stripes]).all()
    lost = patterns(k, p)["mixed"]
    d.view(SMAX + 1, T, nb)[:stripes, lost] = 0
    r.reconstruct_data_flat(d, ne, stripes, [i not in lost for i in range(T)])
    assert not last_kernel().startswith("fft gf16"), last_kernel()
    assert (host(d).reshape(SMAX + 1, T, nb)[:stripes, :k] == want[:stripes, :k]).all()
    with options(R, o54=7) as lib:  # any nonzero value counts as 1
        assert lib.rse_get_option(54) == 1
        # a GF(2^16) codec in the subfield, and one with 2^m - k > 32, are not the kernel's
        assert R.galois_16.ReedSolomon(100, 20).kernel_kind() != "fft-compiled"
        assert R.galois_16.ReedSolomon(300, 60).kernel_kind() != "fft-compiled"
