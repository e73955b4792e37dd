"""The additive-FFT kernel of GF(2^8) 128+128 (rse_fft.hip fft_kernel_quads,
RSE_OPT_FFT = option 51 at 2; the default 1 keeps 128+128 on its wide modules)
against the oracle's coefficient-matrix encode and reconstruct
(core.rs:481-509, 680-923).

Covered: flat encode / verify / rebuild of 1 KiB shards (two stripes per
column, odd counts), whole 2 KiB columns and ragged tails, every stripe
against the oracle, a guard after the batch; workgroups that loop over several
columns (RSE_OPT_GRID_X 2; also for k = p = 16, 32, 64); the per-shard API;
shapes the kernel does not cover (under one column, a misaligned pointer); the
option's three values; GF(2^16) 128+128, which codes in the GF(2^8) subfield.
Every case restores the options it sets."""
import contextlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

K = 128
T = 2 * K


@pytest.fixture(scope="module")
def R():
    import reed_solomon_erasure as R
    return R


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@contextlib.contextmanager
def options(R, **kv):
    """Sets library options by key ("o51"=2), restores them afterwards."""
    lib = R._lib.load()
    old = {int(k_[1:]): lib.rse_get_option(int(k_[1:])) for k_ in kv}
    try:
        for k_, v in kv.items():
            assert lib.rse_set_option(int(k_[1:]), v) == 0
        yield lib
    finally:
        for key, v in old.items():
            lib.rse_set_option(key, v)


def oracle_stripes(field, k, data):
    """data[stripe][k][nb] -> full[stripe][2k][nb] with the oracle's parity."""
    oc = O.Codec(field, k, k)
    stripes, _, nb = data.shape
    full = np.zeros((stripes, 2 * k, nb), np.uint8)
    for s_ in range(stripes):
        sh = [data[s_, i].copy() for i in range(k)] + [np.zeros(nb, np.uint8) for _ in range(k)]
        oc.encode(sh)
        full[s_] = np.stack(sh)
    return full


@pytest.mark.parametrize("nb", [1024, 2048, 4096, 2048 + 48, 6144 + 16])
def test_fft128_flat_encode_verify_rebuild(R, nb):
    from reed_solomon_erasure.core import last_kernel
    counts = (1, 2, 3, 7) if nb <= 2048 else (1, 2, 3)
    smax = max(counts)
    rng = np.random.default_rng(128000 + nb)
    # one batch of smax stripes and a guard stripe; smaller counts code its
    # first stripes, so the oracle runs once per stripe
    buf = rng.integers(0, 256, (smax + 1, T, nb), dtype=np.uint8)
    want = oracle_stripes(8, K, buf[:smax, :K])
    with options(R, o51=2):
        r = R.galois_8.ReedSolomon(K, K)
        for stripes in counts:
            d = dev(buf.reshape(-1))
            r.encode_flat(d, nb, stripes)
            kern = last_kernel()
            assert kern.startswith("fft gf8 128+128 code"), kern
            got = host(d).reshape(smax + 1, T, nb)
            assert (got[stripes:] == buf[stripes:]).all()  # guard (and the stripes past the batch)
            assert (got[:, :K] == buf[:, :K]).all()
            for s_ in range(stripes):  # every stripe
                bad = np.argwhere(got[s_, K:] != want[s_, K:])
                assert bad.size == 0, (stripes, s_, bad[:4])
            # per-stripe verdicts: a parity byte, and a data byte in another stripe
            good = host(d)
            v = good.reshape(smax + 1, T, nb).copy()
            want_ok = np.ones(stripes, bool)
            hits = {stripes - 1: K + int(rng.integers(0, K))}
            if stripes > 1:
                hits[0] = int(rng.integers(0, K))
            for s_, i in hits.items():
                v[s_, i, int(rng.integers(0, nb))] ^= 0x5A
                want_ok[s_] = False
            dv = dev(v.reshape(-1))
            assert (r.verify_flat(dv, nb, stripes) == want_ok).all()
            assert last_kernel().startswith("fft gf8 128+128 check"), last_kernel()
            assert r.verify_flat(d, nb, stripes).all()
            # every data shard rebuilt from the parity shards
            d.view(smax + 1, T, nb)[:stripes, :K].fill_(0xA5)
            r.reconstruct_data_flat(d, nb, stripes, [i >= K for i in range(T)])
            assert last_kernel().startswith("fft gf8 128+128 code"), last_kernel()
            assert (host(d) == good).all()


@pytest.mark.parametrize("nb", [4096, 1024])
@pytest.mark.parametrize("k", [16, 32, 64, 128])
def test_fft_workgroups_loop_over_columns(R, k, nb):
    """Two workgroups for 5 stripes (10 columns of 2 KiB, or 3 columns of two
    1 KiB stripes with the last one's second stripe clamped): each codes
    several columns, with the next column's inputs loaded ahead."""
    from reed_solomon_erasure.core import last_kernel
    stripes = 5
    rng = np.random.default_rng(2000 + k + nb)
    buf = rng.integers(0, 256, (stripes + 1, 2 * k, nb), dtype=np.uint8)
    want = oracle_stripes(8, k, buf[:stripes, :k])
    with options(R, o51=2 if k == 128 else 1, o2=2):
        r = R.galois_8.ReedSolomon(k, k)
        d = dev(buf.reshape(-1))
        r.encode_flat(d, nb, stripes)
        assert last_kernel().startswith(f"fft gf8 {k}+{k} code"), last_kernel()
        got = host(d).reshape(stripes + 1, 2 * k, nb)
        assert (got[stripes] == buf[stripes]).all()
        for s_ in range(stripes):
            assert (got[s_] == want[s_]).all(), s_
        assert r.verify_flat(d, nb, stripes).all()
        assert last_kernel().startswith(f"fft gf8 {k}+{k} check"), last_kernel()


def test_fft128_per_shard_calls(R):
    from reed_solomon_erasure.core import last_kernel
    nb = 4096 + 2048
    rng = np.random.default_rng(128)
    data = rng.integers(0, 256, (1, K, nb), dtype=np.uint8)
    want = oracle_stripes(8, K, data)[0]
    with options(R, o51=2):
        r = R.galois_8.ReedSolomon(K, K)
        sh = [dev(data[0, i]) for i in range(K)] + \
             [torch.zeros(nb, dtype=torch.uint8, device="cuda") for _ in range(K)]
        r.encode(sh)
        assert last_kernel().startswith("fft"), last_kernel()
        for i in range(T):
            assert (host(sh[i]) == want[i]).all(), i
        assert r.verify(sh)
        assert last_kernel().startswith("fft"), last_kernel()
        sh[K + 3][77] ^= 1
        assert not r.verify(sh)
        sh[K + 3][77] ^= 1
        for data_only in (True, False):
            for i in range(K):
                sh[i].fill_(0)
            pairs = [(s, i >= K) for i, s in enumerate(sh)]
            if data_only:
                r.reconstruct_data(pairs)
            else:
                r.reconstruct(pairs)
            assert last_kernel().startswith("fft"), last_kernel()
            for i in range(T):
                assert (host(sh[i]) == want[i]).all(), (data_only, i)


def test_fft128_shapes_the_kernel_does_not_cover(R):
    """Shards under one column, and a parity pointer that is not 16-byte
    aligned, go to the other kernels with the same bytes."""
    from reed_solomon_erasure.core import last_kernel
    with options(R, o51=2):
        r = R.galois_8.ReedSolomon(K, K)
        # under one 2 KiB column (and not 1 KiB)
        nb, stripes = 512 + 16, 2
        rng = np.random.default_rng(1281)
        buf = rng.integers(0, 256, (stripes, T, nb), dtype=np.uint8)
        want = oracle_stripes(8, K, buf[:, :K])
        d = dev(buf.reshape(-1))
        r.encode_flat(d, nb, stripes)
        assert not last_kernel().startswith("fft"), last_kernel()
        assert (host(d).reshape(stripes, T, nb) == want).all()
        assert r.verify_flat(d, nb, stripes).all()
        assert not last_kernel().startswith("fft"), last_kernel()
        d.view(stripes, T, nb)[:, :K].fill_(0)
        r.reconstruct_data_flat(d, nb, stripes, [i >= K for i in range(T)])
        assert not last_kernel().startswith("fft"), last_kernel()
        assert (host(d).reshape(stripes, T, nb) == want).all()
        # one parity shard at offset 8 of a larger buffer
        nb = 4096
        data = rng.integers(0, 256, (1, K, nb), dtype=np.uint8)
        want1 = oracle_stripes(8, K, data)[0]
        big = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")
        sh = [dev(data[0, i]) for i in range(K)] + \
             [torch.zeros(nb, dtype=torch.uint8, device="cuda") for _ in range(K)]
        sh[K + 5] = big[8:8 + nb]
        assert sh[K + 5].data_ptr() % 16 == 8
        r.encode(sh)
        assert not last_kernel().startswith("fft"), last_kernel()
        for i in range(T):
            assert (host(sh[i]) == want1[i]).all(), i
        # verify cannot compare against the misaligned shard in the FFT kernel's
        # check mode; it codes the parity into the library's own (aligned)
        # buffer -- from aligned data shards, so on the FFT kernel in store
        # mode, as 64+64 does -- and compares that: only "fft .. check" is excluded
        assert r.verify(sh)
        assert not last_kernel().startswith("fft gf8 128+128 check"), last_kernel()
        sh[K + 5][nb - 1] ^= 0x80
        assert not r.verify(sh)
        sh[K + 5][nb - 1] ^= 0x80
        for i in range(K):
            sh[i].fill_(0)
        r.reconstruct([(s, i >= K) for i, s in enumerate(sh)])
        assert not last_kernel().startswith("fft"), last_kernel()
        for i in range(T):
            assert (host(sh[i]) == want1[i]).all(), i
        assert (host(big)[:8] == 0).all() and (host(big)[8 + nb:] == 0).all()


def test_fft128_option_values(R):
    from reed_solomon_erasure.core import last_kernel
    nb, stripes = 2048, 2
    rng = np.random.default_rng(1285)
    buf = rng.integers(0, 256, (stripes, T, nb), dtype=np.uint8)
    buf64 = rng.integers(0, 256, (stripes, 128, nb), dtype=np.uint8)
    out = {}
    for value in (2, 1, 0):
        with options(R, o51=value) as lib:
            assert lib.rse_get_option(51) == value
            r = R.galois_8.ReedSolomon(K, K)
            if value == 2:
                assert r.kernel_kind() == "fft-compiled"
            else:
                assert r.kernel_kind() != "fft-compiled"
            d = dev(buf.reshape(-1))
            r.encode_flat(d, nb, stripes)
            assert last_kernel().startswith("fft gf8 128+128") == (value == 2), (value, last_kernel())
            out[value] = host(d)
            r64 = R.galois_8.ReedSolomon(64, 64)
            d64 = dev(buf64.reshape(-1))
            r64.encode_flat(d64, nb, stripes)
            assert last_kernel().startswith("fft gf8 64+64") == (value != 0), (value, last_kernel())
    assert (out[1] == out[2]).all() and (out[0] == out[2]).all()
    with options(R, o51=1) as lib:  # any other nonzero value counts as 1
        for v in (3, -1, 7):
            assert lib.rse_set_option(51, v) == 0 and lib.rse_get_option(51) == 1


def test_fft128_gf16_subfield_codec(R):
    from reed_solomon_erasure.core import last_kernel
    n_elems, stripes = 2048 + 24, 2
    nb = 2 * n_elems
    rng = np.random.default_rng(16128)
    data = rng.integers(0, 256, (stripes, K, nb), dtype=np.uint8)
    full = oracle_stripes(16, K, data)
    with options(R, o51=2):
        r = R.galois_16.ReedSolomon(K, K)
        assert r.kernel_kind() == "fft-compiled"
        buf = full.copy()
        buf[:, K:] = 0x69
        d = dev(buf.reshape(-1))
        r.encode_flat(d, n_elems, stripes)
        assert last_kernel().startswith("fft gf8 128+128 code") or \
            not last_kernel().startswith("fft"), last_kernel()  # the tail ran last
        assert (host(d).reshape(stripes, T, nb) == full).all()
        assert r.verify_flat(d, n_elems, stripes).all()
        d.view(stripes, T, nb)[:, :K].fill_(0)
        r.reconstruct_data_flat(d, n_elems, stripes, [i >= K for i in range(T)])
        assert (host(d).reshape(stripes, T, nb) == full).all()
