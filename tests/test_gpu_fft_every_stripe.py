"""Every stripe of a batch coded by the additive-FFT kernels of GF(2^8)
k = p = 16, 32 and 64 (rse_fft.hip) against the oracle's matrix encode
(core.rs:481-509): tests/test_gpu_fft.py compares the first, middle and last
stripe only.  7 stripes of 1 KiB shards (two stripes per 2 KiB column, the
last column half empty) and of 2 KiB + 48 B shards (a column and a tail for
the other kernels)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    import reed_solomon_erasure as R
    return R


@pytest.mark.parametrize("nb", [1024, 2048 + 48])
@pytest.mark.parametrize("k", [16, 32, 64])
def test_fft_every_stripe_equals_the_oracle(R, k, nb):
    from reed_solomon_erasure.core import last_kernel
    stripes, T = 7, 2 * k
    oc = O.Codec(8, k, k)
    rng = np.random.default_rng(7000 + k + nb)
    buf = rng.integers(0, 256, (stripes + 1, T, nb), dtype=np.uint8)
    r = R.galois_8.ReedSolomon(k, k)
    d = torch.from_numpy(buf.reshape(-1).copy()).cuda()
    r.encode_flat(d, nb, stripes)
    assert last_kernel().startswith(f"fft gf8 {k}+{k} code"), last_kernel()
    torch.cuda.synchronize()
    got = d.cpu().numpy().reshape(stripes + 1, T, nb)
    assert (got[stripes] == buf[stripes]).all()  # guard stripe untouched
    assert (got[:, :k] == buf[:, :k]).all()
    for s_ in range(stripes):
        want = [buf[s_, i].copy() for i in range(k)] + [np.zeros(nb, np.uint8) for _ in range(k)]
        oc.encode(want)
        for i in range(k):
            assert (got[s_, k + i] == want[k + i]).all(), (s_, i)
