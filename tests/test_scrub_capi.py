"""rse_scrub_flat's validation (include/rse_hip.h), through raw ctypes as
tests/test_correct_capi.py does: every refusal happens before any device call,
so fake pointers are never touched and no GPU is needed.  Order: NULL codec /
stripes / status (present, changed, counts, bad_stripes and n_bad may be NULL),
a codec out of scope, an empty shard, zero stripes, more than 2^32 - 1 stripes.
The scope is rse_correct_flat's and the GF(2^16) codecs of at most 255 shards
with at most 16 parity shards."""
import os
import subprocess
import sys

import reed_solomon_erasure as R
from reed_solomon_erasure import Error
from reed_solomon_erasure._lib import EXPORTS, load

L = load()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000
INVALID = 100  # RSE_ERR_INVALID_ARGUMENT
SCRUB_ROUTE = 56  # RSE_OPT_SCRUB_ROUTE (include/rse_hip_tune.h)
NULLABLE = ("present", "changed", "counts", "bad_stripes", "n_bad")


def call(h, stripes=FAKE, shard_len=16, n_stripes=2, present=FAKE, status=FAKE, changed=FAKE,
         counts=FAKE, bad_stripes=FAKE, n_bad=FAKE):
    return L.rse_scrub_flat(h, stripes, shard_len, n_stripes, present, status, changed, counts,
                            bad_stripes, n_bad, None)


def in_scope():
    return [R.galois_8.ReedSolomon(10, 4), R.galois_8.ReedSolomon(1, 1),
            R.galois_8.ReedSolomon(239, 16), R.galois_16.ReedSolomon(10, 4),
            R.galois_16.ReedSolomon(20, 8)]


def test_symbol_is_exported_and_bound():
    assert "rse_scrub_flat" in EXPORTS
    assert hasattr(L, "rse_scrub_flat")
    assert callable(R.galois_8.ReedSolomon.scrub_flat)
    assert callable(R.galois_16.ReedSolomon.scrub_flat)


def test_null_arguments():
    r = R.galois_8.ReedSolomon(10, 4)
    assert call(None) == INVALID
    assert call(r._h, stripes=None) == INVALID
    assert call(r._h, status=None) == INVALID
    # NULL comes first: before the empty shard, the empty batch and the batch too large
    assert call(r._h, stripes=None, shard_len=0) == INVALID
    assert call(r._h, status=None, n_stripes=0) == INVALID
    assert call(r._h, status=None, shard_len=0, n_stripes=0) == INVALID
    assert call(None, n_stripes=1 << 32) == INVALID


def test_nullable_arguments_are_not_refused():
    # nothing is launched for an empty batch, so the fake pointers stay untouched
    for r in in_scope():
        for name in NULLABLE:
            assert call(r._h, n_stripes=0, **{name: None}) == 0, name
            assert call(r._h, shard_len=0, **{name: None}) == Error.EmptyShard, name
        none = {name: None for name in NULLABLE}
        assert call(r._h, n_stripes=0, **none) == 0
        assert call(r._h, shard_len=0, **none) == Error.EmptyShard


def test_out_of_scope_codecs():
    for r in (R.galois_16.ReedSolomon(250, 10),  # GF(2^16) past 255 shards
              R.galois_8.ReedSolomon(10, 17),    # p > 16
              R.galois_8.ReedSolomon(240, 16),   # k + p = 256: no spare field point
              R.galois_16.ReedSolomon(10, 17), R.galois_16.ReedSolomon(240, 16)):
        assert call(r._h) == INVALID
        # the codec comes before the shard length and the stripe count
        assert call(r._h, shard_len=0) == INVALID
        assert call(r._h, n_stripes=0) == INVALID
        assert call(r._h, n_stripes=1 << 32) == INVALID


def test_empty_shard_then_empty_batch_then_too_many_stripes():
    for r in in_scope():
        assert call(r._h, shard_len=0) == Error.EmptyShard
        assert call(r._h, shard_len=0, n_stripes=0) == Error.EmptyShard
        assert call(r._h, shard_len=0, n_stripes=1 << 32) == Error.EmptyShard
        assert call(r._h, n_stripes=0) == 0  # nothing touched, n_bad neither
        assert call(r._h, n_stripes=1 << 32) == INVALID
        assert call(r._h, n_stripes=(1 << 64) - 1) == INVALID


def test_the_route_key_needs_rse_tune():
    """RSE_OPT_SCRUB_ROUTE is a tuning switch: refused without RSE_TUNE=1 in the
    environment, stored clamped to 0..2 with it; 1 (by the rule) is the default."""
    code = ("import sys; sys.path.insert(0, 'reed-solomon-erasure_amd')\n"
            "from reed_solomon_erasure._lib import load; L = load(); out = []\n"
            f"for v in (0, 2, 5, -3, 1): out += [L.rse_set_option({SCRUB_ROUTE}, v), "
            f"L.rse_get_option({SCRUB_ROUTE})]\n"
            "print(*out)")
    env = dict(os.environ)
    env.pop("RSE_TUNE", None)
    plain = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True,
                           cwd=ROOT)
    assert plain.returncode == 0, plain.stderr[-2000:]
    assert [int(v) for v in plain.stdout.split()] == [INVALID, 1] * 5
    tuned = subprocess.run([sys.executable, "-c", code], env=dict(env, RSE_TUNE="1"),
                           capture_output=True, text=True, cwd=ROOT)
    assert tuned.returncode == 0, tuned.stderr[-2000:]
    assert [int(v) for v in tuned.stdout.split()] == [0, 0, 0, 2, 0, 2, 0, 0, 0, 1]
