"""rse_correct_flat's validation (include/rse_hip.h), through raw ctypes as
tests/test_locate_capi.py does: every refusal happens before any device call,
so fake pointers are never touched and no GPU is needed.  Order, as
rse_locate_flat's: NULL arguments (present, changed and counts may be NULL), a
codec out of scope, an empty shard, zero stripes."""
import reed_solomon_erasure as R
from reed_solomon_erasure import Error
from reed_solomon_erasure._lib import EXPORTS, load

L = load()
FAKE = 0x1000
INVALID = 100  # RSE_ERR_INVALID_ARGUMENT


def call(h, stripes=FAKE, shard_len=16, n_stripes=2, present=FAKE, status=FAKE, changed=FAKE,
         counts=FAKE):
    return L.rse_correct_flat(h, stripes, shard_len, n_stripes, present, status, changed, counts,
                              None)


def test_symbol_is_exported_and_bound():
    assert "rse_correct_flat" in EXPORTS
    assert hasattr(L, "rse_correct_flat")
    assert (R.CORRECT_CLEAN, R.CORRECT_CORRECTED, R.CORRECT_UNCORRECTABLE) == (0, 1, 2)
    assert callable(R.ReedSolomon.correct_flat)


def test_null_arguments():
    r = R.galois_8.ReedSolomon(10, 4)
    assert call(None) == INVALID
    assert call(r._h, stripes=None) == INVALID
    assert call(r._h, status=None) == INVALID
    # NULL comes first: before the empty shard, before the empty batch
    assert call(r._h, stripes=None, shard_len=0) == INVALID
    assert call(r._h, status=None, n_stripes=0) == INVALID
    assert call(r._h, status=None, shard_len=0, n_stripes=0) == INVALID


def test_nullable_arguments_are_not_refused():
    r = R.galois_8.ReedSolomon(10, 4)
    # nothing is launched for an empty batch, so the fake pointers stay untouched
    assert call(r._h, n_stripes=0, present=None) == 0
    assert call(r._h, n_stripes=0, changed=None) == 0
    assert call(r._h, n_stripes=0, counts=None) == 0
    assert call(r._h, n_stripes=0, present=None, changed=None, counts=None) == 0
    assert call(r._h, shard_len=0, present=None, changed=None, counts=None) == Error.EmptyShard


def test_out_of_scope_codecs():
    for r in (R.galois_16.ReedSolomon(10, 4),   # GF(2^16)
              R.galois_8.ReedSolomon(10, 17),   # p > 16
              R.galois_8.ReedSolomon(200, 56)):  # k + p = 256: no spare field point
        assert call(r._h) == INVALID
        # the codec comes before the shard length and the stripe count
        assert call(r._h, shard_len=0) == INVALID
        assert call(r._h, n_stripes=0) == INVALID


def test_empty_shard_then_empty_batch():
    for k, p in ((10, 4), (1, 1), (239, 16)):
        r = R.galois_8.ReedSolomon(k, p)
        assert call(r._h, shard_len=0) == Error.EmptyShard
        assert call(r._h, shard_len=0, n_stripes=0) == Error.EmptyShard
        assert call(r._h, n_stripes=0) == 0  # nothing touched
