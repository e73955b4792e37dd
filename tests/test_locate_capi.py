"""rse_locate_flat's validation (include/rse_hip.h), through raw ctypes as
tests/test_capi.py does: every refusal happens before any device call, so fake
pointers are never touched and no GPU is needed.  Order: NULL arguments, a
codec out of scope, an empty shard, zero stripes."""
import ctypes

import reed_solomon_erasure as R
from reed_solomon_erasure import Error
from reed_solomon_erasure._lib import EXPORTS, load

L = load()
FAKE = 0x1000
INVALID = 100  # RSE_ERR_INVALID_ARGUMENT


def test_symbol_is_exported_and_bound():
    assert "rse_locate_flat" in EXPORTS
    assert hasattr(L, "rse_locate_flat")
    assert (R.LOCATE_CLEAN, R.LOCATE_LOCATED, R.LOCATE_UNCORRECTABLE) == (0, 1, 2)
    assert callable(R.ReedSolomon.locate_flat)


def test_null_arguments():
    r = R.galois_8.ReedSolomon(10, 4)
    assert L.rse_locate_flat(None, FAKE, 16, 2, FAKE, FAKE, None) == INVALID
    assert L.rse_locate_flat(r._h, None, 16, 2, FAKE, FAKE, None) == INVALID
    assert L.rse_locate_flat(r._h, FAKE, 16, 2, None, FAKE, None) == INVALID
    assert L.rse_locate_flat(r._h, FAKE, 16, 2, FAKE, None, None) == INVALID
    # NULL comes first: before the empty shard, before the empty batch
    assert L.rse_locate_flat(r._h, None, 0, 2, FAKE, FAKE, None) == INVALID
    assert L.rse_locate_flat(r._h, FAKE, 16, 0, FAKE, None, None) == INVALID


def test_out_of_scope_codecs():
    for r in (R.galois_16.ReedSolomon(10, 4),   # GF(2^16)
              R.galois_8.ReedSolomon(10, 17),   # p > 16
              R.galois_8.ReedSolomon(200, 56)):  # k + p = 256: no spare field point
        assert L.rse_locate_flat(r._h, FAKE, 16, 2, FAKE, FAKE, None) == INVALID
        # the codec comes before the shard length and the stripe count
        assert L.rse_locate_flat(r._h, FAKE, 0, 2, FAKE, FAKE, None) == INVALID
        assert L.rse_locate_flat(r._h, FAKE, 16, 0, FAKE, FAKE, None) == INVALID


def test_empty_shard_then_empty_batch():
    for k, p in ((10, 4), (1, 1), (239, 16)):
        r = R.galois_8.ReedSolomon(k, p)
        assert L.rse_locate_flat(r._h, FAKE, 0, 2, FAKE, FAKE, None) == Error.EmptyShard
        assert L.rse_locate_flat(r._h, FAKE, 0, 0, FAKE, FAKE, None) == Error.EmptyShard
        assert L.rse_locate_flat(r._h, FAKE, 16, 0, FAKE, FAKE, None) == 0  # nothing touched
