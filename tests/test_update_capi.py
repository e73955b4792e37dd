"""rse_update_flat's validation (include/rse_hip.h), through raw ctypes as
tests/test_scrub_capi.py does: every refusal happens before any device call,
so fake pointers are never touched and no GPU is needed.  Order: NULL codec /
stripes / updates / new_data / result, a codec out of scope (GF(2^16) past 256
shards), an empty shard, an empty list (RSE_OK, nothing touched), then zero
stripes and the 2^32 - 1 limits on n_stripes and n_updates."""
import re
import os

import reed_solomon_erasure as R
from reed_solomon_erasure import Error
from reed_solomon_erasure._lib import EXPORTS, load

L = load()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000
INVALID = 100  # RSE_ERR_INVALID_ARGUMENT
POINTERS = ("stripes", "updates", "new_data", "result")


def call(h, stripes=FAKE, shard_len=16, n_stripes=2, updates=FAKE, new_data=FAKE, n_updates=3,
         result=FAKE):
    return L.rse_update_flat(h, stripes, shard_len, n_stripes, updates, new_data, n_updates,
                             result, None)


def in_scope():
    return [R.galois_8.ReedSolomon(10, 4), R.galois_8.ReedSolomon(1, 1),
            R.galois_8.ReedSolomon(4, 20), R.galois_8.ReedSolomon(128, 128),
            R.galois_8.ReedSolomon(240, 16), R.galois_16.ReedSolomon(10, 4),
            R.galois_16.ReedSolomon(20, 8), R.galois_16.ReedSolomon(128, 128)]


def out_of_scope():
    return [R.galois_16.ReedSolomon(300, 20), R.galois_16.ReedSolomon(250, 7)]


def test_symbol_is_exported_and_bound():
    assert "rse_update_flat" in EXPORTS
    assert hasattr(L, "rse_update_flat")
    assert callable(R.galois_8.ReedSolomon.update_flat)
    assert callable(R.galois_16.ReedSolomon.update_flat)
    assert (R.UPDATE_APPLIED, R.UPDATE_REJECTED) == (0, 1)


def test_header_declares_the_entry_and_its_verdicts():
    with open(os.path.join(ROOT, "include", "rse_hip.h")) as f:
        text = f.read()
    assert re.search(r"#define RSE_UPDATE_APPLIED 0\b", text)
    assert re.search(r"#define RSE_UPDATE_REJECTED 1\b", text)
    assert re.search(r"\bint rse_update_flat\(const rse_codec \*codec, void \*stripes, "
                     r"size_t shard_len, size_t n_stripes,", text)


def test_null_arguments():
    r = R.galois_8.ReedSolomon(10, 4)
    assert call(None) == INVALID
    for name in POINTERS:
        assert call(r._h, **{name: None}) == INVALID, name
        # NULL wins over every later check: the empty shard, the empty list, the
        # empty batch, the batch and the list too large
        assert call(r._h, shard_len=0, **{name: None}) == INVALID, name
        assert call(r._h, n_updates=0, **{name: None}) == INVALID, name
        assert call(r._h, n_stripes=0, **{name: None}) == INVALID, name
        assert call(r._h, n_stripes=1 << 32, **{name: None}) == INVALID, name
        assert call(r._h, n_updates=1 << 32, **{name: None}) == INVALID, name
        assert call(r._h, shard_len=0, n_updates=0, n_stripes=0, **{name: None}) == INVALID, name
    assert call(None, shard_len=0, n_updates=0) == INVALID
    # ... and over the codec's scope
    far = out_of_scope()[0]
    for name in POINTERS:
        assert call(far._h, **{name: None}) == INVALID, name


def test_out_of_scope_codecs():
    for r in out_of_scope():
        assert call(r._h) == INVALID
        # the codec comes before the shard length, the list and the stripe count
        assert call(r._h, shard_len=0) == INVALID
        assert call(r._h, n_updates=0) == INVALID
        assert call(r._h, shard_len=0, n_updates=0) == INVALID
        assert call(r._h, n_stripes=0) == INVALID


def test_empty_shard_then_empty_list_then_the_limits():
    for r in in_scope():
        assert call(r._h, shard_len=0) == Error.EmptyShard
        assert call(r._h, shard_len=0, n_updates=0) == Error.EmptyShard
        assert call(r._h, shard_len=0, n_stripes=0) == Error.EmptyShard
        assert call(r._h, shard_len=0, n_stripes=1 << 32, n_updates=1 << 32) == Error.EmptyShard
        # an empty list: RSE_OK with the fake pointers untouched, before the stripe count
        assert call(r._h, n_updates=0) == 0
        assert call(r._h, n_updates=0, n_stripes=0) == 0
        assert call(r._h, n_updates=0, n_stripes=1 << 32) == 0
        assert call(r._h, n_stripes=0) == INVALID
        assert call(r._h, n_stripes=1 << 32) == INVALID
        assert call(r._h, n_stripes=(1 << 64) - 1) == INVALID
        assert call(r._h, n_updates=1 << 32) == INVALID
        assert call(r._h, n_updates=(1 << 64) - 1) == INVALID
