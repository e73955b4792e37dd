"""rse_read_flat's validation (include/rse_hip.h), through raw ctypes as
tests/test_update_capi.py does: every refusal happens before any device call,
so fake pointers are never touched and no GPU is needed.  Order: NULL codec /
stripes / reads / out / status / result (`present` may be NULL), a codec out of
scope (p > 128, GF(2^16) past 256 shards), an empty shard, an empty list
(RSE_OK, nothing touched), then zero stripes and the 2^32 - 1 limits on
n_stripes and n_reads."""
import re
import os

import reed_solomon_erasure as R
from reed_solomon_erasure import Error
from reed_solomon_erasure._lib import EXPORTS, load

L = load()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000
INVALID = 100  # RSE_ERR_INVALID_ARGUMENT
POINTERS = ("stripes", "reads", "out", "status", "result")


def call(h, stripes=FAKE, shard_len=16, n_stripes=2, present=FAKE, reads=FAKE, n_reads=3,
         out=FAKE, status=FAKE, result=FAKE):
    return L.rse_read_flat(h, stripes, shard_len, n_stripes, present, reads, n_reads, out, status,
                           result, None)


def in_scope():
    return [R.galois_8.ReedSolomon(10, 4), R.galois_8.ReedSolomon(1, 1),
            R.galois_8.ReedSolomon(4, 20), R.galois_8.ReedSolomon(128, 128),
            R.galois_8.ReedSolomon(240, 16), R.galois_16.ReedSolomon(10, 4),
            R.galois_16.ReedSolomon(100, 28), R.galois_16.ReedSolomon(128, 128)]


def out_of_scope():
    return [R.galois_8.ReedSolomon(4, 200), R.galois_16.ReedSolomon(300, 20),
            R.galois_8.ReedSolomon(127, 129), R.galois_16.ReedSolomon(250, 7)]


def test_symbol_is_exported_and_bound():
    assert "rse_read_flat" in EXPORTS
    assert hasattr(L, "rse_read_flat")
    assert callable(R.galois_8.ReedSolomon.read_flat)
    assert callable(R.galois_16.ReedSolomon.read_flat)
    assert (R.READ_SERVED, R.READ_REJECTED) == (0, 1)
    assert (R.READ_COPIED, R.READ_REBUILT, R.READ_LOST) == (0, 1, 2)


def test_header_declares_the_entry_and_its_verdicts():
    with open(os.path.join(ROOT, "include", "rse_hip.h")) as f:
        text = f.read()
    for name, value in (("SERVED", 0), ("REJECTED", 1), ("COPIED", 0), ("REBUILT", 1), ("LOST", 2)):
        assert re.search(r"#define RSE_READ_%s %d\b" % (name, value), text), name
    assert re.search(r"\bint rse_read_flat\(const rse_codec \*codec, const void \*stripes, "
                     r"size_t shard_len, size_t n_stripes,", text)


def test_null_arguments():
    r = R.galois_8.ReedSolomon(10, 4)
    assert call(None) == INVALID
    for name in POINTERS:
        assert call(r._h, **{name: None}) == INVALID, name
        # NULL wins over every later check: the empty shard, the empty list, the
        # empty batch, the batch and the list too large
        assert call(r._h, shard_len=0, **{name: None}) == INVALID, name
        assert call(r._h, n_reads=0, **{name: None}) == INVALID, name
        assert call(r._h, n_stripes=0, **{name: None}) == INVALID, name
        assert call(r._h, n_stripes=1 << 32, **{name: None}) == INVALID, name
        assert call(r._h, n_reads=1 << 32, **{name: None}) == INVALID, name
        assert call(r._h, shard_len=0, n_reads=0, n_stripes=0, **{name: None}) == INVALID, name
    assert call(None, shard_len=0, n_reads=0) == INVALID
    # ... and over the codec's scope
    far = out_of_scope()[0]
    for name in POINTERS:
        assert call(far._h, **{name: None}) == INVALID, name


def test_present_may_be_null():
    r = R.galois_8.ReedSolomon(10, 4)
    # no refusal for it: the later checks answer
    assert call(r._h, present=None, shard_len=0) == Error.EmptyShard
    assert call(r._h, present=None, n_reads=0) == 0
    assert call(r._h, present=None, n_stripes=0) == INVALID


def test_out_of_scope_codecs():
    for r in out_of_scope():
        assert call(r._h) == INVALID
        # the codec comes before the shard length, the list and the stripe count
        assert call(r._h, shard_len=0) == INVALID
        assert call(r._h, n_reads=0) == INVALID
        assert call(r._h, shard_len=0, n_reads=0) == INVALID
        assert call(r._h, n_stripes=0) == INVALID


def test_empty_shard_then_empty_list_then_the_limits():
    for r in in_scope():
        assert call(r._h, shard_len=0) == Error.EmptyShard
        assert call(r._h, shard_len=0, n_reads=0) == Error.EmptyShard
        assert call(r._h, shard_len=0, n_stripes=0) == Error.EmptyShard
        assert call(r._h, shard_len=0, n_stripes=1 << 32, n_reads=1 << 32) == Error.EmptyShard
        # an empty list: RSE_OK with the fake pointers untouched, before the stripe count
        assert call(r._h, n_reads=0) == 0
        assert call(r._h, n_reads=0, n_stripes=0) == 0
        assert call(r._h, n_reads=0, n_stripes=1 << 32) == 0
        assert call(r._h, n_stripes=0) == INVALID
        assert call(r._h, n_stripes=1 << 32) == INVALID
        assert call(r._h, n_stripes=(1 << 64) - 1) == INVALID
        assert call(r._h, n_reads=1 << 32) == INVALID
        assert call(r._h, n_reads=(1 << 64) - 1) == INVALID
