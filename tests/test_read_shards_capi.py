"""rse_read_shards' validation (include/rse_hip.h), through raw ctypes as
tests/test_update_shards_capi.py does: every refusal here happens before any
device call, so fake pointers are never touched and no GPU is needed.  Order:
NULL codec / shards / lens / reads / out / status / result (`present` may be
NULL); a codec out of scope; the shard count; the lengths; an empty list
(RSE_OK, nothing touched, `result` neither); more than 2^32 - 1 blocks or
entries.  A NULL shards[i] is NOT refused: it declares a shard without a
buffer.  Each refusal is reached with everything after it wrong as well."""
import ctypes
import os
import re

import reed_solomon_erasure as R
from reed_solomon_erasure import Error
from reed_solomon_erasure._lib import EXPORTS, load

L = load()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000
INVALID = 100  # RSE_ERR_INVALID_ARGUMENT
POINTERS = ("reads", "out", "status", "result")
DEFAULT = object()
FILL32 = 0xA5A5A5A5


def call(r, n=None, ptrs=DEFAULT, lens=DEFAULT, length=16, block_len=4, present=FAKE, reads=FAKE,
         n_reads=3, out=FAKE, status=FAKE, result=FAKE, null_at=(), lens_at=None):
    """n shards (default k + p) of `length` elements at fake addresses; null_at:
    those shards[i] are NULL; lens_at: (i, value) replaces one length."""
    total = r.total_shard_count() if r is not None else 14
    n = total if n is None else n
    if ptrs is DEFAULT:
        vals = [FAKE + 0x100 * i for i in range(n)]
        for i in null_at:
            vals[i] = None
        ptrs = (ctypes.c_void_p * max(1, n))(*vals)
    if lens is DEFAULT:
        vals = [length] * n
        if lens_at is not None:
            vals[lens_at[0]] = lens_at[1]
        lens = (ctypes.c_size_t * max(1, n))(*vals)
    return L.rse_read_shards(r._h if r is not None else None, ptrs, lens, n, block_len, present,
                             reads, n_reads, out, status, result, None)


def in_scope():
    return [R.galois_8.ReedSolomon(10, 4), R.galois_8.ReedSolomon(1, 1),
            R.galois_8.ReedSolomon(4, 20), R.galois_8.ReedSolomon(128, 128),
            R.galois_8.ReedSolomon(240, 16), R.galois_16.ReedSolomon(10, 4),
            R.galois_16.ReedSolomon(100, 28), R.galois_16.ReedSolomon(128, 128)]


def out_of_scope():
    return [R.galois_8.ReedSolomon(4, 200), R.galois_16.ReedSolomon(300, 20),
            R.galois_8.ReedSolomon(127, 129), R.galois_16.ReedSolomon(250, 7)]


def test_symbol_is_exported_and_bound():
    assert "rse_read_shards" in EXPORTS
    assert hasattr(L, "rse_read_shards")
    assert callable(R.galois_8.ReedSolomon.read)
    assert callable(R.galois_16.ReedSolomon.read)


def test_header_declares_the_entry_and_points_at_it():
    with open(os.path.join(ROOT, "include", "rse_hip.h")) as f:
        text = f.read()
    assert re.search(r"\bint rse_read_shards\(const rse_codec \*codec, const void \*const \*shards, "
                     r"const size_t \*lens,\s+size_t n_shards, size_t block_len,", text)
    flat = text[text.index("/* Degraded reads:"):text.index("int rse_read_flat(")]
    scope = flat[flat.index("Out of scope:"):]
    scope = scope[:scope.index(".") + 1]  # the out-of-scope sentence
    assert "host memory" in scope and "separately allocated" not in scope
    assert "rse_read_shards" in flat
    shards = text[text.index("/* rse_update_flat for shards"):text.index("int rse_update_shards(")]
    assert "rse_read_shards" in shards


def test_null_arguments_come_first():
    r = R.galois_8.ReedSolomon(10, 4)
    far = out_of_scope()[0]
    assert call(None) == INVALID
    nulls = [dict(ptrs=None), dict(lens=None)] + [{name: None} for name in POINTERS]
    for kw in nulls:
        assert call(r, **kw) == INVALID, kw
        # ... before the codec's scope, the count, the lengths, the empty list
        # and the limits
        assert call(far, n=3, length=0, **kw) == INVALID, kw
        assert call(r, n=13, **kw) == INVALID, kw
        assert call(r, n=15, length=0, **kw) == INVALID, kw
        if "ptrs" not in kw and "lens" not in kw:
            assert call(r, lens_at=(5, 3), null_at=(2,), **kw) == INVALID, kw
        assert call(r, n_reads=0, **kw) == INVALID, kw
        assert call(r, n_reads=1 << 32, **kw) == INVALID, kw
        assert call(r, length=1 << 33, block_len=1, n_reads=0, **kw) == INVALID, kw
    assert call(None, n=13, length=0, n_reads=0) == INVALID


def test_present_may_be_null():
    r = R.galois_8.ReedSolomon(10, 4)
    # no refusal for it: the later checks answer
    assert call(r, present=None, lens_at=(0, 0)) == Error.EmptyShard
    assert call(r, present=None, n_reads=0) == 0
    assert call(r, present=None, n_reads=1 << 32) == INVALID


def test_out_of_scope_codecs():
    for r in out_of_scope():
        n = r.total_shard_count()
        assert call(r) == INVALID
        # the codec comes before the count, the lengths and the empty list
        assert call(r, n=n - 1) == INVALID
        assert call(r, n=n + 1, length=0) == INVALID
        assert call(r, length=0) == INVALID
        assert call(r, lens_at=(1, 3)) == INVALID
        assert call(r, n_reads=0) == INVALID
        assert call(r, n=n - 1, lens_at=(0, 0), null_at=(0,), block_len=1, n_reads=0) == INVALID


def test_shard_count_then_lengths():
    r = R.galois_8.ReedSolomon(10, 4)
    # 13 and 15 shards for 10+4, with everything later wrong as well
    for kw in (dict(), dict(length=0), dict(lens_at=(3, 5)), dict(null_at=(0,)), dict(n_reads=0),
               dict(length=1 << 33, block_len=1), dict(n_reads=1 << 32),
               dict(length=0, null_at=(1,), n_reads=0)):
        assert call(r, n=13, **kw) == Error.TooFewShards, kw
        assert call(r, n=15, **kw) == Error.TooManyShards, kw
    for r in in_scope():
        n = r.total_shard_count()
        assert call(r, n=n - 1, length=0) == Error.TooFewShards
        assert call(r, n=n + 1, length=0) == Error.TooManyShards
        # a zero first length, one unequal length: before the empty list and the
        # limits, and whether or not that shard has a buffer
        assert call(r, lens_at=(0, 0)) == Error.EmptyShard
        assert call(r, lens_at=(0, 0), null_at=(0,), n_reads=0) == Error.EmptyShard
        assert call(r, length=0, null_at=(n - 1,), block_len=1, n_reads=1 << 32) == Error.EmptyShard
        assert call(r, lens_at=(n - 1, 15)) == Error.IncorrectShardSize
        assert call(r, lens_at=(n - 1, 15), null_at=(n - 1,)) == Error.IncorrectShardSize
        assert call(r, lens_at=(n - 1, 0), n_reads=0) == Error.IncorrectShardSize
        assert call(r, length=1 << 33, block_len=1, lens_at=(n // 2, 7), null_at=(0,),
                    n_reads=1 << 32) == Error.IncorrectShardSize


def test_a_null_shard_is_not_refused():
    """The checks after the lengths answer as if the pointer were there: the
    empty list is RSE_OK, the limits are the limits -- for one NULL shard, for p
    of them, and for every one of them."""
    for r in in_scope():
        n, p = r.total_shard_count(), r.parity_shard_count()
        for null_at in ((0,), (n // 2,), (n - 1,), tuple(range(p)), tuple(range(n))):
            assert call(r, null_at=null_at, n_reads=0) == 0, null_at
            assert call(r, null_at=null_at, n_reads=0, present=None) == 0, null_at
            assert call(r, null_at=null_at, n_reads=0, length=1 << 33, block_len=1) == 0, null_at
            assert call(r, null_at=null_at, length=1 << 33, block_len=1) == INVALID, null_at
            assert call(r, null_at=null_at, n_reads=1 << 32) == INVALID, null_at


def test_empty_list_then_the_limits():
    for r in in_scope():
        # an empty list: RSE_OK with the fake pointers untouched, before the block count
        assert call(r, n_reads=0) == 0
        assert call(r, n_reads=0, block_len=0) == 0
        assert call(r, n_reads=0, length=1 << 33, block_len=1) == 0
        # 2^33 and 2^32 blocks; 2^32 - 1 passes the block count (and fails the list's)
        assert call(r, length=1 << 33, block_len=1) == INVALID
        assert call(r, length=1 << 33, block_len=2) == INVALID
        assert call(r, length=(1 << 33) + 1, block_len=2) == INVALID
        assert call(r, length=(1 << 32) - 1, block_len=1, n_reads=1 << 32) == INVALID
        assert call(r, n_reads=1 << 32) == INVALID
        assert call(r, n_reads=(1 << 64) - 1) == INVALID
        assert call(r, n_reads=1 << 32, block_len=0) == INVALID


def test_an_empty_list_leaves_result_alone():
    """`result` in host memory here: the call must return before it reads or
    writes any of its pointers."""
    r = R.galois_8.ReedSolomon(10, 4)
    result = (ctypes.c_uint32 * 2)(FILL32, FILL32)
    assert call(r, n_reads=0, result=ctypes.addressof(result)) == 0
    assert call(r, n_reads=0, result=ctypes.addressof(result), null_at=(3,)) == 0
    assert list(result) == [FILL32, FILL32]
