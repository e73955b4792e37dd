"""rse_scrub_shards' validation (include/rse_hip.h), through raw ctypes as
tests/test_scrub_capi.py does: every refusal happens before any device call, so
fake pointers are never touched and no GPU is needed.  Order: NULL codec /
shards / lens / status (present, changed, counts, bad_blocks and n_bad may be
NULL); a codec out of scope; the shard count; the lengths; a NULL shards[i];
more than 2^32 - 1 blocks.  Each refusal is reached with everything after it
wrong as well."""
import ctypes

import reed_solomon_erasure as R
from reed_solomon_erasure import Error
from reed_solomon_erasure._lib import EXPORTS, load

L = load()
FAKE = 0x1000
INVALID = 100  # RSE_ERR_INVALID_ARGUMENT
NULLABLE = ("present", "changed", "counts", "bad_blocks", "n_bad")
DEFAULT = object()


def call(r, n=None, ptrs=DEFAULT, lens=DEFAULT, length=16, block_len=4, present=FAKE, status=FAKE,
         changed=FAKE, counts=FAKE, bad_blocks=FAKE, n_bad=FAKE, null_at=None, lens_at=None):
    """n shards (default k + p) of `length` elements at fake addresses; null_at:
    that shards[i] is NULL; lens_at: (i, value) replaces one length."""
    total = r.total_shard_count() if r is not None else 14
    n = total if n is None else n
    if ptrs is DEFAULT:
        vals = [FAKE + 0x100 * i for i in range(n)]
        if null_at is not None:
            vals[null_at] = None
        ptrs = (ctypes.c_void_p * max(1, n))(*vals)
    if lens is DEFAULT:
        vals = [length] * n
        if lens_at is not None:
            vals[lens_at[0]] = lens_at[1]
        lens = (ctypes.c_size_t * max(1, n))(*vals)
    return L.rse_scrub_shards(r._h if r is not None else None, ptrs, lens, n, block_len, present,
                              status, changed, counts, bad_blocks, n_bad, None)


def in_scope():
    return [R.galois_8.ReedSolomon(10, 4), R.galois_8.ReedSolomon(1, 1),
            R.galois_8.ReedSolomon(239, 16), R.galois_16.ReedSolomon(10, 4),
            R.galois_16.ReedSolomon(20, 8)]


def out_of_scope():
    return [R.galois_16.ReedSolomon(250, 10),  # GF(2^16) past 255 shards
            R.galois_8.ReedSolomon(10, 17),    # p > 16
            R.galois_8.ReedSolomon(240, 16),   # k + p = 256: no spare field point
            R.galois_16.ReedSolomon(10, 17), R.galois_16.ReedSolomon(240, 16)]


def test_symbol_is_exported_and_bound():
    assert "rse_scrub_shards" in EXPORTS
    assert hasattr(L, "rse_scrub_shards")
    assert callable(R.galois_8.ReedSolomon.scrub)
    assert callable(R.galois_16.ReedSolomon.scrub)


def test_null_arguments_come_first():
    r = R.galois_8.ReedSolomon(10, 4)
    bad = R.galois_8.ReedSolomon(10, 17)
    assert call(None) == INVALID
    assert call(r, ptrs=None) == INVALID
    assert call(r, lens=None) == INVALID
    assert call(r, status=None) == INVALID
    # ... before the codec's scope, the count, the lengths, a NULL shard and the block count
    for kw in (dict(ptrs=None), dict(lens=None), dict(status=None)):
        assert call(bad, n=3, length=0, **kw) == INVALID
        assert call(r, n=13, **kw) == INVALID
        assert call(r, n=15, length=0, **kw) == INVALID
        assert call(r, lens_at=(5, 3), null_at=2, **kw) == INVALID
    assert call(None, n=13, length=1 << 33, block_len=1) == INVALID


def test_out_of_scope_codecs():
    for r in out_of_scope():
        n = r.total_shard_count()
        assert call(r) == INVALID
        # the codec comes before the count, the lengths, a NULL shard and the block count
        assert call(r, n=n - 1) == INVALID
        assert call(r, n=n + 1, length=0) == INVALID
        assert call(r, length=0) == INVALID
        assert call(r, lens_at=(1, 3)) == INVALID
        assert call(r, n=n - 1, lens_at=(0, 0), null_at=0, block_len=1) == INVALID


def test_shard_count_then_lengths_then_null_shard_then_block_count():
    r = R.galois_8.ReedSolomon(10, 4)
    # 13 and 15 shards for 10+4, with everything later wrong as well
    for kw in (dict(), dict(length=0), dict(lens_at=(3, 5)), dict(null_at=0),
               dict(length=1 << 33, block_len=1), dict(length=0, null_at=1)):
        assert call(r, n=13, **kw) == Error.TooFewShards, kw
        assert call(r, n=15, **kw) == Error.TooManyShards, kw
    for r in in_scope():
        n = r.total_shard_count()
        assert call(r, n=n - 1, length=0) == Error.TooFewShards
        assert call(r, n=n + 1, length=0) == Error.TooManyShards
        # a zero first length, one unequal length; before a NULL shard and the block count
        assert call(r, lens_at=(0, 0)) == Error.EmptyShard
        assert call(r, lens_at=(0, 0), null_at=0) == Error.EmptyShard
        assert call(r, length=0, null_at=n - 1, block_len=1) == Error.EmptyShard
        assert call(r, lens_at=(n - 1, 15)) == Error.IncorrectShardSize
        assert call(r, lens_at=(n - 1, 0)) == Error.IncorrectShardSize
        assert call(r, length=1 << 33, block_len=1, lens_at=(n // 2, 7),
                    null_at=0) == Error.IncorrectShardSize
        # a NULL shards[i], before the block count
        for i in (0, n // 2, n - 1):
            assert call(r, null_at=i) == INVALID
            assert call(r, null_at=i, length=1 << 33, block_len=1) == INVALID
        # 2^33 blocks
        assert call(r, length=1 << 33, block_len=1) == INVALID
        assert call(r, length=1 << 33, block_len=2) == INVALID  # 2^32 blocks
        assert call(r, length=(1 << 33) + 1, block_len=2) == INVALID


def test_nullable_arguments_and_block_len_0_or_past_the_length_are_not_refused():
    """Nothing may reach a device here, so acceptance is shown on an input that
    is refused at the last step of the order, the NULL shard: everything before
    it -- the nullable arguments among it -- was accepted.  The block count
    comes after that step, and block_len = 0 (one block) and block_len > len
    (one block) pass where block_len = 1 gives too many blocks."""
    for r in in_scope():
        n = r.total_shard_count()
        none = {name: None for name in NULLABLE}
        for kw in [{name: None} for name in NULLABLE] + [none]:
            assert call(r, null_at=n - 1, **kw) == INVALID, kw
            assert call(r, lens_at=(n - 1, 3), **kw) == Error.IncorrectShardSize, kw
            assert call(r, length=0, **kw) == Error.EmptyShard, kw
        # the same huge shards: refused for their block count at block_len 1 ...
        assert call(r, length=1 << 33, block_len=1, **none) == INVALID
        # ... and at block_len 0 or past the length only for what comes before it
        for block_len in (0, (1 << 33) + 1, (1 << 64) - 1):
            assert call(r, length=1 << 33, block_len=block_len,
                        lens_at=(n - 1, 1)) == Error.IncorrectShardSize
            assert call(r, length=1 << 33, block_len=block_len, null_at=n - 1) == INVALID
