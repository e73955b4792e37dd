"""What rse_update_shards must leave behind, from tests/update_model.py (and
so from the ORACLE alone): the shards are cut into blocks as include/rse_hip.h
says, and block b's bytes after the call are update_model.apply on block b alone
-- a one-stripe flat arrangement of that block's length -- with block b's
entries in order and the first bytes of their rows of new_data.

Shards are a uint8 array of shape (k + p, bytes per shard); a GF(2^16) shard is
its 2 x len bytes, and `esize` is the element size in bytes.
"""
import numpy as np

import update_model as UM

APPLIED, REJECTED = UM.APPLIED, UM.REJECTED


def cut(length, block_len):
    """(B, n_blocks) in elements for shards of `length` elements."""
    b = length if block_len == 0 or block_len > length else block_len
    return b, -(-length // b)


def expected_result(updates, length, block_len, k):
    """The two words of `result`: update_model's with n_blocks for n_stripes."""
    return UM.expected_result(updates, cut(length, block_len)[1], k)


def apply(field, k, p, before, block_len, updates, new_data):
    """The shards after the call.  before: (k + p, bytes); new_data:
    (n_updates, B x esize), of which an entry for the shorter last block uses the
    first bytes.  A rejected list leaves `before` as it is."""
    esize = field // 8
    length = before.shape[1] // esize
    b, n_blocks = cut(length, block_len)
    after = np.array(before)
    if UM.first_offender(updates, n_blocks, k) is not None:
        return after
    assert new_data.shape == (len(updates), b * esize)
    for block in sorted({int(blk) for blk, _ in updates}):
        lo, hi = block * b * esize, min((block + 1) * b, length) * esize
        mine = [u for u, (blk, _) in enumerate(updates) if int(blk) == block]
        one = UM.apply(field, k, p, np.ascontiguousarray(before[None, :, lo:hi]),
                       [(0, int(updates[u][1])) for u in mine],
                       np.ascontiguousarray(new_data[mine, :hi - lo]), 1)
        after[:, lo:hi] = one[0]
    return after


def encode(field, k, p, shards):
    """Parity of the shards written by the oracle, in place."""
    UM.encode(field, k, p, shards[None], 1)
    return shards
