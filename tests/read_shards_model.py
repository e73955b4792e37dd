"""What rse_read_shards must hand out, from tests/read_model.py (and so from
the ORACLE alone): the shards are cut into blocks as include/rse_hip.h says,
the in-order verdict is read_model.first_offender with n_blocks for n_stripes,
and entry {b, r} is read_model.expected on block b alone -- a one-stripe flat
arrangement of that block's length -- under flag row b with the flags of the
shards that have no buffer cleared.

Shards are a uint8 array of shape (k + p, bytes per shard); a GF(2^16) shard is
its 2 x len bytes.  A shard without a buffer still has a row here (the bytes it
would hold): the model never looks at it, as its flag is 0.
"""
import numpy as np

import read_model as RM

SERVED, REJECTED = RM.SERVED, RM.REJECTED
COPIED, REBUILT, LOST = RM.COPIED, RM.REBUILT, RM.LOST


def cut(length, block_len):
    """(B, n_blocks) in elements for shards of `length` elements."""
    b = length if block_len == 0 or block_len > length else block_len
    return b, -(-length // b)


def block_flags(k, p, present, block, null=()):
    """Flag row `block` (all ones for present = None) with the NULL shards'
    flags cleared."""
    flags = np.ones(k + p, np.uint8) if present is None else np.array(present[block], np.uint8)
    flags[list(null)] = 0
    return flags


def expected(field, k, p, shards, block_len, present, reads, null=()):
    """(rows, status, result) of a call.  rows[u] is the bytes entry u writes at
    the start of its row of B x esize bytes -- as many as its block has -- or
    None where the row is not written; status[u] its class; result the two
    words.  A rejected list: every row None, status None."""
    esize = field // 8
    length = shards.shape[1] // esize
    b, n_blocks = cut(length, block_len)
    bad = RM.first_offender(reads, n_blocks, k + p)
    if bad is not None:
        return [None] * len(reads), None, [REJECTED, bad]
    rows, status = [None] * len(reads), [None] * len(reads)
    for block in sorted({int(blk) for blk, _ in reads}):
        lo, hi = block * b * esize, min((block + 1) * b, length) * esize
        one = np.ascontiguousarray(shards[None, :, lo:hi])
        flags = block_flags(k, p, present, block, null)
        mine = [u for u, (blk, _) in enumerate(reads) if int(blk) == block]
        r, s, res = RM.expected(field, k, p, one, flags[None],
                                [(0, int(reads[u][1])) for u in mine], 1)
        assert res[0] == SERVED
        for u, row, cls in zip(mine, r, s):
            rows[u], status[u] = row, cls
    return rows, status, [SERVED, status.count(LOST)]


def encode(field, k, p, shards):
    """Parity of the shards written by the oracle, in place."""
    RM.encode(field, k, p, shards[None], 1)
    return shards
