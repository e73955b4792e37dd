"""What rse_read_flat must hand out, from the ORACLE alone (never from the
library): the in-order rule of include/rse_hip.h in a few lines of Python, and
per touched stripe

    O.Codec.reconstruct(a copy of the stripe with the erased shards zeroed,
                        the stripe's flag row)

of which the wanted shards are taken.  The oracle raising TooFewShardsPresent
means LOST for that stripe's erased entries; a present entry is the stripe's
own bytes.  The oracle's reconstruct rebuilds from the first k present shards
in index order (core.rs:801-841), which is the contract's choice of inputs, so
the model is right on stripes that are not codewords too.

Stripes are uint8 arrays of shape (n_stripes, k + p, bytes per shard); a
GF(2^16) shard is its 2 x shard_len bytes.
"""
import numpy as np

from oracle import oracle as O

SERVED, REJECTED = 0, 1
COPIED, REBUILT, LOST = 0, 1, 2
TOO_FEW_SHARDS_PRESENT = 10


def first_offender(reads, n_stripes, total):
    """Index of the first entry that is not in order, or None."""
    prev = None
    for u, (stripe, shard) in enumerate(reads):
        cur = (int(stripe), int(shard))
        if cur[0] >= n_stripes or cur[1] >= total or (prev is not None and not prev < cur):
            return u
        prev = cur
    return None


def rebuilt_stripe(field, k, p, stripe, flags):
    """The stripe after the oracle's reconstruct for that flag row (the erased
    shards' own bytes are never looked at), or None: too few shards present."""
    shards = [np.ascontiguousarray(stripe[i]) if flags[i] else np.zeros_like(stripe[i])
              for i in range(k + p)]
    try:
        O.Codec.shared(field, k, p).reconstruct(shards, [bool(f) for f in flags])
    except O.OracleError as err:
        assert err.code == TOO_FEW_SHARDS_PRESENT
        return None
    return shards


def expected(field, k, p, stripes, present, reads, n_stripes):
    """(rows, status, result) of a call: rows[u] is entry u's bytes or None
    where the row is not written; status[u] its class; result the two words.  A
    rejected list: every row None, status None."""
    total = k + p
    bad = first_offender(reads, n_stripes, total)
    if bad is not None:
        return [None] * len(reads), None, [REJECTED, bad]
    rows, status = [], []
    cache = {}
    for stripe, shard in reads:
        stripe, shard = int(stripe), int(shard)
        flags = [1] * total if present is None else [int(f) for f in present[stripe]]
        if flags[shard]:
            rows.append(np.array(stripes[stripe, shard]))
            status.append(COPIED)
            continue
        if stripe not in cache:
            cache[stripe] = rebuilt_stripe(field, k, p, stripes[stripe], flags)
        if cache[stripe] is None:
            rows.append(None)
            status.append(LOST)
        else:
            rows.append(np.array(cache[stripe][shard]))
            status.append(REBUILT)
    return rows, status, [SERVED, status.count(LOST)]


def encode(field, k, p, stripes, n):
    """Parity of the first n stripes written by the oracle, in place."""
    oracle = O.Codec.shared(field, k, p)
    for s in range(n):
        shards = [np.ascontiguousarray(stripes[s, i]) for i in range(k + p)]
        oracle.encode(shards)
        for j in range(p):
            stripes[s, k + j] = shards[k + j]
    return stripes
