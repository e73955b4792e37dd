"""What rse_update_flat must leave behind, from the ORACLE alone (never from
the library): the in-order rule of include/rse_hip.h in a few lines of Python,
and the expected bytes -- the named data shards replaced, and for every touched
stripe

    expected parity = parity before ^ parity(O.Codec.encode of a stripe whose
                      data is old ^ new at the updated shards and zero elsewhere)

which is the delta identity of a linear code: the stripe's syndrome (stored
parity ^ re-encoded parity) is what it was, consistent stripe or not.

Stripes are uint8 arrays of shape (n_stripes, k + p, bytes per shard); a
GF(2^16) shard is its 2 x shard_len bytes.
"""
import numpy as np

from oracle import oracle as O

APPLIED, REJECTED = 0, 1


def first_offender(updates, n_stripes, k):
    """Index of the first entry that is not in order, or None."""
    prev = None
    for u, (stripe, shard) in enumerate(updates):
        cur = (int(stripe), int(shard))
        if cur[0] >= n_stripes or cur[1] >= k or (prev is not None and not prev < cur):
            return u
        prev = cur
    return None


def expected_result(updates, n_stripes, k):
    """The two words of `result`."""
    bad = first_offender(updates, n_stripes, k)
    if bad is not None:
        return [REJECTED, bad]
    return [APPLIED, len({int(s) for s, _ in updates})]


def apply(field, k, p, before, updates, new_data, n_stripes=None):
    """The stripes after the call.  before: (stripes, k + p, bytes), of which
    the first n_stripes (default: all) are the call's -- the rest must keep
    their bytes; new_data: (n_updates, bytes).  A rejected list leaves `before`
    as it is."""
    n_stripes = before.shape[0] if n_stripes is None else n_stripes
    after = np.array(before)
    if first_offender(updates, n_stripes, k) is not None:
        return after
    oracle = O.Codec.shared(field, k, p)
    nbytes = before.shape[2]
    by_stripe = {}
    for u, (stripe, shard) in enumerate(updates):
        by_stripe.setdefault(int(stripe), []).append((int(shard), u))
    for stripe, entries in by_stripe.items():
        delta = [np.zeros(nbytes, np.uint8) for _ in range(k + p)]
        for shard, u in entries:
            delta[shard] = np.ascontiguousarray(before[stripe, shard] ^ new_data[u])
            after[stripe, shard] = new_data[u]
        oracle.encode(delta)
        for j in range(p):
            after[stripe, k + j] = before[stripe, k + j] ^ delta[k + j]
    return after


def encode(field, k, p, stripes, n):
    """Parity of the first n stripes written by the oracle, in place."""
    oracle = O.Codec.shared(field, k, p)
    for s in range(n):
        shards = [np.ascontiguousarray(stripes[s, i]) for i in range(k + p)]
        oracle.encode(shards)
        for j in range(p):
            stripes[s, k + j] = shards[k + j]
    return stripes
