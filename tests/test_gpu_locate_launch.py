"""Launch geometry of rse_locate_flat and rse_correct_flat: the loops of their
kernels that the 5-stripe batches of tests/test_gpu_locate.py and
tests/test_gpu_correct.py run exactly once.

Both kernels are launched on loc_grid() (rse_locate_core.hpp):
gridDim.y = min(n_stripes, 65535); gridDim.x = max(4096 / gy, units / 4),
at most 65536 / gy + 1, at least 1, at most units, where a unit is 256 lanes
of 16 bytes (shards on 16-byte boundaries and shard_len % 16 == 0) or of one
byte.  A workgroup walks the stripes blockIdx.y, blockIdx.y + gridDim.y, ...
and in each the units blockIdx.x, blockIdx.x + gridDim.x, ...; the finalize
kernels run min(ceil(n_stripes (k+p) / 256), 65536) blocks of 256 threads
over the (stripe, shard) pairs with a grid-stride loop.

  shape (stripes, codec, shard_len)     units  grid (x, y)  what repeats
  70 000  10+4   16  (vector)             1    (1, 65535)   stripe loop: s, s + 65535
  70 000  10+4    5  (byte-wise)          1    (1, 65535)   the same
  66 000  239+16  1  (byte-wise, MULTI)   1    (1, 65535)   stripe loop; finalize loop:
                                                            66 000 x 255 > 65536 x 256
  2049    10+4   1023 (byte-wise)         4    (1, 2049)    4 units per workgroup
  2049    3+2    8208 (vector)            3    (1, 2049)    3 units, the last with one lane
  2049    129+16  257 (byte-wise, MULTI)  2    (1, 2049)    2 units, the last with one lane
  5       10+4   4096 at base + 1        16    (16, 5)      byte-wise through the base alone
  5       10+4   4096 at base + 16        1    (1, 5)       vector path off a moved base

(2049 stripes: 4096 / 2049 = 1 and units / 4 <= 1.)  The large batches tile a
pool of 8 clean stripes -- random data with the ORACLE's parity -- so that
stripe s is pool[s % 8] before injection.  Expected bytes are those clean
stripes wherever the injection is within a column's capacity 2 nu + f <= p;
flags and counts follow from before -> clean.  Past capacity (one column of
10+4) the brute-force models of tests/locate_model.py and
tests/correct_model.py decide.  The library is never compared with itself,
except where a test's statement is "the same as the full call".

Every stripe of every batch is checked.  Outputs carry one spare row of 0xA5
past the batch, and the batch is followed by a guard stripe.

Untested: saturation of counts at 2^32 - 1.  It needs more than 4 GiB of wrong
bytes in one stripe.
"""

import numpy as np
import pytest
import torch

import reed_solomon_erasure as R
from oracle import oracle as O
from reed_solomon_erasure._lib import load

import correct_model as CM
import locate_model as LM
from test_gpu_correct import correct, expect as expect_corrected
from test_gpu_locate import corrupt_shards, locate

pytestmark = pytest.mark.gpu

LIB = load()
CLEAN, LOCATED, UNCORRECTABLE = 0, 1, 2  # LOCATED is CORRECTED for rse_correct_flat
POOL = 8
GRID_Y = 65535

_POOL = {}


def clean_batch(k, p, length, n_stripes):
    """n_stripes clean stripes, stripe s = pool[s % POOL], and a guard stripe
    of random bytes: (n_stripes + 1, k + p, length), writable.  The pool is
    encoded by the oracle once per shape."""
    n = k + p
    key = (k, p, length)
    if key not in _POOL:
        rng = np.random.default_rng(77000 + 1000 * k + 10 * p + length)
        pool = rng.integers(0, 256, (POOL + 1, n, length), dtype=np.uint8)  # the last: guard
        codec = O.Codec(8, k, p)
        for s in range(POOL):
            codec.encode([pool[s, i] for i in range(n)])
        pool.setflags(write=False)
        _POOL[key] = pool
    pool = _POOL[key]
    buf = np.empty((n_stripes + 1, n, length), np.uint8)
    full = n_stripes // POOL
    buf[:full * POOL].reshape(full, POOL, n, length)[:] = pool[:POOL]
    buf[full * POOL:n_stripes] = pool[:n_stripes - full * POOL]
    buf[n_stripes] = pool[POOL]
    return buf


def erase(buf, present, stripe, shards):
    for q in shards:
        buf[stripe, q] = 0xEE
        present[stripe, q] = 0


def check_corrected(before, result, want, hot, skipped=(), undecodable=None):
    """The whole batch against `want`.  Stripes outside `hot` were clean and
    must report nothing; the hot ones go through tests/test_gpu_correct.py's
    expect(), except `skipped` (more than p erasures: UNCORRECTABLE, untouched,
    counts {0, 0}).  undecodable: {stripe: columns left as they were}."""
    got, status, changed, counts = result
    ns = len(want)
    assert (got == want).all(), np.argwhere((got != want).any(axis=(1, 2)))[:8].ravel().tolist()
    cold = np.ones(ns, bool)
    cold[list(hot)] = False
    assert (before[:ns][cold] == want[cold]).all(), "a stripe outside `hot` was not clean"
    assert not status[cold].any(), np.nonzero(status * cold)[0][:8].tolist()
    assert not changed[cold].any(), np.nonzero(changed.any(axis=1) * cold)[0][:8].tolist()
    assert not counts[cold].any(), np.nonzero(counts.any(axis=1) * cold)[0][:8].tolist()
    for s in skipped:
        assert status[s] == UNCORRECTABLE and not changed[s].any(), (s, int(status[s]))
        assert counts[s].tolist() == [0, 0], (s, counts[s].tolist())
    keep = [s for s in sorted(hot) if s not in skipped]
    bad = [(undecodable or {}).get(s, 0) for s in keep]
    expect_corrected(before[keep], (got[keep], status[keep], changed[keep], counts[keep]),
                     want[keep], undecodable=bad)
    for s, b in (undecodable or {}).items():
        assert counts[s][1] == b, (s, counts[s].tolist())


def check_located(present, status, want):
    """want: {stripe: set of shards (LOCATED) or 'bad'}; every other stripe CLEAN."""
    ns, n = present.shape
    flags = np.ones((ns, n), np.uint8)
    code = np.zeros(ns, np.uint8)
    for s, w in want.items():
        if isinstance(w, str):
            code[s] = UNCORRECTABLE
        elif w:
            code[s] = LOCATED
            flags[s, sorted(w)] = 0
    assert (status == code).all(), [(int(s), int(status[s]), want.get(int(s)))
                                    for s in np.nonzero(status != code)[0][:8]]
    assert (present == flags).all(), np.nonzero((present != flags).any(axis=1))[0][:8].tolist()


def model_verdict(k, p, stripe):
    code, flags = LM.stripe_verdict(k, p, stripe)
    return "bad" if code == UNCORRECTABLE else set(np.nonzero(flags == 0)[0].tolist())


# ---- A1: more than 65535 stripes ----------------------------------------------

def pairs_batch(length):
    """10+4, 70 000 stripes.  Stripes s and s + 65535 share a workgroup: ten
    such pairs, two of each kind (see the tests), everything else clean.
    Returns (clean, corrupted, present, per-kind stripe lists, located sets)."""
    k, p, ns = 10, 4, 70000
    n, t = k + p, p // 2
    rng = np.random.default_rng(41 + length)
    clean = clean_batch(k, p, length, ns)
    buf = clean.copy()
    present = np.ones((ns, n), np.uint8)
    firsts = [0, 7, 501, 1234, 2222, 3000, 3333, 4000, 4400, ns - 1 - GRID_Y]
    info = {"hot": [], "skipped": [], "past": [], "errors": {}, "erased_first": []}
    for i, s in enumerate(firsts):
        s2 = s + GRID_Y
        assert s2 < ns
        info["hot"] += [s, s2]
        perm = [int(q) for q in rng.permutation(n)]
        kind = i % 5
        if kind == 0:    # t wrong shards | clean
            corrupt_shards(buf, rng, s, perm[:t])
            info["errors"][s] = set(perm[:t])
        elif kind == 1:  # one column past capacity | a single wrong byte
            corrupt_shards(buf, rng, s, perm[:t + 1], cols=[length - 1])
            info["past"].append(s)
            corrupt_shards(buf, rng, s2, perm[4:5], cols=[i % length])
            info["errors"][s2] = {perm[4]}
        elif kind == 2:  # p erasures with both end shards | no erasure, t errors elsewhere
            era = [0, n - 1] + [q for q in perm if q not in (0, n - 1)][:p - 2]
            erase(buf, present, s, era)
            info["erased_first"].append(s)
            others = [q for q in perm if q not in era][:t]
            corrupt_shards(buf, rng, s2, others)
            info["errors"][s2] = set(others)
        elif kind == 3:  # p + 1 erasures: skipped | 1 erasure + (p - 1) // 2 errors
            erase(buf, present, s, perm[:p + 1])
            info["skipped"].append(s)
            info["erased_first"].append(s)
            erase(buf, present, s2, perm[p + 1:p + 2])
            more = perm[p + 2:p + 2 + (p - 1) // 2]
            corrupt_shards(buf, rng, s2, more)
            info["errors"][s2] = set(perm[p + 1:p + 2] + more)  # what locate sees: all wrong
        else:            # 3 erasures | 1 erasure at another shard + 1 error
            erase(buf, present, s, perm[:3])
            info["erased_first"].append(s)
            erase(buf, present, s2, perm[3:4])
            corrupt_shards(buf, rng, s2, perm[4:5])
            info["errors"][s2] = set(perm[3:5])
    return clean, buf, present, info


@pytest.mark.parametrize("length", [16, 5])
def test_correct_pairs_of_stripes_65535_apart(length):
    """What a workgroup keeps in LDS from stripe s must not reach stripe
    s + 65535: changed mask and byte count (first of the pair: t wrong shards;
    second: clean), undecodable count (a column past capacity; a single wrong
    byte), erasure mask, count and Gamma (p erasures; none, t errors), the
    skip path (p + 1 erasures; 1 erasure + (p - 1) // 2 errors), the tail of
    the erasure list (3 erasures; 1 other erasure + 1 error)."""
    k, p = 10, 4
    clean, buf, present, info = pairs_batch(length)
    ns = len(present)
    want = clean[:ns]
    undecodable = {}
    for s in info["skipped"]:
        want[s] = buf[s]
    for s in info["past"]:  # one column with t + 1 wrong shards: the model decides
        code, col, bad = CM.correct_stripe(k, p, buf[s], [])
        assert code == UNCORRECTABLE and bad == 1, "seed: the column must be undecodable"
        want[s] = col
        undecodable[s] = 1
    result = correct(R.galois_8.ReedSolomon(k, p), buf, length, present, n_stripes=ns)
    check_corrected(buf, result, want, info["hot"], info["skipped"], undecodable)
    status, counts = result[1], result[3]
    for s in info["past"]:
        assert status[s + GRID_Y] == LOCATED and counts[s + GRID_Y].tolist() == [1, 0]


@pytest.mark.parametrize("length", [16, 5])
def test_locate_pairs_of_stripes_65535_apart(length):
    """The same batch without present flags: erased (0xEE) shards are plain
    corruption now.  At most t wrong shards are located exactly; the firsts
    with 3, 4 and 5 wrong shards are past t and follow the brute-force model."""
    k, p = 10, 4
    clean, buf, _, info = pairs_batch(length)
    ns = len(buf) - 1
    want = dict(info["errors"])
    for s in info["past"]:
        assert model_verdict(k, p, buf[s]) == "bad", "seed: the column must be undecodable"
        want[s] = "bad"
    for s in info["erased_first"]:
        want[s] = model_verdict(k, p, buf[s])
    present, status = locate(R.galois_8.ReedSolomon(k, p), buf, length, n_stripes=ns)
    check_located(present, status, want)
    for s in info["hot"]:  # spelled out: nothing of the first reaches the second
        if s < GRID_Y:
            assert status[s] != CLEAN
            if s + GRID_Y not in info["errors"]:
                assert status[s + GRID_Y] == CLEAN and present[s + GRID_Y].all()
            else:
                assert status[s + GRID_Y] == LOCATED
                assert present[s + GRID_Y].sum() == k + p - len(info["errors"][s + GRID_Y])


# ---- A2: more than 2^24 (stripe, shard) pairs ---------------------------------

def wide_batch():
    """239+16, shard_len 1, 66 000 stripes: corrupted and erased stripes at the
    start and in the last 200 (past pair 2^24 of the finalize kernels; second
    stripes of their workgroups).  Returns (clean, errors only, errors and
    erasures, present, hot stripes, {stripe: error shards}, skipped)."""
    k, p, ns = 239, 16, 66000
    n = k + p
    assert ns * n > 65536 * 256 and (ns - 200) * n > 65536 * 256
    rng = np.random.default_rng(43)
    clean = clean_batch(k, p, 1, ns)
    err = clean.copy()
    hot = [0, 1, 2, 255, 464, 465] + list(range(ns - 200, ns))
    present = np.ones((ns, n), np.uint8)
    errors, erased, skipped = {}, {}, []
    for j, s in enumerate(hot):
        perm = [int(q) for q in rng.permutation(n)]
        kind, step = j % 4, j // 4
        if kind == 0:    # 1 .. t errors, the end shards among them now and then
            nu, f = 1 + step % 8, 0
            if step % 3 == 0:
                perm = [n - 1, 0] + [q for q in perm if q not in (0, n - 1)]
        elif kind == 1:  # f erasures and as many errors as still fit
            f = 1 + step % 16
            nu = (p - f) // 2
        elif kind == 2:  # p erasures with both end shards
            nu, f = 0, p
            perm = [0, n - 1] + [q for q in perm if q not in (0, n - 1)]
        else:            # p + 1 erasures: skipped
            nu, f = 0, p + 1
            skipped.append(s)
        erased[s] = perm[:f]
        errors[s] = set(perm[f:f + nu])
        corrupt_shards(err, rng, s, perm[f:f + nu])
    full = err.copy()
    for s, era in erased.items():
        erase(full, present, s, era)
    return clean, err, full, present, hot, errors, skipped


def test_more_than_2_to_24_stripe_shard_pairs():
    k, p = 239, 16
    clean, err, full, flags, hot, errors, skipped = wide_batch()
    ns = len(flags)
    r = R.galois_8.ReedSolomon(k, p)
    present, status = locate(r, err, 1, n_stripes=ns)
    check_located(present, status, {s: e for s, e in errors.items() if e})
    with_errors = [s for s in hot if errors[s]]
    check_corrected(err, correct(r, err, 1, n_stripes=ns), clean[:ns], with_errors)
    want = clean[:ns].copy()
    for s in skipped:
        want[s] = full[s]
    check_corrected(full, correct(r, full, 1, flags, n_stripes=ns), want, hot, skipped)


# ---- A3: several units per workgroup ------------------------------------------

UNIT_SHAPES = [(10, 4, 1023, 256, 4), (3, 2, 8208, 4096, 3), (129, 16, 257, 256, 2)]


def units_batch(k, p, length, unit_bytes, units):
    """2049 stripes, a dozen of them with wrong bytes in every unit of the
    stripe: byte 0, one byte inside every further unit, the last valid byte.
    129+16: the first unit's wrong bytes fill lanes 0 .. 63, one wave of four,
    so the table rebuild for the second unit meets waves that decoded and waves
    that did not.  Every column has 1 .. t wrong shards out of p of the stripe."""
    ns = 2049
    n, t = k + p, p // 2
    assert (length + unit_bytes - 1) // unit_bytes == units
    rng = np.random.default_rng(47 + k)
    clean = clean_batch(k, p, length, ns)
    buf = clean.copy()
    located = {}
    for i, s in enumerate(np.linspace(0, ns - 1, 12).astype(int).tolist()):
        cols = list(range(64)) if k > 128 else [0]
        cols += [u * unit_bytes + (37 * i + 11 * u) % min(unit_bytes, length - u * unit_bytes)
                 for u in range(1, units)]
        cols = sorted(set(cols + [length - 1]))
        assert all(any(c // unit_bytes == u for c in cols) for u in range(units))
        pool = [int(q) for q in rng.permutation(n)[:p]]
        if i % 2:  # both ends of the point shift; the last shard is the last byte's alone
            pool = [0] + [q for q in pool if q not in (0, n - 1)][:p - 2] + [n - 1]
        used = set()
        for j, c in enumerate(cols):
            # the last valid byte's shard is wrong nowhere else: locate names it
            # only if the last unit was swept
            shards = [pool[(j + q) % (p - 1)] for q in range(1 + j % t)]
            if c == length - 1:
                shards[0] = pool[p - 1]
            corrupt_shards(buf, rng, s, shards, cols=[c])
            used.update(shards)
        assert pool[p - 1] in used and len(used) <= p
        located[s] = used
    return clean, buf, located


@pytest.mark.parametrize("k,p,length,unit_bytes,units", UNIT_SHAPES)
def test_correct_several_units_per_workgroup(k, p, length, unit_bytes, units):
    clean, buf, located = units_batch(k, p, length, unit_bytes, units)
    ns = len(buf) - 1
    result = correct(R.galois_8.ReedSolomon(k, p), buf, length, n_stripes=ns)
    check_corrected(buf, result, clean[:ns], list(located))
    for s, used in located.items():  # a dropped or twice-counted unit shows here
        assert result[3][s][0] == (buf[s] != clean[s]).sum()
        assert set(np.nonzero(result[2][s])[0].tolist()) == used


@pytest.mark.parametrize("k,p,length,unit_bytes,units", UNIT_SHAPES)
def test_locate_several_units_per_workgroup(k, p, length, unit_bytes, units):
    _, buf, located = units_batch(k, p, length, unit_bytes, units)
    ns = len(buf) - 1
    present, status = locate(R.galois_8.ReedSolomon(k, p), buf, length, n_stripes=ns)
    check_located(present, status, located)


# ---- A4: base alignment -------------------------------------------------------

PAD = 256
NS = 5


def aligned_batch():
    k, p, length = 10, 4, 4096
    rng = np.random.default_rng(53)
    clean = clean_batch(k, p, length, NS)
    buf = clean.copy()
    corrupt_shards(buf, rng, 0, [3, 13])
    for q, c in zip((0, 13, 5, 9), (0, 15, 16, 4095)):
        corrupt_shards(buf, rng, 1, [q], cols=[c])
    corrupt_shards(buf, rng, 3, [1])
    for q, c in zip((7, 2, 12, 4), (0, 15, 16, 4095)):
        corrupt_shards(buf, rng, 3, [q], cols=[c])
    return clean, buf, {0: {3, 13}, 1: {0, 13, 5, 9}, 3: {1, 7, 2, 12, 4}}


def run_at_offset(r, host, length, off, entry):
    """The batch (NS stripes and a guard) at byte PAD + off of a 0xA5-filled
    device buffer, through the C entry; returns (stripes, outputs...) after
    checking the bytes around the batch and the spare rows."""
    n = r.total_shard_count()
    raw = torch.full((PAD + off + host.size + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    assert raw.data_ptr() % 256 == 0
    lo, hi = PAD + off, PAD + off + host.size
    raw[lo:hi] = torch.from_numpy(host.reshape(-1)).cuda()
    status = torch.full((NS + 1,), 0xA5, dtype=torch.uint8, device="cuda")
    flags = torch.full((NS + 1, n), 0xA5, dtype=torch.uint8, device="cuda")
    counts = torch.full((NS + 1, 2), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    if entry == "locate":
        rc = LIB.rse_locate_flat(r._h, raw.data_ptr() + lo, length, NS, flags.data_ptr(),
                                 status.data_ptr(), stream)
    else:
        rc = LIB.rse_correct_flat(r._h, raw.data_ptr() + lo, length, NS, None, status.data_ptr(),
                                  flags.data_ptr(), counts.data_ptr(), stream)
    assert rc == 0
    torch.cuda.synchronize()
    raw = raw.cpu().numpy()
    assert (raw[:lo] == 0xA5).all() and (raw[hi:] == 0xA5).all(), "bytes around the batch"
    got = raw[lo:hi].reshape(host.shape)
    assert (got[NS] == host[NS]).all(), "guard stripe"
    status, flags = status.cpu().numpy(), flags.cpu().numpy()
    counts = counts.cpu().numpy().view(np.uint32)
    assert status[NS] == 0xA5 and (flags[NS] == 0xA5).all()
    if entry == "locate":
        assert (got == host).all(), "the call only reads"
        assert (counts == 0xA5A5A5A5).all()
    else:
        assert (counts[NS] == 0xA5A5A5A5).all()
    return got[:NS], status[:NS], flags[:NS], counts[:NS]


@pytest.mark.parametrize("off", [1, 16])
def test_base_alignment(off):
    """Shards that start at odd addresses through the base alone (shard_len is
    a multiple of 16: the byte-wise path), and a base moved by 16 (still the
    vector path): the same results as at offset 0, the expected ones."""
    k, p, length = 10, 4, 4096
    clean, buf, located = aligned_batch()
    r = R.galois_8.ReedSolomon(k, p)
    for at in (0, off):
        _, status, present, _ = run_at_offset(r, buf, length, at, "locate")
        want = {s: (w if len(w) <= p else "bad") for s, w in located.items()}
        check_located(present, status, want)
        result = run_at_offset(r, buf, length, at, "correct")
        check_corrected(buf, result, clean[:NS], list(located))
        for s, used in located.items():
            assert set(np.nonzero(result[2][s])[0].tolist()) == used


# ---- A5: nullable outputs -----------------------------------------------------

@pytest.mark.parametrize("length", [17, 4096 + 16])
def test_changed_and_counts_may_be_null(length):
    k, p = 10, 4
    n, t = k + p, p // 2
    rng = np.random.default_rng(59)
    clean = clean_batch(k, p, length, NS)
    buf = clean.copy()
    corrupt_shards(buf, rng, 0, [0, n - 1])
    corrupt_shards(buf, rng, 1, [4], cols=[length - 1])
    corrupt_shards(buf, rng, 3, [int(q) for q in rng.permutation(n)[:t + 1]])  # past capacity
    r = R.galois_8.ReedSolomon(k, p)
    full = correct(r, buf, length)
    for s in (0, 1, 2, 4):
        assert (full[0][s] == clean[s]).all()
    assert full[1].tolist() == [LOCATED, LOCATED, CLEAN, UNCORRECTABLE, CLEAN]
    for no_changed, no_counts in ((True, False), (False, True), (True, True)):
        dev = torch.from_numpy(buf.copy()).cuda()
        status = torch.full((NS + 1,), 0xA5, dtype=torch.uint8, device="cuda")
        changed = torch.full((NS + 1, n), 0xA5, dtype=torch.uint8, device="cuda")
        counts = torch.full((NS + 1, 2), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32,
                            device="cuda")
        rc = LIB.rse_correct_flat(r._h, dev.data_ptr(), length, NS, None, status.data_ptr(),
                                  None if no_changed else changed.data_ptr(),
                                  None if no_counts else counts.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        got = dev.cpu().numpy()
        assert (got[:NS] == full[0]).all() and (got[NS] == buf[NS]).all()
        status, changed = status.cpu().numpy(), changed.cpu().numpy()
        counts = counts.cpu().numpy().view(np.uint32)
        assert (status[:NS] == full[1]).all() and status[NS] == 0xA5
        # an output that was not passed is not written through another's pointer
        assert (changed == 0xA5).all() if no_changed else (
            (changed[:NS] == full[2]).all() and (changed[NS] == 0xA5).all())
        assert (counts == 0xA5A5A5A5).all() if no_counts else (
            (counts[:NS] == full[3]).all() and (counts[NS] == 0xA5A5A5A5).all())
