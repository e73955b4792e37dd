"""rse_scrub_shards on the GPU: rse_scrub_flat for separately allocated shards,
with a verdict per block of columns.

Every case runs on both routes, forced with RSE_OPT_SCRUB_ROUTE (0 direct, 2
pre-filter), and rse_last_kernel() must name the route.  Expected bytes are the
ORACLE's clean shards wherever the injection is within a column's capacity
2 nu + f <= p (every byte column is its own codeword, so the oracle's encode of
whole shards is the encode of every block); past it the damaged block is held
to the definition (tests/test_gpu_scrub.py check_definition).  In addition,
never alone: the entry's defining property.  The blocks are gathered into the
flat layout -- the full blocks as one batch of stripes, the shorter last block
as a batch of one, since rse_scrub_flat treats every stripe of a batch on its
own -- and rse_scrub_flat on the same route must leave the same bytes, status,
changed, counts and list.

Buffers: every shard is its own allocation with 64 guard bytes of 0xA5 before
and after its bytes, which must survive; status, changed and counts carry a
spare row of 0xA5; bad_blocks is filled with 0xA5 and keeps it from n_bad on.
A GF(2^16) shard is handled as its bytes: 2 x len per shard.

What each test is aimed at: the block offset missing from the
parity pointers -- test_all_clean and test_errors on every shape with more than
one block; a store at the flat address -- test_errors and
test_damage_in_one_block_of_one_shard (bytes, guards, changed); the last
block's verdict word or accumulator slot off by one, and a work list made of
the full blocks only -- test_damage_lands_in_its_row; the vector path with an
unaligned pointer -- test_alignment (and tests/test_scrub_shards_plan.py).
"""

import ctypes

import numpy as np
import pytest
import torch

import reed_solomon_erasure as R
from reed_solomon_erasure._lib import load

from test_gpu_correct import erase
from test_gpu_locate import NS, corrupt_shards, disjoint_columns, reference
from test_gpu_scrub import check_definition, clean_stripes

pytestmark = pytest.mark.gpu

LIB = load()
CLEAN, CORRECTED, UNCORRECTABLE = 0, 1, 2
SCRUB_ROUTE = 56  # RSE_OPT_SCRUB_ROUTE
ROUTES = [(0, "direct"), (2, "prefilter")]
FILL32 = 0xA5A5A5A5
GUARD = 64

# (field, k, p, len, block_len) in elements
SHAPES = [
    (8, 10, 4, 17, 0),                      # one block, byte-wise
    (8, 10, 4, 5 * 1024, 1024),             # the 1 KiB sub-chunk check
    (8, 10, 4, 5 * 4096 + 37, 4096),        # vector blocks, then a 37-byte last block
    (8, 10, 4, 5 * (4096 + 16), 4096 + 16),
    (8, 10, 4, 5 * 48 + 5, 48),             # fewer vectors than lanes
    (8, 10, 4, 5 * 50, 50),                 # aligned pointers, byte-wise because of B
    (8, 10, 4, 16384 + 4096 + 48, 0),       # one block: 16 KiB + 4 KiB chunks, a table tail
    (8, 20, 8, 2 * 1024 + 5, 1024),         # NO = 8
    (8, 100, 16, 2 * (4096 + 16) + 40, 4096 + 16),  # 116 pointers, the check cut into chunks
    (8, 239, 16, 64, 32),                   # MULTI
    (8, 16, 16, 2 * 2048 + 24, 2048),       # the FFT check
    (8, 12, 4, 4096 + 19, 4096),            # a run-time codec: its module may not be built
    (16, 20, 8, 2048 + 8, 1024), (16, 10, 4, 2048 + 8, 1024),
    (16, 20, 8, 9, 4), (16, 10, 4, 9, 4),
]
CASES = [pytest.param(*shape, *route, id="gf%d-%d+%d-%d-%d-%s" % (*shape, route[1]))
         for shape in SHAPES for route in ROUTES]


def codec(field, k, p):
    return (R.galois_16 if field == 16 else R.galois_8).ReedSolomon(k, p)


def clean_shards(field, k, p, elems):
    """The k + p clean shards as bytes, (k + p, bytes per shard), parity by the
    ORACLE: the first stripe of the shared references; never modified."""
    return reference(k, p, elems)[0] if field == 8 else clean_stripes(field, k, p, elems)[0]


def blocks_of(field, elems, block_len):
    """[(first byte, end byte)] of every block."""
    es = field // 8
    b = min(block_len or elems, elems)
    return [(lo * es, min(lo + b, elems) * es) for lo in range(0, elems, b)]


def stripe_of(arr, blk):
    """Block `blk` of the shards (k + p, bytes) as a batch of one stripe: a view."""
    return arr[None, :, blk[0]:blk[1]]


def gather(arr, blocks):
    """The blocks in the flat layout: (full blocks, k + p, B), and the shorter
    last block (1, k + p, its bytes) or None."""
    bb = blocks[0][1] - blocks[0][0]
    nf = sum(1 for lo, hi in blocks if hi - lo == bb)
    full = np.ascontiguousarray(arr[:, :nf * bb].reshape(arr.shape[0], nf, bb).transpose(1, 0, 2))
    tail = np.ascontiguousarray(arr[None, :, nf * bb:]) if nf < len(blocks) else None
    return full, tail


def outputs(rows, n):
    return (torch.full((rows + 1,), 0xA5, dtype=torch.uint8, device="cuda"),
            torch.full((rows + 1, n), 0xA5, dtype=torch.uint8, device="cuda"),
            torch.full((rows + 1, 2), FILL32 - (1 << 32), dtype=torch.int32, device="cuda"),
            torch.full((rows + 1,), FILL32 - (1 << 32), dtype=torch.int32, device="cuda"),
            torch.full((2,), FILL32 - (1 << 32), dtype=torch.int32, device="cuda"))


def fetch(outs, rows):
    """(status, changed, counts, list) of the batch after checking the spare
    rows and the list against status."""
    status, changed = outs[0].cpu().numpy(), outs[1].cpu().numpy()
    counts = outs[2].cpu().numpy().view(np.uint32)
    bad, n_bad = outs[3].cpu().numpy().view(np.uint32), outs[4].cpu().numpy().view(np.uint32)
    assert status[rows] == 0xA5 and (changed[rows] == 0xA5).all()
    assert (counts[rows] == FILL32).all() and n_bad[1] == FILL32
    listed = np.nonzero(status[:rows])[0]
    assert n_bad[0] == len(listed), (int(n_bad[0]), listed[:8].tolist())
    assert (bad[:len(listed)] == listed).all()
    assert (bad[len(listed):] == FILL32).all(), "entries from n_bad on are not written"
    return status[:rows], changed[:rows], counts[:rows], listed


def flat_scrub(r, elems, flat, present, stream):
    """rse_scrub_flat (the route is the caller's) on a batch in the flat layout."""
    ns, n = flat.shape[0], flat.shape[1]
    with torch.cuda.stream(stream):
        dev = torch.from_numpy(np.array(flat)).cuda()
        outs = outputs(ns, n)
        pres = torch.from_numpy(np.ascontiguousarray(present)).cuda() if present is not None else None
    rc = LIB.rse_scrub_flat(r._h, dev.data_ptr(), elems, ns, pres.data_ptr() if pres is not None
                            else None, *[t.data_ptr() for t in outs], stream.cuda_stream)
    assert rc == 0
    stream.synchronize()
    return (dev.cpu().numpy(),) + fetch(outs, ns)


def separate(host, offsets):
    """Every shard in an allocation of its own: guard, `offsets[i]` spare bytes,
    the shard, guard.  Returns (allocations, the shards as views of them)."""
    allocs, views = [], []
    for row, off in zip(host, offsets):
        a = torch.full((GUARD + off + len(row) + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        v = a[GUARD + off:GUARD + off + len(row)]
        v.copy_(torch.from_numpy(np.array(row)))
        allocs.append(a)
        views.append(v)
    return allocs, views


def two_tensors(host, k):
    """Data as the rows of one [k, L] tensor, parity as the rows of a separate
    [p, L] tensor, each between guards."""
    allocs, views = [], []
    for part in (host[:k], host[k:]):
        rows, length = part.shape
        a = torch.full((GUARD + rows * length + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        t = a[GUARD:GUARD + rows * length].view(rows, length)
        t.copy_(torch.from_numpy(np.array(part)))
        allocs.append(a)
        views += [t[i] for i in range(rows)]
    return allocs, views


def guards_kept(allocs, views):
    for a in allocs:
        h = a.cpu().numpy()
        inner = [(v.data_ptr() - a.data_ptr(), v.numel()) for v in views
                 if a.data_ptr() <= v.data_ptr() < a.data_ptr() + a.numel()]
        keep = np.ones(len(h), bool)
        for lo, cnt in inner:
            keep[lo:lo + cnt] = False
        assert keep[:GUARD].all() and keep[-GUARD:].all()
        assert (h[keep] == 0xA5).all(), "bytes around a shard were written"


def scrub(field, k, p, elems, block_len, route, host, present=None, offsets=None, layout=separate):
    """rse_scrub_shards through the C entry on a copy of `host` (k + p, bytes)
    in HBM on the forced route (route[0] 1: by the rule); checks the route's
    name, the guards, the spare rows, the list, and everything against
    rse_scrub_flat on the gathered blocks.  Returns (shards, status, changed,
    counts)."""
    r = codec(field, k, p)
    n = k + p
    blocks = blocks_of(field, elems, block_len)
    nb = len(blocks)
    stream = torch.cuda.current_stream()
    with torch.cuda.stream(stream):
        if layout is separate:
            allocs, views = separate(host, offsets or [0] * n)
        else:
            allocs, views = layout(host, k)
        outs = outputs(nb, n)
        pres = None
        if present is not None:
            pres = torch.from_numpy(np.ascontiguousarray(present, dtype=np.uint8)).cuda()
            assert tuple(pres.shape) == (nb, n)
    ptrs = (ctypes.c_void_p * n)(*[v.data_ptr() for v in views])
    lens = (ctypes.c_size_t * n)(*[elems] * n)
    old = LIB.rse_get_option(SCRUB_ROUTE)
    assert LIB.rse_set_option(SCRUB_ROUTE, route[0]) == 0
    try:
        rc = LIB.rse_scrub_shards(r._h, ptrs, lens, n, block_len,
                                  pres.data_ptr() if pres is not None else None,
                                  *[t.data_ptr() for t in outs], stream.cuda_stream)
        assert rc == 0
        assert R.core.last_kernel() == "scrub-shards gf%d %d+%d %s" % (field, k, p, route[1])
        stream.synchronize()
        got = np.stack([v.cpu().numpy() for v in views])
        guards_kept(allocs, views)
        status, changed, counts, listed = fetch(outs, nb)
        if pres is not None:
            assert (pres.cpu().numpy() == np.asarray(present, np.uint8)).all(), "present is only read"
        # in addition: rse_scrub_flat on the gathered blocks, the same route
        full, tail = gather(np.asarray(host), blocks)
        gfull, gtail = gather(got, blocks)
        nf = full.shape[0]
        parts = [(full, gfull, 0, nf, (blocks[0][1] - blocks[0][0]) * 8 // field)]
        if tail is not None:
            parts.append((tail, gtail, nf, nb, (blocks[-1][1] - blocks[-1][0]) * 8 // field))
        want_list = []
        for flat, after, lo, hi, blen in parts:
            fb, fs, fc, fn, fl = flat_scrub(r, blen, flat, None if present is None
                                            else np.asarray(present, np.uint8)[lo:hi], stream)
            assert (fb == after).all(), "bytes as rse_scrub_flat leaves them"
            assert (fs == status[lo:hi]).all() and (fc == changed[lo:hi]).all()
            assert (fn == counts[lo:hi]).all()
            want_list += (fl + lo).tolist()
        assert want_list == listed.tolist()
    finally:
        LIB.rse_set_option(SCRUB_ROUTE, old)
    return got, status, changed, counts


def definition(k, p, before, result, blocks, b, erased=None):
    """Block b against the definition of tests/test_gpu_scrub.py."""
    got, status, changed, counts = result
    lo, hi = blocks[b]
    check_definition(k, p, [before[:, lo:hi]],
                     ([got[:, lo:hi]], status[b:b + 1], changed[b:b + 1], counts[b:b + 1]),
                     [erased] if erased is not None else None)


@pytest.mark.parametrize("field,k,p,elems,block_len,route,name", CASES)
def test_all_clean(field, k, p, elems, block_len, route, name):
    ref = clean_shards(field, k, p, elems)
    got, status, changed, counts = scrub(field, k, p, elems, block_len, (route, name), ref)
    assert (got == ref).all()
    assert len(status) == len(blocks_of(field, elems, block_len))
    assert not status.any() and not changed.any() and not counts.any()


@pytest.mark.parametrize("field,k,p,elems,block_len,route,name", CASES)
def test_errors(field, k, p, elems, block_len, route, name):
    """Every block: disjoint sets of at most t wrong shards in different
    columns, up to p + 1 shards between them, another choice per block."""
    t = p // 2
    rng = np.random.default_rng(71)
    ref = clean_shards(field, k, p, elems)
    buf = ref.copy()
    blocks = blocks_of(field, elems, block_len)
    sizes = []
    for blk in blocks:
        width = blk[1] - blk[0]
        size = min(p + 1, t * min(-(-(p + 1) // t), width))
        sets, cols = disjoint_columns(k, p, width, rng, size)
        for shards, col in zip(sets, cols):
            corrupt_shards(stripe_of(buf, blk), rng, 0, shards, cols=[col])
        sizes.append(size)
    result = scrub(field, k, p, elems, block_len, (route, name), buf)
    got, status, changed, counts = result
    assert (got == ref).all(), "repaired shards equal the oracle's encode"
    assert (status == CORRECTED).all()
    assert counts[:, 0].tolist() == sizes and not counts[:, 1].any()
    assert changed.sum(axis=1).tolist() == sizes
    for b in range(len(blocks)):
        definition(k, p, buf, result, blocks, b)


@pytest.mark.parametrize("field,k,p,elems,block_len,route,name", CASES)
def test_erasures(field, k, p, elems, block_len, route, name):
    """By block b % 5.  0: p erasures alone.  1: p - 2 erasures beside a wholly
    wrong shard.  2: p + 1 erasures (not touched).  3: erased flags on a block
    whose bytes already are a codeword: CLEAN, not listed.  4: p + 1 erased
    flags on such a block: it passes the check, and is UNCORRECTABLE, untouched
    and listed all the same."""
    n = k + p
    rng = np.random.default_rng(73)
    ref = clean_shards(field, k, p, elems)
    buf = ref.copy()
    blocks = blocks_of(field, elems, block_len)
    present = np.ones((len(blocks), n), np.uint8)
    for b, blk in enumerate(blocks):
        view, row = stripe_of(buf, blk), present[b:b + 1]
        perm = [int(q) for q in rng.permutation(n)]
        if b % 5 == 0:
            erase(view, row, 0, perm[:p])
        elif b % 5 == 1:
            erase(view, row, 0, perm[:p - 2])
            corrupt_shards(view, rng, 0, perm[p - 2:p - 1])
        elif b % 5 == 2:
            erase(view, row, 0, perm[:p + 1])
        elif b % 5 == 3:
            present[b, perm[:2]] = 0
        else:
            present[b, perm[:p + 1]] = 0
    result = scrub(field, k, p, elems, block_len, (route, name), buf, present)
    got, status, changed, counts = result
    want = [CORRECTED, CORRECTED, UNCORRECTABLE, CLEAN, UNCORRECTABLE]
    assert status.tolist() == [want[b % 5] for b in range(len(blocks))]
    for b, (lo, hi) in enumerate(blocks):
        definition(k, p, buf, result, blocks, b, np.nonzero(present[b] == 0)[0].tolist())
        if b % 5 == 2:
            assert (got[:, lo:hi] == buf[:, lo:hi]).all()
        else:
            assert (got[:, lo:hi] == ref[:, lo:hi]).all(), (b, "the oracle's encode")
    assert changed[0].sum() == p


@pytest.mark.parametrize("field,k,p,elems,block_len,route,name", CASES)
def test_past_capacity_in_one_block(field, k, p, elems, block_len, route, name):
    """t + 1 wholly wrong shards in the middle block, one wrong byte in every
    other block."""
    n, t = k + p, p // 2
    rng = np.random.default_rng(79)
    ref = clean_shards(field, k, p, elems)
    buf = ref.copy()
    blocks = blocks_of(field, elems, block_len)
    mid = len(blocks) // 2
    for b, blk in enumerate(blocks):
        if b == mid:
            corrupt_shards(stripe_of(buf, blk), rng, 0, [int(q) for q in rng.permutation(n)[:t + 1]])
        else:
            corrupt_shards(stripe_of(buf, blk), rng, 0, [b % n], cols=[blk[1] - blk[0] - 1])
    result = scrub(field, k, p, elems, block_len, (route, name), buf)
    got, status, changed, counts = result
    for b, (lo, hi) in enumerate(blocks):
        definition(k, p, buf, result, blocks, b)
        if b != mid:
            assert (got[:, lo:hi] == ref[:, lo:hi]).all() and status[b] == CORRECTED
            assert counts[b].tolist() == [1, 0] and np.nonzero(changed[b])[0].tolist() == [b % n]
    assert status[mid] == UNCORRECTABLE


ADDR = (8, 10, 4, 5 * 4096 + 37, 4096)  # blocks 0 .. 4 full, block 5 of 37 bytes


@pytest.mark.parametrize("route,name", ROUTES)
@pytest.mark.parametrize("where", [4, 5], ids=["last-full", "tail"])
def test_damage_lands_in_its_row(where, route, name):
    rng = np.random.default_rng(83)
    ref = clean_shards(*ADDR[:4])
    buf = ref.copy()
    blocks = blocks_of(8, ADDR[3], ADDR[4])
    width = blocks[where][1] - blocks[where][0]
    corrupt_shards(stripe_of(buf, blocks[where]), rng, 0, [3], cols=[0, width - 1])
    corrupt_shards(stripe_of(buf, blocks[where]), rng, 0, [12], cols=[width // 2])
    got, status, changed, counts = scrub(*ADDR, (route, name), buf)
    assert (got == ref).all()
    want = [CLEAN] * 6
    want[where] = CORRECTED
    assert status.tolist() == want
    assert counts[where].tolist() == [3, 0] and counts.sum() == 3
    assert np.nonzero(changed[where])[0].tolist() == [3, 12] and changed.sum() == 2


@pytest.mark.parametrize("route,name", ROUTES)
def test_damage_in_one_block_of_one_shard(route, name):
    """Block 1 of shard 0 wholly wrong: block 1 of every other shard and block
    0 of shard 0 are not written."""
    rng = np.random.default_rng(89)
    ref = clean_shards(*ADDR[:4])
    buf = ref.copy()
    buf[0, 4096:8192] ^= rng.integers(1, 256, 4096, dtype=np.uint8)
    got, status, changed, counts = scrub(*ADDR, (route, name), buf)
    assert (got == ref).all()
    assert status.tolist() == [CLEAN, CORRECTED, CLEAN, CLEAN, CLEAN, CLEAN]
    assert changed[1].tolist() == [1] + [0] * 13 and changed.sum() == 1
    assert counts[1].tolist() == [4096, 0]


ALIGNED = (8, 10, 4, 3 * 4096, 4096)


@pytest.mark.parametrize("route,name", ROUTES + [(1, None)], ids=["direct", "prefilter", "rule"])
@pytest.mark.parametrize("how", ["one-off-by-1", "all-off-by-16", "two-tensors"])
def test_alignment(how, route, name):
    """By the rule a compiled codec pre-filters 4 KiB blocks when every pointer
    is 16-byte aligned, and one unaligned pointer makes the whole call
    byte-wise: the direct route."""
    rng = np.random.default_rng(97)
    ref = clean_shards(*ALIGNED[:4])
    buf = ref.copy()
    blocks = blocks_of(8, ALIGNED[3], ALIGNED[4])
    for b, blk in enumerate(blocks):
        corrupt_shards(stripe_of(buf, blk), rng, 0, [7 + b], cols=[16 * b + 1, 4095])
    if name is None:
        name = "direct" if how == "one-off-by-1" else "prefilter"
    kw = {"one-off-by-1": dict(offsets=[0] * 7 + [1] + [0] * 6),
          "all-off-by-16": dict(offsets=[16] * 14), "two-tensors": dict(layout=two_tensors)}[how]
    got, status, changed, counts = scrub(*ALIGNED, (route, name), buf, **kw)
    assert (got == ref).all()
    assert status.tolist() == [CORRECTED] * 3 and counts[:, 0].tolist() == [2] * 3
    assert [np.nonzero(c)[0].tolist() for c in changed] == [[7], [8], [9]]


def tiny_blocks(n_blocks, bad):
    """10+4 shards of n_blocks blocks of 16 bytes, the oracle's; one wrong byte
    in shard b % 14, column b % 16 of every block b in `bad`."""
    ref = reference(10, 4, 16)
    clean = np.ascontiguousarray(
        ref[np.arange(n_blocks) % NS].transpose(1, 0, 2).reshape(14, n_blocks * 16))
    buf = clean.copy()
    bad = np.asarray(sorted(bad), np.int64)
    buf[bad % 14, bad * 16 + bad % 16] ^= ((bad % 255) + 1).astype(np.uint8)
    return clean, buf


@pytest.mark.parametrize("route,name", ROUTES)
@pytest.mark.parametrize("n_blocks,step", [(300, 3), (300, 1), (70000, 3), (70000, 1)],
                         ids=["300-third", "300-all", "70000-third", "70000-all"])
def test_the_list(n_blocks, step, route, name):
    """More than 65,535 blocks: a workgroup's second block on the direct route,
    the compaction's and the list kernel's second trip on the other."""
    bad = range(0, n_blocks, step)
    clean, buf = tiny_blocks(n_blocks, bad)
    got, status, changed, counts = scrub(8, 10, 4, n_blocks * 16, 16, (route, name), buf)
    assert (got == clean).all()
    want = np.zeros(n_blocks, np.uint8)
    want[list(bad)] = CORRECTED
    assert (status == want).all()  # the list equals nonzero(status): checked in scrub()
    assert (counts[:, 0] == want).all() and not counts[:, 1].any()
    assert (changed.sum(axis=1) == want).all()


@pytest.mark.parametrize("route,name", ROUTES)
def test_two_calls_on_one_stream_and_the_python_entry(route, name):
    """Back to back on one stream through ReedSolomon.scrub, the second on
    clean shards: the verdict words and the count belong to a call."""
    clean, buf = tiny_blocks(300, range(0, 300, 7))
    r = codec(8, 10, 4)
    old = LIB.rse_get_option(SCRUB_ROUTE)
    assert LIB.rse_set_option(SCRUB_ROUTE, route) == 0
    try:
        damaged = [torch.from_numpy(row.copy()).cuda() for row in buf]
        first = r.scrub(damaged, 16)
        shards = [torch.from_numpy(row.copy()).cuda() for row in clean]
        status, changed, counts, bad, n_bad = r.scrub(shards, block_len=16)
    finally:
        LIB.rse_set_option(SCRUB_ROUTE, old)
    assert R.core.last_kernel() == "scrub-shards gf8 10+4 " + name
    torch.cuda.synchronize()
    assert first[4].cpu().tolist() == [43] and first[3][:43].cpu().tolist() == list(range(0, 300, 7))
    assert (np.stack([t.cpu().numpy() for t in damaged]) == clean).all(), "repaired in place"
    assert n_bad.cpu().tolist() == [0] and not status.cpu().numpy().any()
    assert not changed.cpu().numpy().any() and not counts.cpu().numpy().any()
    assert [tuple(t.shape) for t in (status, changed, counts, bad, n_bad)] == \
        [(300,), (300, 14), (300, 2), (300,), (1,)]
    assert bad.dtype == torch.int32 and counts.dtype == torch.int32
    # one block by default, and a shorter last block
    assert [tuple(t.shape) for t in r.scrub(shards)] == [(1,), (1, 14), (1, 2), (1,), (1,)]
    assert tuple(r.scrub(shards, 17 * 16)[0].shape) == (18,)
    with pytest.raises(R.RSError):
        r.scrub(shards[:13], 16)
    with pytest.raises(R.RSError):  # flags of the wrong shape
        r.scrub(shards, 16, np.ones((299, 14), np.uint8))
    torch.cuda.synchronize()


@pytest.mark.parametrize("route,name", ROUTES)
def test_non_default_stream(route, name):
    rng = np.random.default_rng(101)
    ref = clean_shards(*ADDR[:4])
    buf = ref.copy()
    corrupt_shards(stripe_of(buf, (3 * 4096, 4 * 4096)), rng, 0, [5, 12])
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        got, status, changed, counts = scrub(*ADDR, (route, name), buf)
    assert (got == ref).all()
    assert status.tolist() == [CLEAN, CLEAN, CLEAN, CORRECTED, CLEAN, CLEAN]
    assert np.nonzero(changed[3])[0].tolist() == [5, 12] and counts[3].tolist() == [2 * 4096, 0]
