"""rse_read_shards on the GPU: rse_read_flat for separately allocated shards, a
block of columns in the place of a stripe, and shards that have no buffer.

Expected rows, classes and `result` come from tests/read_shards_model.py --
read_model.expected, which is the ORACLE's reconstruct, on every block alone
with that block's length and the flags of the NULL shards cleared.  Whole
buffers are compared: `out` has rows of stride B, a sentinel fill and a guard
row past n_reads, so the rows of lost entries, the rest of a row of the shorter
last block and the guard must keep their bytes; `status` has a guard entry;
`result` starts as 0xA5A5A5A5.  Every shard that has a buffer lies in an
allocation of its own between 64 guard bytes of 0xA5 and is compared whole
afterwards: the shards are only read.  A shard without a buffer is a NULL
pointer and nothing else: its bytes never reach the device.
rse_last_kernel() must name the route the contract predicts.  A GF(2^16) shard
is handled as its bytes: 2 x len per shard.
"""
import ctypes

import numpy as np
import pytest
import torch

import reed_solomon_erasure as R
from reed_solomon_erasure._lib import load

import read_model as RM
import read_shards_model as RSM
from test_gpu_read import flag_rows

pytestmark = pytest.mark.gpu

LIB = load()
FILL32 = 0xA5A5A5A5
OUT_FILL, STATUS_FILL = 0xC3, 0xEE
GUARD = 64
GRID_X = 2  # RSE_OPT_GRID_X (include/rse_hip_tune.h)
INVALID = 100  # RSE_ERR_INVALID_ARGUMENT

# (field, k, p, len, block_len) in elements
SHAPES = [
    (8, 10, 4, 1, 0),                    # one byte, one block
    (8, 10, 4, 17, 5),                   # the byte path, a tail of 2
    (8, 10, 4, 4096 + 48, 1024),         # the vector path, a tail of 48
    (8, 10, 4, 3 * 4112 + 32, 4112),     # two spans per block, a short second span; the tail in the first
    (8, 10, 4, 2 * 1024 + 8, 1024),      # aligned pointers, the tail forces the byte path
    (8, 10, 4, 64, 100),                 # block_len > len
    (8, 1, 1, 16, 16),                   # the smallest codec, one block of exactly len
    (8, 4, 20, 3 * 272, 272),            # 24 entries in a block: two output groups
    (8, 128, 128, 96, 48),               # 256 pointers
    (16, 10, 4, 9, 4),                   # 8-byte blocks, a tail of one element
    (16, 100, 28, 2064, 1032),           # GF(2^16), a wide codec, the vector path
]
LISTS = ("one-erased", "everything", "mixed", "erased-parity")
A = (8, 10, 4, 4096 + 48, 1024)  # the shape of most further cases: five blocks, the last of 48 bytes
NB = 5

_CLEAN = {}
_MODELS = {}


def codec(field, k, p):
    return (R.galois_16 if field == 16 else R.galois_8).ReedSolomon(k, p)


def clean_shards(field, k, p, elems):
    """k + p consistent shards as bytes (parity by the ORACLE), (k + p, bytes per
    shard); computed once per shape, never modified."""
    key = (field, k, p, elems)
    if key not in _CLEAN:
        rng = np.random.default_rng(1000003 * field + 4099 * k + 17 * p + elems)
        buf = rng.integers(0, 256, (k + p, elems * (field // 8)), dtype=np.uint8)
        RSM.encode(field, k, p, buf)
        buf.setflags(write=False)
        _CLEAN[key] = buf
    return _CLEAN[key]


def block_flags(k, p, nb, rng):
    """Block b gets flag row (b + 1) mod 6 of test_gpu_read.flag_rows' six kinds:
    block 0 has one data shard erased, block 2 is past repair."""
    rows = flag_rows(k, p, rng)
    return np.stack([rows[(b + 1) % 6] for b in range(nb)])


def kind(block):
    return (block + 1) % 6


def make_list(which, k, p, present, rng):
    nb, T = present.shape
    if which == "one-erased":
        return [(0, int(np.flatnonzero(present[0, :k] == 0)[0]))]
    if which == "everything":
        return [(b, i) for b in range(nb) for i in range(T)]
    if which == "erased-parity":  # of the rows with erased parity: mixed, past repair, parity only
        return [(b, int(i)) for b in range(nb) if kind(b) in (2, 3, 5)
                for i in np.flatnonzero(present[b] == 0) if i >= k]
    out = []  # erased and present shards mixed, in every block that has both
    for b in range(nb):
        erased = np.flatnonzero(present[b] == 0).tolist()
        there = np.flatnonzero(present[b] != 0).tolist()
        pick = set(rng.choice(erased, min(len(erased), 3), replace=False).tolist()) if erased else set()
        pick |= set(rng.choice(there, min(len(there), 2), replace=False).tolist()) if there else set()
        out += [(b, int(i)) for i in sorted(pick)]
    return out


def with_erased(host, present, block_bytes, fill, rng=None):
    """The shards with every erased shard's bytes of that block zeroed or
    filled with garbage."""
    out = np.array(host)
    for b, i in np.argwhere(present == 0):
        lo, hi = b * block_bytes, min((b + 1) * block_bytes, out.shape[1])
        out[i, lo:hi] = 0 if fill == "zeros" else rng.integers(0, 256, hi - lo, dtype=np.uint8)
    return out


def separate(host, offsets, null=()):
    """Every shard that has a buffer in an allocation of its own: guard,
    `offsets[i]` spare bytes, the shard, guard.  A shard in `null` gets nothing."""
    allocs, views = [], []
    for i, row in enumerate(host):
        if i in null:
            views.append(None)
            continue
        off = offsets[i]
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


def shards_kept(allocs, views, host):
    """The guards and everything else around the shards are 0xA5, and every
    shard that has a buffer is what it was."""
    for a in allocs:
        h = a.cpu().numpy()
        keep = np.ones(len(h), bool)
        for v in views:
            if v is not None and a.data_ptr() <= v.data_ptr() < a.data_ptr() + a.numel():
                lo = v.data_ptr() - a.data_ptr()
                keep[lo:lo + v.numel()] = False
        assert keep[:GUARD].all() and keep[-GUARD:].all()
        assert (h[keep] == 0xA5).all(), "bytes around a shard were written"
    for i, v in enumerate(views):
        if v is not None:
            assert np.array_equal(v.cpu().numpy(), host[i]), "shard %d was written" % i


def offset_fill(n, off, fill):
    """n bytes of `fill` in HBM starting `off` bytes into their allocation."""
    buf = torch.full((n + 64,), fill, dtype=torch.uint8, device="cuda")
    return buf[off:off + n]


def pointer_arrays(views, elems):
    n = len(views)
    return ((ctypes.c_void_p * n)(*[None if v is None else v.data_ptr() for v in views]),
            (ctypes.c_size_t * n)(*[elems] * n))


def run(r, field, elems, block_len, host, present, reads, null=(), offsets=None, out_off=0,
        layout="separate"):
    """rse_read_shards through the C entry on a copy of `host` (k + p, bytes) in
    HBM, the shards in `null` without a buffer.  Returns (out with its guard row,
    status with its guard entry, result words, kernel name); the shards are
    checked to be what they were."""
    T = host.shape[0]
    n = len(reads)
    bbytes = RSM.cut(elems, block_len)[0] * (field // 8)
    if layout == "separate":
        allocs, views = separate(host, offsets or [0] * T, set(null))
    else:
        allocs, views = two_tensors(host, r.data_shard_count())
    out = offset_fill((n + 1) * bbytes, out_off, OUT_FILL)
    dpres = None if present is None else torch.from_numpy(np.array(present)).cuda()
    lst = torch.from_numpy(np.array(reads, dtype=np.uint32).reshape(-1, 2).view(np.int32)).cuda()
    status = torch.full((n + 1,), STATUS_FILL, dtype=torch.uint8, device="cuda")
    result = torch.full((2,), FILL32 - (1 << 32), dtype=torch.int32, device="cuda")
    ptrs, lens = pointer_arrays(views, elems)
    rc = LIB.rse_read_shards(r._h, ptrs, lens, T, block_len,
                             None if dpres is None else dpres.data_ptr(), lst.data_ptr(), n,
                             out.data_ptr(), status.data_ptr(), result.data_ptr(),
                             torch.cuda.current_stream().cuda_stream)
    name = LIB.rse_last_kernel().decode()
    assert rc == 0
    torch.cuda.synchronize()
    shards_kept(allocs, views, host)
    return (out.cpu().numpy().reshape(n + 1, bbytes), status.cpu().numpy(),
            [int(v) & 0xFFFFFFFF for v in result.cpu().tolist()], name)


def wanted(model, n, bbytes):
    """The whole `out` and `status` buffers the model expects, guards included:
    a row of the shorter last block keeps the sentinel past the block's length."""
    rows, status, result = model
    out = np.full((n + 1, bbytes), OUT_FILL, np.uint8)
    st = np.full(n + 1, STATUS_FILL, np.uint8)
    for u, row in enumerate(rows):
        if row is not None:
            out[u, :len(row)] = row
        if status is not None:
            st[u] = status[u]
    return out, st, result


def check(got, model, n, bbytes, what=""):
    out, status, result = got
    want_out, want_status, want_result = wanted(model, n, bbytes)
    assert result == want_result, what
    assert np.array_equal(status, want_status), (what, status.tolist(), want_status.tolist())
    assert np.array_equal(out, want_out), (what, np.argwhere(out != want_out)[:4].tolist())


def predicted_name(field, k, p, elems, block_len, offsets=(0,), out_off=0):
    # torch's allocations and the guards are multiples of 16: the offsets decide
    es = field // 8
    vec = (all(o % 16 == 0 for o in offsets) and out_off % 16 == 0
           and (RSM.cut(elems, block_len)[0] * es) % 16 == 0 and (elems * es) % 16 == 0)
    return "read-shards gf%d %d+%d %s" % (field, k, p, "vec" if vec else "bytes")


def test_predicted_routes_of_the_shapes():
    """The table's reasons, restated: which shapes take which route."""
    vec = [predicted_name(*s).endswith("vec") for s in SHAPES]
    assert vec == [False, False, True, True, False, True, True, True, True, False, True]


@pytest.mark.parametrize("field,k,p,elems,block_len", SHAPES,
                         ids=["gf%d-%d+%d-%d-%d" % s for s in SHAPES])
def test_lists_over_the_flag_rows(field, k, p, elems, block_len):
    """Every list on shards whose erased ranges hold zeros, and -- the results
    must not change -- garbage."""
    r = codec(field, k, p)
    clean = clean_shards(field, k, p, elems)
    b, nb = RSM.cut(elems, block_len)
    bbytes = b * (field // 8)
    rng = np.random.default_rng(7 * elems + 31 * k + p)
    present = block_flags(k, p, nb, rng)
    zeros = with_erased(clean, present, bbytes, "zeros")
    garbage = with_erased(clean, present, bbytes, "garbage", rng)
    for which in LISTS:
        reads = make_list(which, k, p, present, rng)
        if not reads:  # no block with erased parity
            assert which == "erased-parity" and (nb == 1 or p == 1)
            continue
        assert RM.first_offender(reads, nb, k + p) is None
        model = RSM.expected(field, k, p, clean, block_len, present, reads)
        assert model[2][0] == RSM.SERVED
        if which == "everything" and nb >= 3:  # every class occurs, and block 2 is past repair
            assert set(model[1]) == {RSM.COPIED, RSM.REBUILT, RSM.LOST}
            assert model[2][1] == p + 1
        if which == "one-erased":
            assert model[1] == [RSM.REBUILT]
        for start, host in (("zeros", zeros), ("garbage", garbage)):
            *got, name = run(r, field, elems, block_len, host, present, reads)
            assert name == predicted_name(field, k, p, elems, block_len), (which, start)
            check(got, model, len(reads), bbytes, (which, start))


NULL_CASES = ("one-no-flags", "one-with-flags", "p-of-them", "p+1-of-them")


@pytest.mark.parametrize("case", NULL_CASES)
@pytest.mark.parametrize("elems,block_len", [(4096 + 48, 1024), (17, 5)], ids=["vec", "bytes"])
def test_shards_without_a_buffer(elems, block_len, case):
    """NULL pointers among the shards of 10+4: one data shard with present =
    NULL is rebuilt in every block; the same under flags that erase others too;
    p of them are all rebuilt; with p + 1 every erased entry is lost, the present
    ones are copied and result[1] counts the lost."""
    field, k, p = 8, 10, 4
    r = codec(field, k, p)
    clean = clean_shards(field, k, p, elems)
    b, nb = RSM.cut(elems, block_len)
    rng = np.random.default_rng(elems + NULL_CASES.index(case))
    null = {"one-no-flags": (3,), "one-with-flags": (3,), "p-of-them": (0, 5, k, k + 2),
            "p+1-of-them": (0, 5, 9, k, k + 2)}[case]
    present = block_flags(k, p, nb, rng) if case == "one-with-flags" else None
    host = clean if present is None else with_erased(clean, present, b, "garbage", rng)
    reads = [(blk, i) for blk in range(nb) for i in range(k + p)]
    model = RSM.expected(field, k, p, clean, block_len, present, reads, null)
    rows, status, result = model
    for u, (blk, i) in enumerate(reads):
        if i in null:
            assert status[u] != RSM.COPIED
        if case == "one-no-flags":
            assert status[u] == (RSM.REBUILT if i in null else RSM.COPIED)
        if case == "p-of-them":
            assert status[u] == (RSM.REBUILT if i in null else RSM.COPIED)
        if case == "p+1-of-them":
            assert status[u] == (RSM.LOST if i in null else RSM.COPIED)
    if case == "p+1-of-them":
        assert result == [RSM.SERVED, (p + 1) * nb]
    if case == "one-with-flags":  # the NULL shard joins the row's own erasures
        assert {RSM.COPIED, RSM.REBUILT, RSM.LOST} == set(status)
        assert result[1] >= p + 1
    *got, name = run(r, field, elems, block_len, host, present, reads, null=null)
    assert name == predicted_name(field, k, p, elems, block_len)
    check(got, model, len(reads), b, case)
    if case != "p+1-of-them" and present is None:
        for u, (blk, i) in enumerate(reads):  # the rebuilt rows are the bytes that never got there
            assert np.array_equal(got[0][u, :len(rows[u])], clean[i, blk * b:blk * b + len(rows[u])])


def test_blocks_that_are_not_codewords_pin_the_inputs():
    """Data shard 4 of 10+4 has no buffer: the valid set of every block is the
    nine other data shards and parity 0.  A byte flipped in a shard of the valid
    set changes the rebuilt bytes of its block; one flipped in a present shard
    outside it does not."""
    field, k, p, elems, block_len = A
    r = codec(field, k, p)
    clean = clean_shards(field, k, p, elems)
    reads = [(b, i) for b in range(NB) for i in (4, k + 2)]
    null = (4,)
    base = RSM.expected(field, k, p, clean, block_len, None, reads, null)
    inside, outside = np.array(clean), np.array(clean)
    inside[k, 2 * 1024 + 100] ^= 0x40   # parity 0, block 2: the last shard of the valid set
    inside[7, elems - 1] ^= 1           # a data shard of it, the last byte of the shorter last block
    outside[k + 1, 2 * 1024 + 100] ^= 0x40  # parity 1 and 3: present, not among the first k
    outside[k + 3, elems - 1] ^= 1
    m_in = RSM.expected(field, k, p, inside, block_len, None, reads, null)
    m_out = RSM.expected(field, k, p, outside, block_len, None, reads, null)
    for u, (b, i) in enumerate(reads):
        if i == 4:
            assert m_in[1][u] == RSM.REBUILT
            assert np.array_equal(m_out[0][u], base[0][u])
            assert np.array_equal(m_in[0][u], base[0][u]) == (b not in (2, 4))
    for host, model, what in ((inside, m_in, "inside"), (outside, m_out, "outside")):
        *got, _ = run(r, field, elems, block_len, host, None, reads, null=null)
        check(got, model, len(reads), 1024, what)


@pytest.mark.parametrize("offsets,out_off", [({3: 1}, 0), ({12: 8}, 0), ({}, 8)],
                         ids=["shard3+1", "parity2+8", "out+8"])
def test_a_misaligned_pointer_takes_the_byte_route(offsets, out_off):
    field, k, p, elems, block_len = A
    r = codec(field, k, p)
    clean = clean_shards(field, k, p, elems)
    rng = np.random.default_rng(91)
    present = block_flags(k, p, NB, rng)
    reads = make_list("mixed", k, p, present, rng)
    model = RSM.expected(field, k, p, clean, block_len, present, reads)
    offs = [offsets.get(i, 0) for i in range(k + p)]
    *aligned, name_a = run(r, field, elems, block_len, clean, present, reads)
    *got, name = run(r, field, elems, block_len, clean, present, reads, offsets=offs,
                     out_off=out_off)
    assert name_a == "read-shards gf8 10+4 vec" and name == "read-shards gf8 10+4 bytes"
    assert name == predicted_name(field, k, p, elems, block_len, offs, out_off)
    check(got, model, len(reads), 1024)
    assert np.array_equal(aligned[0], got[0]) and np.array_equal(aligned[1], got[1])


def test_a_misaligned_shard_without_a_buffer_decides_nothing():
    """The misaligned shard is the one that is NULL: the vector route stays."""
    field, k, p, elems, block_len = A
    r = codec(field, k, p)
    clean = clean_shards(field, k, p, elems)
    reads = [(b, i) for b in range(NB) for i in (2, 3)]
    offs = [1 if i == 3 else 0 for i in range(k + p)]
    model = RSM.expected(field, k, p, clean, block_len, None, reads, (3,))
    *got, name = run(r, field, elems, block_len, clean, None, reads, null=(3,), offsets=offs)
    assert name == "read-shards gf8 10+4 vec"
    check(got, model, len(reads), 1024)


def test_rows_of_two_tensors():
    """Data as the rows of a [k, L] tensor, parity as the rows of a [p, L]
    tensor: the layout of INTEGRATION section 4."""
    field, k, p, elems, block_len = A
    r = codec(field, k, p)
    clean = clean_shards(field, k, p, elems)
    rng = np.random.default_rng(5)
    present = block_flags(k, p, NB, rng)
    host = with_erased(clean, present, 1024, "garbage", rng)
    reads = make_list("everything", k, p, present, rng)
    model = RSM.expected(field, k, p, clean, block_len, present, reads)
    *got, name = run(r, field, elems, block_len, host, present, reads, layout="two-tensors")
    assert name == "read-shards gf8 10+4 vec"
    check(got, model, len(reads), 1024)


BASE = [(0, 1), (0, 13), (1, 2), (2, 0), (2, 5), (3, 9), (4, 0)]


def rejected_lists():
    swapped = list(BASE)
    swapped[3], swapped[4] = swapped[4], swapped[3]
    return [
        ("block-is-n_blocks", BASE + [(NB, 0)], 7),
        ("shard-is-k+p", BASE[:5] + [(3, 14)] + BASE[6:], 5),
        ("shard-is-all-ones", BASE[:6] + [(4, 0xFFFFFFFF)], 6),
        ("duplicate", BASE[:2] + [BASE[1]] + BASE[2:], 2),
        ("descending-shards", swapped, 4),
        ("descending-blocks", [(0, 1), (1, 2), (0, 13)] + BASE[3:], 2),
        ("offender-first", [(NB + 3, 0)] + BASE, 0),
        ("offender-last", BASE + [(4, 0)], 7),
    ]


@pytest.mark.parametrize("reads,offender", [pytest.param(u, o, id=n)
                                            for n, u, o in rejected_lists()])
def test_rejected_lists_write_nothing(reads, offender):
    field, k, p, elems, block_len = A
    r = codec(field, k, p)
    clean = clean_shards(field, k, p, elems)
    present = block_flags(k, p, NB, np.random.default_rng(5))
    assert RSM.cut(elems, block_len)[1] == NB and RM.first_offender(BASE, NB, k + p) is None
    model = RSM.expected(field, k, p, clean, block_len, present, reads, (6,))
    assert model[2] == [RSM.REJECTED, offender]
    *got, _ = run(r, field, elems, block_len, clean, present, reads, null=(6,))
    assert got[2] == [1, offender]
    assert (got[0] == OUT_FILL).all(), "a rejected list wrote rows"
    assert (got[1] == STATUS_FILL).all(), "a rejected list wrote classes"
    check(got, model, len(reads), 1024)


def with_grid(grid, fn):
    old = LIB.rse_get_option(GRID_X)
    assert LIB.rse_set_option(GRID_X, grid) == 0
    try:
        return fn()
    finally:
        LIB.rse_set_option(GRID_X, old)


def many_runs():
    """300 blocks of 48 B and a last one of 16 B of 10+4, shard 7 without a
    buffer, random erasures beside it and a run of 1..4 entries in about every
    fourth block, the last block among them."""
    if "many" not in _MODELS:
        field, k, p, elems, block_len, nb = 8, 10, 4, 300 * 48 + 16, 48, 301
        clean = clean_shards(field, k, p, elems)
        rng = np.random.default_rng(300)
        present = np.ones((nb, k + p), np.uint8)
        reads = []
        for block in sorted(set(rng.choice(nb, 80, replace=False).tolist() + [0, nb - 1])):
            present[block, rng.choice(k + p, int(rng.integers(0, p + 1)), replace=False)] = 0
            reads += [(block, int(i)) for i in sorted(rng.choice(k + p, int(rng.integers(1, 5)),
                                                                 replace=False).tolist())]
        model = RSM.expected(field, k, p, clean, block_len, present, reads, (7,))
        assert {RSM.COPIED, RSM.REBUILT, RSM.LOST} == set(model[1])
        _MODELS["many"] = (field, k, p, elems, block_len, clean, present, reads, model)
    return _MODELS["many"]


@pytest.mark.parametrize("grid", [1, 3])
def test_grid_stride_over_many_runs(grid):
    """With 1 or 3 workgroups each walks many runs."""
    field, k, p, elems, block_len, clean, present, reads, model = many_runs()
    r = codec(field, k, p)
    *got, name = with_grid(grid, lambda: run(r, field, elems, block_len, clean, present, reads,
                                             null=(7,)))
    assert name == "read-shards gf8 10+4 vec"
    check(got, model, len(reads), 48)


@pytest.mark.parametrize("grid", [1, 3])
def test_grid_stride_over_many_spans(grid):
    """A block of 64 KiB + 16 (17 spans, the last one of 16 bytes) and a last
    block of 4 KiB + 32 (2 of its 17 items have bytes), a rebuilt and a copied
    entry in each, walked by 1 or 3 workgroups."""
    field, k, p, block_len = 8, 10, 4, 64 * 1024 + 16
    elems = block_len + 4096 + 32
    r = codec(field, k, p)
    clean = clean_shards(field, k, p, elems)
    reads = [(0, 0), (0, 4), (0, 11), (1, 1), (1, 4), (1, 11)]
    model = RSM.expected(field, k, p, clean, block_len, None, reads, (4, 11))
    assert model[1] == [RSM.COPIED, RSM.REBUILT, RSM.REBUILT] * 2
    *got, name = with_grid(grid, lambda: run(r, field, elems, block_len, clean, None, reads,
                                             null=(4, 11)))
    assert name == "read-shards gf8 10+4 vec"
    check(got, model, len(reads), block_len)


def test_a_host_pointer_among_the_shards_is_refused():
    """Shard 5 in host memory, under a list that would be rejected anyway (so
    no kernel could touch it): RSE_ERR_INVALID_ARGUMENT, nothing written."""
    field, k, p, elems, block_len = 8, 10, 4, 64, 16
    r = codec(field, k, p)
    clean = clean_shards(field, k, p, elems)
    allocs, views = separate(clean, [0] * (k + p), {2})
    ptrs, lens = pointer_arrays(views, elems)
    host_shard = np.array(clean[5])
    ptrs[5] = host_shard.ctypes.data
    lst = torch.tensor([[4, 0]], dtype=torch.int32, device="cuda")  # block 4 of 4: not in order
    out = torch.full((16,), OUT_FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((1,), STATUS_FILL, dtype=torch.uint8, device="cuda")
    result = torch.full((2,), FILL32 - (1 << 32), dtype=torch.int32, device="cuda")
    rc = LIB.rse_read_shards(r._h, ptrs, lens, k + p, block_len, None, lst.data_ptr(), 1,
                             out.data_ptr(), status.data_ptr(), result.data_ptr(),
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == INVALID
    assert [int(v) & 0xFFFFFFFF for v in result.cpu().tolist()] == [FILL32, FILL32]
    assert (out.cpu().numpy() == OUT_FILL).all() and status.cpu().tolist() == [STATUS_FILL]
    shards_kept(allocs, views, clean)


def test_round_trip_of_a_failed_device_onto_a_spare():
    """Encode a [k, L] / [p, L] pair, drop data shard 3's buffer (None), read
    the whole shard onto a spare: the spare holds the original data, and the
    shards verify with the spare in its place."""
    field, k, p, elems, block_len, lost = 8, 10, 4, 4 * 1024, 1024, 3
    r = codec(field, k, p)
    rng = np.random.default_rng(11)
    host = rng.integers(0, 256, (k, elems), dtype=np.uint8)
    data = torch.from_numpy(host).cuda()
    parity = torch.zeros((p, elems), dtype=torch.uint8, device="cuda")
    shards = [data[i] for i in range(k)] + [parity[j] for j in range(p)]
    r.encode(shards)
    assert r.verify(shards)
    degraded = list(shards)
    degraded[lost] = None
    spare = torch.full((elems,), OUT_FILL, dtype=torch.uint8, device="cuda")
    out, status, result = r.read(degraded, block_len, None, [(b, lost) for b in range(4)],
                                 out=spare)
    torch.cuda.synchronize()
    assert out is spare
    assert result.cpu().tolist() == [R.READ_SERVED, 0]
    assert status.cpu().tolist() == [R.READ_REBUILT] * 4
    assert np.array_equal(spare.cpu().numpy(), host[lost])
    healed = list(shards)
    healed[lost] = spare
    assert r.verify(healed)
    spare[5] ^= 1
    assert not r.verify(healed)


@pytest.mark.parametrize("field", [8, 16])
def test_python_wrapper_host_list_and_device_list_agree(field):
    k, p, elems, block_len = 10, 4, 2 * 520 + 24, 520
    es = field // 8
    r = codec(field, k, p)
    clean = clean_shards(field, k, p, elems)
    nb, bbytes = 3, block_len * es
    rng = np.random.default_rng(field)
    present = block_flags(k, p, nb, rng)
    reads = make_list("mixed", k, p, present, rng) + [(2, 6)]
    reads = sorted(set(reads))
    null = (6,)
    model = RSM.expected(field, k, p, clean, block_len, present, reads, null)
    dev = torch.from_numpy(np.array(clean)).cuda()
    shards = [None if i in null else dev[i] for i in range(k + p)]
    dpres = torch.from_numpy(present).cuda()
    dlist = torch.tensor(reads, dtype=torch.int32, device="cuda")
    mine = torch.full((len(reads) * bbytes,), OUT_FILL, dtype=torch.uint8, device="cuda")
    out_a, st_a, res_a = r.read(shards, block_len, dpres, reads, out=mine)
    out_b, st_b, res_b = r.read(shards, block_len, dpres, dlist)
    assert out_a is mine and out_b.numel() == len(reads) * bbytes and out_b.is_cuda
    assert st_a.shape == st_b.shape == (len(reads),) and st_a.dtype == torch.uint8
    assert res_a.shape == res_b.shape == (2,) and res_a.dtype == torch.int32
    torch.cuda.synchronize()
    assert res_a.cpu().tolist() == res_b.cpu().tolist() == model[2]
    assert st_a.cpu().tolist() == st_b.cpu().tolist() == model[1]
    a, b = out_a.cpu().numpy().reshape(-1, bbytes), out_b.cpu().numpy().reshape(-1, bbytes)
    for u, row in enumerate(model[0]):
        if row is not None:  # a fresh buffer holds anything where nothing is written
            assert np.array_equal(a[u, :len(row)], row) and np.array_equal(b[u, :len(row)], row)
            assert (a[u, len(row):] == OUT_FILL).all()
        else:
            assert (a[u] == OUT_FILL).all()
    assert np.array_equal(dev.cpu().numpy(), clean)
    # a rejected list comes back in `result`, not as an exception
    _, _, bad = r.read(shards, block_len, dpres, [(1, 0), (0, 0)])
    torch.cuda.synchronize()
    assert bad.cpu().tolist() == [R.READ_REJECTED, 1]
    # the argument checks of read_flat()
    with pytest.raises(ValueError):
        r.read(shards, block_len, dpres, reads, out=mine[:-1])
    with pytest.raises(ValueError):
        r.read(shards, block_len, dpres, reads, out=mine.cpu())
    with pytest.raises(ValueError):
        r.read([None] * (k + p), block_len, None, reads)
    with pytest.raises(R.RSError):
        r.read(shards, block_len, dpres[:2], reads)
