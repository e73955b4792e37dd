"""rse_update_shards on the GPU: rse_update_flat for separately allocated
shards, a block of columns in the place of a stripe.

Expected bytes come from tests/update_shards_model.py -- update_model.apply,
which is the ORACLE's encode of the difference XORed into the parity that was
there, on every block alone with that block's length.  Every shard is compared
whole and lies between 64 guard bytes of 0xA5 before and after, which must
survive.  new_data is compared with itself afterwards (it is only read);
`result` starts as 0xA5A5A5A5.  Every list runs on consistent shards (parity by
the oracle) and on shards made inconsistent first, as tests/test_gpu_update.py
does: the syndrome must be preserved, not repaired and not sealed in.
rse_last_kernel() must name the route the contract predicts.  A GF(2^16) shard
is handled as its bytes: 2 x len per shard.
"""
import ctypes

import numpy as np
import pytest
import torch

import reed_solomon_erasure as R
from reed_solomon_erasure._lib import load

import update_model as UM
import update_shards_model as USM

pytestmark = pytest.mark.gpu

LIB = load()
FILL32 = 0xA5A5A5A5
GUARD = 64
GRID_X = 2  # RSE_OPT_GRID_X (include/rse_hip_tune.h)
INVALID = 100  # RSE_ERR_INVALID_ARGUMENT

# (field, k, p, len, block_len) in elements
SHAPES = [
    (8, 10, 4, 1, 0),                    # one byte
    (8, 10, 4, 17, 5),                   # the byte path, a tail of 2
    (8, 10, 4, 4096 + 48, 1024),         # the vector path, a tail of 48
    (8, 10, 4, 3 * 4112 + 32, 4112),     # two spans per block, a short second span; the tail in the first
    (8, 10, 4, 2 * 1024 + 8, 1024),      # aligned pointers, the tail forces the byte path
    (8, 10, 4, 64, 100),                 # block_len > len
    (8, 1, 1, 16, 16),                   # the smallest codec, one block of exactly len
    (8, 4, 20, 3 * 272, 272),            # two row groups
    (8, 128, 128, 96, 48),               # 256 pointers, eight groups, a run of 128 entries
    (16, 10, 4, 9, 4),                   # 8-byte blocks, a tail of one element
    (16, 20, 8, 2064, 1032),             # GF(2^16), the vector path, two full blocks
    (16, 128, 128, 32, 16),              # GF(2^16) at 256 shards
]
LISTS = ("one", "per-block", "whole-block", "mixed")
CASES = [pytest.param(*shape, which, id="gf%d-%d+%d-%d-%d-%s" % (*shape, which))
         for shape in SHAPES for which in LISTS]

_CLEAN = {}


def codec(field, k, p):
    return (R.galois_16 if field == 16 else R.galois_8).ReedSolomon(k, p)


def clean_shards(field, k, p, elems):
    """k + p consistent shards as bytes (parity by the ORACLE), (k + p, bytes per
    shard); computed once per shape, never modified."""
    key = (field, k, p, elems)
    if key not in _CLEAN:
        rng = np.random.default_rng(1000003 * field + 4099 * k + 17 * p + elems)
        buf = rng.integers(0, 256, (k + p, elems * (field // 8)), dtype=np.uint8)
        USM.encode(field, k, p, buf)
        buf.setflags(write=False)
        _CLEAN[key] = buf
    return _CLEAN[key]


def make_list(which, k, nb, rng):
    if which == "one":
        return [(nb // 2, k // 2)]
    if which == "per-block":
        return [(b, (3 * b + 1) % k) for b in range(nb)]
    if which == "whole-block":
        return [(nb - 1, i) for i in range(k)]  # the shorter last block where there is one
    out = []  # runs of mixed length that include block 0 and the last block
    blocks = sorted({0, 1 % nb, nb // 2, nb - 1})
    for block, length in zip(blocks, (1, 5, 3, 2)[-len(blocks):]):
        shards = sorted(rng.choice(k, min(k, length), replace=False).tolist())
        out += [(block, i) for i in shards]
    return out


def make_inconsistent(before, field, block_len, updates, k, p, rng):
    """One stale parity byte in every touched block, and one wrong byte in a
    data shard of it that the list does not name (where there is one)."""
    out = np.array(before)
    es = field // 8
    elems = out.shape[1] // es
    b, _ = USM.cut(elems, block_len)
    for block in sorted({blk for blk, _ in updates}):
        lo, hi = block * b * es, min((block + 1) * b, elems) * es
        out[k + int(rng.integers(p)), int(rng.integers(lo, hi))] ^= 0x5A
        free = sorted(set(range(k)) - {i for blk, i in updates if blk == block})
        if free:
            out[free[int(rng.integers(len(free)))], int(rng.integers(lo, hi))] ^= 0x3C
    return out


def new_bytes(n, field, elems, block_len, rng):
    return rng.integers(0, 256, (n, USM.cut(elems, block_len)[0] * (field // 8)), dtype=np.uint8)


def separate(host, offsets, order=None):
    """Every shard in an allocation of its own, made in `order`: guard,
    `offsets[i]` spare bytes, the shard, guard."""
    n = len(host)
    allocs, views = [None] * n, [None] * n
    for i in (order if order is not None else range(n)):
        row, off = host[i], offsets[i]
        a = torch.full((GUARD + off + len(row) + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        v = a[GUARD + off:GUARD + off + len(row)]
        v.copy_(torch.from_numpy(np.array(row)))
        allocs[i], views[i] = a, v
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
        keep = np.ones(len(h), bool)
        for v in views:
            if a.data_ptr() <= v.data_ptr() < a.data_ptr() + a.numel():
                lo = v.data_ptr() - a.data_ptr()
                keep[lo:lo + v.numel()] = False
        assert keep[:GUARD].all() and keep[-GUARD:].all()
        assert (h[keep] == 0xA5).all(), "bytes around a shard were written"


def offset_copy(host, off):
    """`host` in HBM starting `off` bytes into its allocation."""
    flat = np.array(host).reshape(-1)
    buf = torch.zeros(flat.size + 64, dtype=torch.uint8, device="cuda")
    view = buf[off:off + flat.size]
    view.copy_(torch.from_numpy(flat))
    return view


def pointer_arrays(views, elems):
    n = len(views)
    return ((ctypes.c_void_p * n)(*[v.data_ptr() for v in views]),
            (ctypes.c_size_t * n)(*[elems] * n))


def run(r, elems, block_len, before, updates, new, offsets=None, new_off=0, layout="separate",
        order=None, stream=None, sync=True, rc_want=0):
    """rse_update_shards through the C entry on a copy of `before` (k + p,
    bytes) in HBM.  Returns (shards after, result words, kernel name)."""
    stream = stream or torch.cuda.current_stream()
    n = before.shape[0]
    with torch.cuda.stream(stream):
        if layout == "separate":
            allocs, views = separate(before, offsets or [0] * n, order)
        else:
            allocs, views = two_tensors(before, r.data_shard_count())
        dnew = offset_copy(new, new_off)
        upd = torch.from_numpy(np.array(updates, dtype=np.uint32).reshape(-1, 2).view(np.int32)).cuda()
        result = torch.full((2,), FILL32 - (1 << 32), dtype=torch.int32, device="cuda")
    ptrs, lens = pointer_arrays(views, elems)
    rc = LIB.rse_update_shards(r._h, ptrs, lens, n, block_len, upd.data_ptr(), dnew.data_ptr(),
                               len(updates), result.data_ptr(), stream.cuda_stream)
    name = LIB.rse_last_kernel().decode()
    assert rc == rc_want
    handles = (allocs, views, dnew, upd, result, np.array(new))
    if not sync:
        return handles, name
    return (*collect(handles, stream), name)


def collect(handles, stream):
    allocs, views, dnew, upd, result, new = handles
    stream.synchronize()
    assert np.array_equal(dnew.cpu().numpy().reshape(new.shape), new), "new_data was written"
    guards_kept(allocs, views)
    got = np.stack([v.cpu().numpy() for v in views])
    return got, [int(v) & 0xFFFFFFFF for v in result.cpu().tolist()]


def predicted_name(field, k, p, elems, block_len, offsets=(0,), new_off=0):
    # torch's allocations and the guards are multiples of 16: the offsets decide
    es = field // 8
    vec = (all(o % 16 == 0 for o in offsets) and new_off % 16 == 0
           and (USM.cut(elems, block_len)[0] * es) % 16 == 0 and (elems * es) % 16 == 0)
    return "update-shards gf%d %d+%d %s" % (field, k, p, "vec" if vec else "bytes")


def test_predicted_routes_of_the_shapes():
    """The table's reasons, restated: which shapes take which route."""
    vec = [predicted_name(*s).endswith("vec") for s in SHAPES]
    assert vec == [False, False, True, True, False, True, True, True, True, False, True, True]


@pytest.mark.parametrize("field,k,p,elems,block_len,which", CASES)
def test_accepted_lists(field, k, p, elems, block_len, which):
    r = codec(field, k, p)
    clean = clean_shards(field, k, p, elems)
    nb = USM.cut(elems, block_len)[1]
    rng = np.random.default_rng(7 * elems + k + LISTS.index(which))
    updates = make_list(which, k, nb, rng)
    assert UM.first_offender(updates, nb, k) is None
    new = new_bytes(len(updates), field, elems, block_len, rng)
    for start in ("consistent", "inconsistent"):
        before = clean if start == "consistent" else make_inconsistent(clean, field, block_len,
                                                                       updates, k, p, rng)
        want = USM.apply(field, k, p, before, block_len, updates, new)
        got, result, name = run(r, elems, block_len, before, updates, new)
        assert name == predicted_name(field, k, p, elems, block_len), start
        assert result == USM.expected_result(updates, elems, block_len, k), start
        assert result == [0, len({b for b, _ in updates})], start
        assert np.array_equal(got, want), (start, np.argwhere(got != want)[:4].tolist())
        if start == "consistent":
            # a consistent code word stays one: the parity of a fresh oracle encode
            fresh = np.array(got)
            fresh[k:] = 0
            assert np.array_equal(USM.encode(field, k, p, fresh), got)


@pytest.mark.parametrize("offsets,new_off", [({3: 1}, 0), ({12: 8}, 0), ({}, 1)],
                         ids=["shard3+1", "parity2+8", "new+1"])
def test_misaligned_pointers_take_the_byte_path(offsets, new_off):
    field, k, p, elems, block_len = 8, 10, 4, 4096 + 48, 1024
    r = codec(field, k, p)
    clean = clean_shards(field, k, p, elems)
    rng = np.random.default_rng(91)
    updates = make_list("mixed", k, 5, rng)
    new = new_bytes(len(updates), field, elems, block_len, rng)
    offs = [offsets.get(i, 0) for i in range(k + p)]
    aligned, res_a, name_a = run(r, elems, block_len, clean, updates, new)
    got, res, name = run(r, elems, block_len, clean, updates, new, offsets=offs, new_off=new_off)
    assert name_a == "update-shards gf8 10+4 vec" and name == "update-shards gf8 10+4 bytes"
    assert name == predicted_name(field, k, p, elems, block_len, offs, new_off)
    assert res == res_a == USM.expected_result(updates, elems, block_len, k)
    assert np.array_equal(got, aligned)
    assert np.array_equal(got, USM.apply(field, k, p, clean, block_len, updates, new))


@pytest.mark.parametrize("layout", ["two-tensors", "shuffled"])
def test_rows_of_two_tensors_and_allocations_in_shuffled_order(layout):
    field, k, p, elems, block_len = 8, 10, 4, 4096 + 48, 1024
    r = codec(field, k, p)
    clean = clean_shards(field, k, p, elems)
    rng = np.random.default_rng(5)
    updates = make_list("mixed", k, 5, rng) + [(4, 9)]
    updates = sorted(set(updates))
    new = new_bytes(len(updates), field, elems, block_len, rng)
    before = make_inconsistent(clean, field, block_len, updates, k, p, rng)
    if layout == "shuffled":
        order = rng.permutation(k + p).tolist()
        got, result, name = run(r, elems, block_len, before, updates, new, order=order)
    else:
        got, result, name = run(r, elems, block_len, before, updates, new, layout="two-tensors")
    assert name == "update-shards gf8 10+4 vec"
    assert result == USM.expected_result(updates, elems, block_len, k)
    assert np.array_equal(got, USM.apply(field, k, p, before, block_len, updates, new))


NB = 5  # blocks of the shape below
BASE = [(0, 1), (0, 3), (1, 2), (2, 0), (2, 5), (3, 9), (4, 0)]


def rejected_lists():
    swapped = list(BASE)
    swapped[2], swapped[3] = swapped[3], swapped[2]
    return [
        ("block-is-n_blocks", BASE + [(NB, 0)], 7),
        ("shard-is-k", BASE[:5] + [(3, 10)] + BASE[6:], 5),
        ("block-is-all-ones", BASE + [(0xFFFFFFFF, 0)], 7),
        ("shard-is-all-ones", BASE[:6] + [(4, 0xFFFFFFFF)], 6),
        ("duplicate", BASE[:2] + [BASE[1]] + BASE[2:], 2),
        ("descending", swapped, 3),
        ("split-run", [(0, 1), (1, 2), (0, 3)] + BASE[3:], 2),
    ]


@pytest.mark.parametrize("updates,offender", [pytest.param(u, o, id=n)
                                              for n, u, o in rejected_lists()])
def test_rejected_lists_write_nothing(updates, offender):
    field, k, p, elems, block_len = 8, 10, 4, 4096 + 48, 1024
    r = codec(field, k, p)
    clean = clean_shards(field, k, p, elems)
    assert USM.cut(elems, block_len)[1] == NB and UM.first_offender(BASE, NB, k) is None
    assert USM.expected_result(updates, elems, block_len, k) == [1, offender]
    new = new_bytes(len(updates), field, elems, block_len, np.random.default_rng(offender))
    got, result, _ = run(r, elems, block_len, clean, updates, new)  # the guards: in collect()
    assert result == [1, offender]
    assert np.array_equal(got, clean), "a rejected list wrote shard bytes"


def test_host_memory_is_refused_before_anything_runs():
    """new_data in host memory, under a list that would be rejected anyway (so
    no kernel could touch it): RSE_ERR_INVALID_ARGUMENT, `result` untouched."""
    field, k, p, elems, block_len = 8, 10, 4, 64, 16
    r = codec(field, k, p)
    clean = clean_shards(field, k, p, elems)
    allocs, views = separate(clean, [0] * (k + p))
    ptrs, lens = pointer_arrays(views, elems)
    host_new = np.zeros((1, 16), np.uint8)
    upd = torch.tensor([[4, 0]], dtype=torch.int32, device="cuda")  # block 4 of 4: not in order
    result = torch.full((2,), FILL32 - (1 << 32), dtype=torch.int32, device="cuda")
    rc = LIB.rse_update_shards(r._h, ptrs, lens, k + p, block_len, upd.data_ptr(),
                               host_new.ctypes.data, 1, result.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == INVALID
    assert [int(v) & 0xFFFFFFFF for v in result.cpu().tolist()] == [FILL32, FILL32]
    assert np.array_equal(np.stack([v.cpu().numpy() for v in views]), clean)


def with_grid(grid, fn):
    old = LIB.rse_get_option(GRID_X)
    assert LIB.rse_set_option(GRID_X, grid) == 0
    try:
        return fn()
    finally:
        LIB.rse_set_option(GRID_X, old)


@pytest.mark.parametrize("grid", [1, 3])
def test_grid_stride_over_many_runs(grid):
    """300 blocks of 48 B and a last one of 16 B, about 200 entries in runs of
    1..4, the last block among them: with 1 or 3 workgroups each walks many
    runs."""
    field, k, p, elems, block_len, nb = 8, 10, 4, 300 * 48 + 16, 48, 301
    r = codec(field, k, p)
    clean = clean_shards(field, k, p, elems)
    rng = np.random.default_rng(300)
    updates = []
    for block in sorted(set(rng.choice(nb, 80, replace=False).tolist() + [0, nb - 1])):
        shards = sorted(rng.choice(k, int(rng.integers(1, 5)), replace=False).tolist())
        updates += [(block, i) for i in shards]
    assert 150 <= len(updates) <= 330
    new = new_bytes(len(updates), field, elems, block_len, rng)
    got, result, name = with_grid(grid, lambda: run(r, elems, block_len, clean, updates, new))
    assert name == "update-shards gf8 10+4 vec"
    assert result == USM.expected_result(updates, elems, block_len, k)
    assert np.array_equal(got, USM.apply(field, k, p, clean, block_len, updates, new))


@pytest.mark.parametrize("grid", [1, 3])
def test_grid_stride_over_many_spans(grid):
    """A block of 256 KiB + 16 (65 spans, the last one of 16 bytes) and a last
    block of 4 KiB + 32 (2 of its 65 items have bytes), three entries in each,
    walked by 1 or 3 workgroups."""
    field, k, p, block_len = 8, 10, 4, 256 * 1024 + 16
    elems = block_len + 4096 + 32
    r = codec(field, k, p)
    clean = clean_shards(field, k, p, elems)
    rng = np.random.default_rng(65)
    updates = [(0, 0), (0, 4), (0, 9), (1, 1), (1, 4), (1, 8)]
    new = new_bytes(len(updates), field, elems, block_len, rng)
    got, result, name = with_grid(grid, lambda: run(r, elems, block_len, clean, updates, new))
    assert name == "update-shards gf8 10+4 vec"
    assert result == [0, 2]
    assert np.array_equal(got, USM.apply(field, k, p, clean, block_len, updates, new))


def test_two_streams():
    """Two calls queued back to back on two streams over disjoint shards with
    different lists: both right."""
    field, k, p, elems, block_len = 8, 10, 4, 3 * 4112 + 32, 4112
    r = codec(field, k, p)
    clean = clean_shards(field, k, p, elems)
    rng = np.random.default_rng(2)
    lists = [make_list("mixed", k, 4, rng), make_list("per-block", k, 4, rng)]
    news = [new_bytes(len(u), field, elems, block_len, rng) for u in lists]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    queued = [run(r, elems, block_len, clean, u, nw, stream=s, sync=False)
              for u, nw, s in zip(lists, news, streams)]
    for (handles, name), u, nw, s in zip(queued, lists, news, streams):
        got, result = collect(handles, s)
        assert name == "update-shards gf8 10+4 vec"
        assert result == USM.expected_result(u, elems, block_len, k)
        assert np.array_equal(got, USM.apply(field, k, p, clean, block_len, u, nw))


@pytest.mark.parametrize("elems", [1024, 1000 + 37])
def test_block_len_0_on_one_flat_stripe_is_rse_update_flat(elems):
    """The shards as pointers into one stripe of the flat layout, one block:
    the same bytes and `result` as rse_update_flat on that stripe."""
    field, k, p = 8, 10, 4
    r = codec(field, k, p)
    clean = clean_shards(field, k, p, elems)
    rng = np.random.default_rng(elems)
    updates = [(0, 1), (0, 2), (0, 7)]
    new = new_bytes(len(updates), field, elems, 0, rng)
    before = make_inconsistent(clean, field, 0, updates, k, p, rng)
    upd = torch.tensor(updates, dtype=torch.int32, device="cuda")
    dnew = torch.from_numpy(new).cuda()
    st = torch.cuda.current_stream().cuda_stream
    outs = []
    for entry in ("shards", "flat"):
        dev = torch.from_numpy(np.array(before)).cuda()
        result = torch.full((2,), FILL32 - (1 << 32), dtype=torch.int32, device="cuda")
        if entry == "shards":
            ptrs, lens = pointer_arrays([dev[i] for i in range(k + p)], elems)
            rc = LIB.rse_update_shards(r._h, ptrs, lens, k + p, 0, upd.data_ptr(), dnew.data_ptr(),
                                       len(updates), result.data_ptr(), st)
        else:
            rc = LIB.rse_update_flat(r._h, dev.data_ptr(), elems, 1, upd.data_ptr(),
                                     dnew.data_ptr(), len(updates), result.data_ptr(), st)
        assert rc == 0
        torch.cuda.synchronize()
        outs.append((dev.cpu().numpy(), result.cpu().tolist()))
    assert outs[0][1] == outs[1][1] == [0, 1]
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][0], USM.apply(field, k, p, before, 0, updates, new))


def test_write_update_scrub_in_place():
    """A flipped byte of data shard 7 in block 2, then an update of shards 2 and
    3 of that block (and of shard 0 of the shorter last block): the scrub
    reports block 2 CORRECTED with shard 7 alone changed, and afterwards every
    block verifies, with the parity of the oracle's encode of the new data."""
    field, k, p, elems, block_len = 8, 10, 4, 4096 + 48, 1024
    r = codec(field, k, p)
    clean = clean_shards(field, k, p, elems)
    rng = np.random.default_rng(7)
    before = np.array(clean)
    before[7, 2 * 1024 + 123] ^= 0x81
    updates = [(2, 2), (2, 3), (4, 0)]
    new = new_bytes(len(updates), field, elems, block_len, rng)
    data = torch.from_numpy(before[:k]).cuda()    # [k, L]
    parity = torch.from_numpy(before[k:]).cuda()  # [p, L]
    shards = [data[i] for i in range(k)] + [parity[j] for j in range(p)]
    result = r.update(shards, block_len, updates, torch.from_numpy(new).cuda())
    torch.cuda.synchronize()
    assert result.cpu().tolist() == [0, 2]
    assert not r.verify(shards)
    status, changed, counts, bad, n_bad = r.scrub(shards, block_len)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [R.CORRECT_CLEAN, R.CORRECT_CLEAN, R.CORRECT_CORRECTED,
                                     R.CORRECT_CLEAN, R.CORRECT_CLEAN]
    only7 = [1 if i == 7 else 0 for i in range(k + p)]
    assert changed.cpu().tolist() == [[0] * (k + p)] * 2 + [only7] + [[0] * (k + p)] * 2
    assert n_bad.cpu().tolist() == [1] and bad.cpu().tolist()[:1] == [2]
    assert counts.cpu().tolist()[2] == [1, 0]
    want = np.array(clean)
    want[2, 2048:3072], want[3, 2048:3072], want[0, 4096:] = new[0], new[1], new[2, :48]
    USM.encode(field, k, p, want)
    got = np.concatenate([data.cpu().numpy(), parity.cpu().numpy()])
    assert np.array_equal(got, want)
    status, _, _, _, n_bad = r.scrub(shards, block_len)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [R.CORRECT_CLEAN] * 5 and n_bad.cpu().tolist() == [0]
    assert r.verify(shards)


@pytest.mark.parametrize("field", [8, 16])
def test_python_wrapper_host_list_and_device_tensor_agree(field):
    k, p, elems, block_len = 10, 4, 2 * 520 + 24, 520
    r = codec(field, k, p)
    clean = clean_shards(field, k, p, elems)
    rng = np.random.default_rng(field)
    updates = make_list("mixed", k, 3, rng)
    new = new_bytes(len(updates), field, elems, block_len, rng)
    want = USM.apply(field, k, p, clean, block_len, updates, new)
    dnew = torch.from_numpy(new).cuda()
    a = torch.from_numpy(np.array(clean)).cuda()
    b = torch.from_numpy(np.array(clean)).cuda()
    dupd = torch.tensor(updates, dtype=torch.int32, device="cuda")
    res_a = r.update([a[i] for i in range(k + p)], block_len, updates, dnew)
    res_b = r.update([b[i] for i in range(k + p)], block_len, dupd, dnew)
    assert res_a.shape == res_b.shape == (2,) and res_a.dtype == torch.int32 and res_a.is_cuda
    torch.cuda.synchronize()
    assert res_a.cpu().tolist() == res_b.cpu().tolist() == \
        USM.expected_result(updates, elems, block_len, k)
    assert np.array_equal(a.cpu().numpy(), want) and np.array_equal(b.cpu().numpy(), want)
    # a rejected list comes back in `result`, not as an exception
    rows = [a[i] for i in range(k + p)]
    bad = r.update(rows, block_len, [(1, 0), (0, 0)], dnew[:2])
    torch.cuda.synchronize()
    assert bad.cpu().tolist() == [R.UPDATE_REJECTED, 1]
    assert np.array_equal(a.cpu().numpy(), want)
    # the argument checks of update_flat()
    with pytest.raises(ValueError):
        r.update(rows, block_len, updates, dnew.to(torch.int8))
    with pytest.raises(ValueError):
        r.update(rows, block_len, updates, dnew.t())
    with pytest.raises(ValueError):
        r.update(rows, block_len, updates, dnew.cpu())
    with pytest.raises(ValueError):
        r.update(rows, block_len, updates, dnew[:-1])
    with pytest.raises(ValueError):
        r.update(rows, block_len, updates + [(2, 9)], dnew)  # one row of new_data too few
    with pytest.raises(ValueError):
        r.update(rows, block_len, dupd.to(torch.int64), dnew)
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy(), want)
