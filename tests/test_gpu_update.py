"""rse_update_flat on the GPU: data shards rewritten in place, the parity
patched by the delta.

Expected bytes come from tests/update_model.py -- the ORACLE's encode of the
difference, XORed into the parity that was there -- and the whole buffer is
compared: 6 stripes and a guard stripe that must keep its bytes.  new_data is
compared with itself afterwards (it is only read); `result` starts as
0xA5A5A5A5.  Every list runs on consistent stripes (parity by the oracle) and
on stripes made inconsistent first: the syndrome must be preserved, not
repaired and not sealed in.  rse_last_kernel() must name the path the plan
predicts.  A GF(2^16) stripe is handled as its bytes: 2 x shard_len per shard.
"""
import numpy as np
import pytest
import torch

import reed_solomon_erasure as R
from oracle import oracle as O
from reed_solomon_erasure._lib import load

import update_model as UM

pytestmark = pytest.mark.gpu

LIB = load()
NS = 6
FILL32 = 0xA5A5A5A5
GRID_X = 2  # RSE_OPT_GRID_X (include/rse_hip_tune.h)

# (field, k, p, shard_len in elements)
SHAPES = [
    (8, 10, 4, 1), (8, 10, 4, 17),   # the byte path
    (8, 10, 4, 1024),
    (8, 10, 4, 4096 + 37),           # odd shard addresses in an aligned buffer
    (8, 10, 4, 16384 + 48),
    (8, 1, 1, 16),
    (8, 3, 2, 64),
    (8, 4, 20, 272),                 # two row groups, 16 + 4
    (8, 128, 128, 48),               # k + p = 256, eight groups, a run of 128
    (16, 10, 4, 9),                  # 18 bytes: the byte path
    (16, 20, 8, 1032),
    (16, 128, 128, 16),
]
LISTS = ("one", "per-stripe", "whole-stripe", "mixed")
CASES = [pytest.param(*shape, which, id="gf%d-%d+%d-%d-%s" % (*shape, which))
         for shape in SHAPES for which in LISTS]

_CLEAN = {}


def codec(field, k, p):
    return (R.galois_16 if field == 16 else R.galois_8).ReedSolomon(k, p)


def clean_stripes(field, k, p, elems, n=NS):
    """n consistent stripes (parity by the ORACLE) and a guard stripe of random
    bytes, (n + 1, k + p, bytes per shard); computed once per shape, never
    modified."""
    key = (field, k, p, elems, n)
    if key not in _CLEAN:
        rng = np.random.default_rng(1000003 * field + 4099 * k + 17 * p + elems + n)
        buf = rng.integers(0, 256, (n + 1, k + p, elems * (field // 8)), dtype=np.uint8)
        UM.encode(field, k, p, buf, n)
        buf.setflags(write=False)
        _CLEAN[key] = buf
    return _CLEAN[key]


def make_list(which, k, rng):
    if which == "one":
        return [(2, k // 2)]
    if which == "per-stripe":
        return [(s, (3 * s + 1) % k) for s in range(NS)]
    if which == "whole-stripe":
        return [(4, i) for i in range(k)]
    out = []  # runs of mixed length that include the first and the last stripe
    for stripe, length in zip((0, 2, 3, NS - 1), (1, 5, 3, 2)):
        shards = sorted(rng.choice(k, min(k, length), replace=False).tolist())
        out += [(stripe, i) for i in shards]
    return out


def make_inconsistent(before, updates, k, p, rng):
    """One stale parity byte in every touched stripe, and one wrong byte in a
    data shard of it that the list does not name (where there is one)."""
    out = np.array(before)
    nbytes = out.shape[2]
    for stripe in sorted({s for s, _ in updates}):
        out[stripe, k + int(rng.integers(p)), int(rng.integers(nbytes))] ^= 0x5A
        free = sorted(set(range(k)) - {i for s, i in updates if s == stripe})
        if free:
            out[stripe, free[int(rng.integers(len(free)))], int(rng.integers(nbytes))] ^= 0x3C
    return out


def new_bytes(n, nbytes, rng):
    return rng.integers(0, 256, (n, nbytes), dtype=np.uint8)


def offset_copy(host, off):
    """`host` in HBM starting `off` bytes into its allocation."""
    flat = np.array(host).reshape(-1)  # a writable copy: the shared stripes are read-only
    buf = torch.zeros(flat.size + 64, dtype=torch.uint8, device="cuda")
    view = buf[off:off + flat.size]
    view.copy_(torch.from_numpy(flat))
    return view


def run(r, elems, before, updates, new, n_stripes=NS, stripes_off=0, new_off=0, stream=None,
        sync=True):
    """rse_update_flat through the C entry on a copy of `before` in HBM.
    Returns (stripes after, result words, kernel name, device handles)."""
    stream = stream or torch.cuda.current_stream()
    with torch.cuda.stream(stream):
        dev = offset_copy(before, stripes_off)
        dnew = offset_copy(new, new_off)
        upd = torch.from_numpy(np.array(updates, dtype=np.uint32).reshape(-1, 2).view(np.int32)).cuda()
        result = torch.full((2,), FILL32 - (1 << 32), dtype=torch.int32, device="cuda")
    rc = LIB.rse_update_flat(r._h, dev.data_ptr(), elems, n_stripes, upd.data_ptr(),
                             dnew.data_ptr(), len(updates), result.data_ptr(),
                             stream.cuda_stream)
    name = LIB.rse_last_kernel().decode()
    assert rc == 0
    handles = (dev, dnew, upd, result, before.shape, np.array(new))
    if not sync:
        return handles, name
    return (*collect(handles, stream), name)


def collect(handles, stream):
    dev, dnew, upd, result, shape, new = handles
    stream.synchronize()
    assert np.array_equal(dnew.cpu().numpy().reshape(new.shape), new), "new_data was written"
    return dev.cpu().numpy().reshape(shape), [int(v) & 0xFFFFFFFF for v in result.cpu().tolist()]


def predicted_name(field, k, p, nbytes, stripes_off=0, new_off=0):
    # torch's allocations start on a multiple of 16: the offsets decide
    vec = stripes_off % 16 == 0 and new_off % 16 == 0 and nbytes % 16 == 0
    return "update gf%d %d+%d %s" % (field, k, p, "vec" if vec else "bytes")


@pytest.mark.parametrize("field,k,p,elems,which", CASES)
def test_accepted_lists(field, k, p, elems, which):
    r = codec(field, k, p)
    clean = clean_stripes(field, k, p, elems)
    nbytes = clean.shape[2]
    rng = np.random.default_rng(7 * elems + k + LISTS.index(which))
    updates = make_list(which, k, rng)
    assert UM.first_offender(updates, NS, k) is None
    new = new_bytes(len(updates), nbytes, rng)
    for start in ("consistent", "inconsistent"):
        before = clean if start == "consistent" else make_inconsistent(clean, updates, k, p, rng)
        want = UM.apply(field, k, p, before, updates, new, NS)
        got, result, name = run(r, elems, before, updates, new)
        assert name == predicted_name(field, k, p, nbytes), start
        assert result == UM.expected_result(updates, NS, k), start
        assert result == [0, len({s for s, _ in updates})], start
        assert np.array_equal(got, want), (start, np.argwhere(got != want)[:4].tolist())
        assert np.array_equal(got[NS], clean[NS]), "the guard stripe was written"
        if which == "whole-stripe" and start == "consistent":
            # every data shard new: the parity is a fresh oracle encode of the new data
            fresh = np.array(got[4:5])
            fresh[0, k:] = 0
            UM.encode(field, k, p, fresh, 1)
            assert np.array_equal(got[4], fresh[0])


@pytest.mark.parametrize("stripes_off,new_off", [(1, 0), (0, 8)], ids=["stripes+1", "new+8"])
def test_misaligned_bases_take_the_byte_path(stripes_off, new_off):
    field, k, p, elems = 8, 10, 4, 1024
    r = codec(field, k, p)
    clean = clean_stripes(field, k, p, elems)
    rng = np.random.default_rng(91)
    updates = make_list("mixed", k, rng)
    new = new_bytes(len(updates), elems, rng)
    aligned, res_a, name_a = run(r, elems, clean, updates, new)
    got, res, name = run(r, elems, clean, updates, new, stripes_off=stripes_off, new_off=new_off)
    assert name_a == "update gf8 10+4 vec" and name == "update gf8 10+4 bytes"
    assert res == res_a == UM.expected_result(updates, NS, k)
    assert np.array_equal(got, aligned)
    assert np.array_equal(got, UM.apply(field, k, p, clean, updates, new, NS))


BASE = [(0, 1), (0, 3), (1, 2), (2, 0), (2, 5), (4, 9), (5, 0)]


def rejected_lists():
    swapped = list(BASE)
    swapped[2], swapped[3] = swapped[3], swapped[2]
    two = list(BASE)
    two[2] = (1, 10)
    two[4], two[5] = two[5], two[4]
    return [
        ("swapped", swapped, 3),
        ("duplicate", BASE[:2] + [BASE[1]] + BASE[2:], 2),
        ("split-run", [(0, 1), (1, 2), (0, 3)] + BASE[3:], 2),
        ("stripe-is-n_stripes", BASE + [(NS, 0)], 7),
        ("shard-is-k", BASE[:5] + [(4, 10)] + BASE[6:], 5),
        ("shard-is-all-ones", BASE[:6] + [(5, 0xFFFFFFFF)], 6),
        ("two-defects", two, 2),
    ]


@pytest.mark.parametrize("updates,offender", [pytest.param(u, o, id=n)
                                              for n, u, o in rejected_lists()])
def test_rejected_lists_write_nothing(updates, offender):
    field, k, p, elems = 8, 10, 4, 1024
    r = codec(field, k, p)
    clean = clean_stripes(field, k, p, elems)
    assert UM.first_offender(BASE, NS, k) is None
    assert UM.expected_result(updates, NS, k) == [1, offender]
    new = new_bytes(len(updates), elems, np.random.default_rng(offender))
    got, result, _ = run(r, elems, clean, updates, new)
    assert result == [1, offender]
    assert np.array_equal(got, clean), "a rejected list wrote stripe bytes"


def with_grid(grid, fn):
    old = LIB.rse_get_option(GRID_X)
    assert LIB.rse_set_option(GRID_X, grid) == 0
    try:
        return fn()
    finally:
        LIB.rse_set_option(GRID_X, old)


@pytest.mark.parametrize("grid", [1, 3])
def test_grid_stride_over_many_runs(grid):
    """300 stripes of 10+4 x 48 B, about 200 entries in runs of 1..4: with 1 or
    3 workgroups each walks many runs."""
    field, k, p, elems, n = 8, 10, 4, 48, 300
    r = codec(field, k, p)
    clean = clean_stripes(field, k, p, elems, n)
    rng = np.random.default_rng(300)
    updates = []
    for stripe in sorted(rng.choice(n, 80, replace=False).tolist() + [0, n - 1]):
        if updates and updates[-1][0] == stripe:
            continue
        shards = sorted(rng.choice(k, int(rng.integers(1, 5)), replace=False).tolist())
        updates += [(stripe, i) for i in shards]
    assert 150 <= len(updates) <= 330
    new = new_bytes(len(updates), elems, rng)
    got, result, name = with_grid(grid, lambda: run(r, elems, clean, updates, new, n_stripes=n))
    assert name == "update gf8 10+4 vec"
    assert result == UM.expected_result(updates, n, k)
    assert np.array_equal(got, UM.apply(field, k, p, clean, updates, new, n))


@pytest.mark.parametrize("grid", [1, 3])
def test_grid_stride_over_many_spans(grid):
    """One stripe of 10+4 x (256 KiB + 16) with three entries: 65 spans, the
    last one of 16 bytes, walked by 1 or 3 workgroups."""
    field, k, p, elems, n = 8, 10, 4, 256 * 1024 + 16, 1
    r = codec(field, k, p)
    clean = clean_stripes(field, k, p, elems, n)
    rng = np.random.default_rng(65)
    updates = [(0, 0), (0, 4), (0, 9)]
    new = new_bytes(len(updates), elems, rng)
    got, result, name = with_grid(grid, lambda: run(r, elems, clean, updates, new, n_stripes=n))
    assert name == "update gf8 10+4 vec"
    assert result == [0, 1]
    assert np.array_equal(got, UM.apply(field, k, p, clean, updates, new, n))


def test_two_streams():
    """Two calls queued back to back on two streams over disjoint buffers with
    different lists: both right."""
    field, k, p, elems = 8, 10, 4, 16384 + 48
    r = codec(field, k, p)
    clean = clean_stripes(field, k, p, elems)
    rng = np.random.default_rng(2)
    lists = [make_list("mixed", k, rng), make_list("per-stripe", k, rng)]
    news = [new_bytes(len(u), elems, rng) for u in lists]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    queued = [run(r, elems, clean, u, nw, stream=s, sync=False)
              for u, nw, s in zip(lists, news, streams)]
    for (handles, name), u, nw, s in zip(queued, lists, news, streams):
        got, result = collect(handles, s)
        assert name == "update gf8 10+4 vec"
        assert result == UM.expected_result(u, NS, k)
        assert np.array_equal(got, UM.apply(field, k, p, clean, u, nw, NS))


def test_update_then_scrub_repairs_what_reencoding_would_have_sealed():
    """A flipped byte of data shard 7, then an update of shards 2 and 3: the
    stripe still fails the check, the scrub still repairs it, and the result is
    the oracle's encode of the new data with shard 7's original byte."""
    field, k, p, elems = 8, 10, 4, 4096
    r = codec(field, k, p)
    clean = clean_stripes(field, k, p, elems, 1)
    rng = np.random.default_rng(7)
    before = np.array(clean)
    before[0, 7, 1234] ^= 0x81
    new = new_bytes(2, elems, rng)
    dev = torch.from_numpy(before).cuda()
    result = r.update_flat(dev.view(-1), elems, 1, [(0, 2), (0, 3)], torch.from_numpy(new).cuda())
    torch.cuda.synchronize()
    assert result.cpu().tolist() == [0, 1]
    assert r.verify_flat(dev.view(-1), elems, 1).tolist() == [False]
    status, _, counts, _, n_bad = r.scrub_flat(dev.view(-1), elems, 1)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [R.CORRECT_CORRECTED]
    assert n_bad.cpu().tolist() == [1] and counts.cpu().tolist() == [[1, 0]]
    want = np.array(clean)
    want[0, 2], want[0, 3] = new[0], new[1]
    UM.encode(field, k, p, want, 1)
    got = dev.cpu().numpy()
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], clean[1]), "the guard stripe was written"
    assert r.verify_flat(dev.view(-1), elems, 1).tolist() == [True]


@pytest.mark.parametrize("field", [8, 16])
def test_python_wrapper_host_list_and_device_tensor_agree(field):
    k, p, elems = 10, 4, 1032
    r = codec(field, k, p)
    clean = clean_stripes(field, k, p, elems)
    nbytes = clean.shape[2]
    rng = np.random.default_rng(field)
    updates = make_list("mixed", k, rng)
    new = new_bytes(len(updates), nbytes, rng)
    want = UM.apply(field, k, p, clean, updates, new, NS)
    dnew = torch.from_numpy(new).cuda()
    a = torch.from_numpy(np.array(clean)).cuda()
    b = torch.from_numpy(np.array(clean)).cuda()
    dupd = torch.tensor(updates, dtype=torch.int32, device="cuda")
    res_a = r.update_flat(a.view(-1), elems, NS, updates, dnew)
    res_b = r.update_flat(b.view(-1), elems, NS, dupd, dnew)
    assert res_a.shape == res_b.shape == (2,) and res_a.dtype == torch.int32 and res_a.is_cuda
    torch.cuda.synchronize()
    assert res_a.cpu().tolist() == res_b.cpu().tolist() == UM.expected_result(updates, NS, k)
    assert np.array_equal(a.cpu().numpy(), want) and np.array_equal(b.cpu().numpy(), want)
    # a rejected list comes back in `result`, not as an exception
    bad = r.update_flat(a.view(-1), elems, NS, [(1, 0), (0, 0)], dnew)
    torch.cuda.synchronize()
    assert bad.cpu().tolist() == [R.UPDATE_REJECTED, 1]
    assert np.array_equal(a.cpu().numpy(), want)
