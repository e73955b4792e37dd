"""rse_read_flat on the GPU: shards read into the caller's rows, the erased
ones rebuilt on the way from the first k present shards of their stripe.

Expected rows, classes and `result` come from tests/read_model.py -- the
ORACLE's reconstruct of a copy of the stripe -- and whole buffers are compared:
`out` has a guard row past n_reads and a sentinel fill, so the rows of lost
entries and the guard must keep their bytes; `status` has a guard entry too;
`result` starts as 0xA5A5A5A5; `stripes` (6 stripes and a guard stripe) must be
byte-identical after the call.  rse_last_kernel() must name the route the plan
predicts.  A GF(2^16) stripe is handled as its bytes: 2 x shard_len per shard.
"""
import numpy as np
import pytest
import torch

import reed_solomon_erasure as R
from reed_solomon_erasure._lib import load

import read_model as RM

pytestmark = pytest.mark.gpu

LIB = load()
NS = 6
FILL32 = 0xA5A5A5A5
OUT_FILL, STATUS_FILL = 0xC3, 0xEE
GRID_X = 2  # RSE_OPT_GRID_X (include/rse_hip_tune.h)

# (field, k, p); 4+20: a stripe read whole is two output groups
CODECS = [(8, 3, 2), (8, 10, 4), (8, 4, 20), (8, 40, 3), (8, 128, 128), (16, 10, 4), (16, 100, 28)]
BYTES = [1, 15, 16, 17, 4096, 4096 + 16, 4096 + 37, 2 * 4096 + 48]
WIDE_BYTES = [16, 4096 + 16]  # of 128+128 and 100+28
SHAPES = [(f, k, p, b) for f, k, p in CODECS
          for b in (WIDE_BYTES if k + p > 100 else BYTES) if b % (f // 8) == 0]
LISTS = ("one-erased", "everything", "mixed", "erased-parity")

_CLEAN = {}


def codec(field, k, p):
    return (R.galois_16 if field == 16 else R.galois_8).ReedSolomon(k, p)


def clean_stripes(field, k, p, nbytes, n=NS):
    """n consistent stripes (parity by the ORACLE) and a guard stripe of random
    bytes, (n + 1, k + p, nbytes); computed once per shape, never modified."""
    key = (field, k, p, nbytes, n)
    if key not in _CLEAN:
        rng = np.random.default_rng(1000003 * field + 4099 * k + 17 * p + nbytes + n)
        buf = rng.integers(0, 256, (n + 1, k + p, nbytes), dtype=np.uint8)
        RM.encode(field, k, p, buf, n)
        buf.setflags(write=False)
        _CLEAN[key] = buf
    return _CLEAN[key]


def flag_rows(k, p, rng):
    """The six flag rows of a case, one per stripe: nothing erased; one data
    shard; p erased, data and parity mixed; p + 1 erased (past repair); all
    data erased (k <= p; else the first p data shards); only parity erased."""
    T = k + p
    rows = np.ones((NS, T), np.uint8)
    rows[1, int(rng.integers(k))] = 0
    n_data = max(1, min(k, p) // 2) if p > 1 else 1
    mixed = rng.choice(k, n_data, replace=False).tolist()
    mixed += (k + rng.choice(p, p - n_data, replace=False)).tolist() if p > n_data else []
    rows[2, mixed] = 0
    rows[3, rng.choice(T, p + 1, replace=False)] = 0
    rows[4, :min(k, p)] = 0
    rows[5, k + rng.choice(p, max(1, p // 2), replace=False)] = 0
    assert (rows == 0).sum(axis=1).tolist() == [0, 1, p, p + 1, min(k, p), max(1, p // 2)]
    # other non-zero values mean present too
    rows[rows != 0] = rng.integers(1, 256, int((rows != 0).sum()), dtype=np.uint8)
    return rows


def make_list(which, k, p, present, rng):
    T = k + p
    if which == "one-erased":
        return [(1, int(np.flatnonzero(present[1, :k] == 0)[0]))]
    if which == "everything":
        return [(s, i) for s in range(NS) for i in range(T)]
    if which == "erased-parity":
        return [(s, int(i)) for s in (2, 3, 5) for i in np.flatnonzero(present[s] == 0) if i >= k]
    out = []  # erased and present shards mixed, stripe 0 and 4 skipped... and 3 lost
    for stripe in (1, 2, 3, 5):
        erased = np.flatnonzero(present[stripe] == 0).tolist()
        there = np.flatnonzero(present[stripe] != 0).tolist()
        pick = set(rng.choice(erased, min(len(erased), 3), replace=False).tolist())
        pick |= set(rng.choice(there, min(len(there), 2), replace=False).tolist())
        out += [(stripe, int(i)) for i in sorted(pick)]
    return out


def offset_copy(host, off, fill=0):
    """`host` in HBM starting `off` bytes into its allocation."""
    flat = np.array(host).reshape(-1)  # a writable copy: the shared stripes are read-only
    buf = torch.full((flat.size + 64,), fill, dtype=torch.uint8, device="cuda")
    view = buf[off:off + flat.size]
    view.copy_(torch.from_numpy(flat))
    return view


def with_erased(stripes, present, fill, rng=None):
    """The stripes with every erased shard's buffer zeroed or filled with garbage."""
    out = np.array(stripes)
    for s, i in np.argwhere(present == 0):
        out[s, i] = 0 if fill == "zeros" else rng.integers(0, 256, out.shape[2], dtype=np.uint8)
    return out


def run(r, elems, stripes, present, reads, n_stripes=NS, stripes_off=0, out_off=0, stream=None,
        sync=True):
    """rse_read_flat through the C entry on a copy of `stripes` in HBM.  Returns
    (out with its guard row, status with its guard entry, result words, kernel
    name); `stripes` is checked to be what it was."""
    stream = stream or torch.cuda.current_stream()
    n = len(reads)
    nbytes = stripes.shape[2]
    with torch.cuda.stream(stream):
        dev = offset_copy(stripes, stripes_off)
        out = offset_copy(np.full((n + 1, nbytes), OUT_FILL, np.uint8), out_off, OUT_FILL)
        dpres = None if present is None else torch.from_numpy(np.array(present)).cuda()
        lst = torch.from_numpy(np.array(reads, dtype=np.uint32).reshape(-1, 2).view(np.int32)).cuda()
        status = torch.full((n + 1,), STATUS_FILL, dtype=torch.uint8, device="cuda")
        result = torch.full((2,), FILL32 - (1 << 32), dtype=torch.int32, device="cuda")
    rc = LIB.rse_read_flat(r._h, dev.data_ptr(), elems, n_stripes,
                           None if dpres is None else dpres.data_ptr(), lst.data_ptr(), n,
                           out.data_ptr(), status.data_ptr(), result.data_ptr(),
                           stream.cuda_stream)
    name = LIB.rse_last_kernel().decode()
    assert rc == 0
    handles = (dev, out, status, result, dpres, lst, np.array(stripes), n, nbytes)
    if not sync:
        return handles, name
    return (*collect(handles, stream), name)


def collect(handles, stream):
    dev, out, status, result, _, _, stripes, n, nbytes = handles
    stream.synchronize()
    assert np.array_equal(dev.cpu().numpy().reshape(stripes.shape), stripes), "stripes were written"
    return (out.cpu().numpy().reshape(n + 1, nbytes), status.cpu().numpy(),
            [int(v) & 0xFFFFFFFF for v in result.cpu().tolist()])


def wanted(model, n, nbytes):
    """The whole `out` and `status` buffers the model expects, guards included."""
    rows, status, result = model
    out = np.full((n + 1, nbytes), OUT_FILL, np.uint8)
    st = np.full(n + 1, STATUS_FILL, np.uint8)
    for u, row in enumerate(rows):
        if row is not None:
            out[u] = row
        if status is not None:
            st[u] = status[u]
    return out, st, result


def check(got, model, n, nbytes, what=""):
    out, status, result = got
    want_out, want_status, want_result = wanted(model, n, nbytes)
    assert result == want_result, what
    assert np.array_equal(status, want_status), (what, status.tolist(), want_status.tolist())
    assert np.array_equal(out, want_out), (what, np.argwhere(out != want_out)[:4].tolist())


def predicted_name(field, k, p, nbytes, stripes_off=0, out_off=0):
    # torch's allocations start on a multiple of 16: the offsets decide
    vec = stripes_off % 16 == 0 and out_off % 16 == 0 and nbytes % 16 == 0
    return "read gf%d %d+%d %s" % (field, k, p, "vec" if vec else "bytes")


@pytest.mark.parametrize("field,k,p,nbytes", SHAPES,
                         ids=["gf%d-%d+%d-%d" % s for s in SHAPES])
def test_lists_over_the_flag_rows(field, k, p, nbytes):
    """Every list on stripes whose erased buffers hold zeros, and -- the
    results must not change -- garbage."""
    r = codec(field, k, p)
    elems = nbytes // (field // 8)
    clean = clean_stripes(field, k, p, nbytes)
    rng = np.random.default_rng(7 * nbytes + 31 * k + p)
    present = flag_rows(k, p, rng)
    zeros = with_erased(clean, present, "zeros")
    garbage = with_erased(clean, present, "garbage", rng)
    for which in LISTS:
        reads = make_list(which, k, p, present, rng)
        assert RM.first_offender(reads, NS, k + p) is None
        model = RM.expected(field, k, p, clean, present, reads, NS)
        assert model[2][0] == RM.SERVED
        if which == "everything":  # every class occurs, and stripe 3 is past repair
            assert set(model[1]) == {RM.COPIED, RM.REBUILT, RM.LOST}
            assert model[2][1] == p + 1
        for start, stripes in (("zeros", zeros), ("garbage", garbage)):
            *got, name = run(r, elems, stripes, present, reads)
            assert name == predicted_name(field, k, p, nbytes), (which, start)
            check(got, model, len(reads), nbytes, (which, start))


def test_stripes_that_are_not_codewords_pin_the_inputs():
    """One data shard erased in 10+4: the valid set is the nine other data
    shards and parity 0.  A byte flipped in a shard of the valid set changes the
    rebuilt bytes; one flipped in a present shard outside it does not."""
    field, k, p, nbytes = 8, 10, 4, 4096 + 16
    r = codec(field, k, p)
    clean = clean_stripes(field, k, p, nbytes)
    present = np.ones((NS, k + p), np.uint8)
    present[:, 4] = 0
    reads = [(s, i) for s in range(NS) for i in (4, k + 2)]
    base = RM.expected(field, k, p, clean, present, reads, NS)
    inside, outside = np.array(clean), np.array(clean)
    inside[2, k, 100] ^= 0x40       # parity 0: the last shard of the valid set
    inside[3, 7, nbytes - 1] ^= 1   # a data shard of it
    outside[2, k + 1, 100] ^= 0x40  # parity 1 and 3: present, not among the first k
    outside[3, k + 3, nbytes - 1] ^= 1
    m_in = RM.expected(field, k, p, inside, present, reads, NS)
    m_out = RM.expected(field, k, p, outside, present, reads, NS)
    for u, (s, i) in enumerate(reads):
        if i == 4:
            assert np.array_equal(m_out[0][u], base[0][u])
            assert np.array_equal(m_in[0][u], base[0][u]) == (s not in (2, 3))
    for stripes, model, what in ((inside, m_in, "inside"), (outside, m_out, "outside")):
        *got, _ = run(r, nbytes, stripes, present, reads)
        check(got, model, len(reads), nbytes, what)


def test_null_present_copies_everything():
    field, k, p, nbytes = 8, 10, 4, 4096 + 37
    r = codec(field, k, p)
    clean = clean_stripes(field, k, p, nbytes)
    reads = [(0, 0), (0, 13), (2, 5), (5, 9), (5, 10)]
    *got, name = run(r, nbytes, clean, None, reads)
    assert name == "read gf8 10+4 bytes"
    assert got[1][:-1].tolist() == [RM.COPIED] * len(reads) and got[2] == [0, 0]
    check(got, RM.expected(field, k, p, clean, None, reads, NS), len(reads), nbytes)
    for u, (s, i) in enumerate(reads):
        assert np.array_equal(got[0][u], clean[s, i])


@pytest.mark.parametrize("stripes_off,out_off,nbytes", [(1, 0, 1024), (0, 8, 1024), (0, 0, 1023)],
                         ids=["stripes+1", "out+8", "odd-length"])
def test_misaligned_bases_take_the_byte_route(stripes_off, out_off, nbytes):
    field, k, p = 8, 10, 4
    r = codec(field, k, p)
    clean = clean_stripes(field, k, p, nbytes)
    rng = np.random.default_rng(91)
    present = flag_rows(k, p, rng)
    reads = make_list("mixed", k, p, present, rng)
    model = RM.expected(field, k, p, clean, present, reads, NS)
    *got, name = run(r, nbytes, clean, present, reads, stripes_off=stripes_off, out_off=out_off)
    assert name == "read gf8 10+4 bytes"
    check(got, model, len(reads), nbytes)
    if nbytes % 16 == 0:
        *aligned, name_a = run(r, nbytes, clean, present, reads)
        assert name_a == "read gf8 10+4 vec"
        assert np.array_equal(aligned[0], got[0]) and np.array_equal(aligned[1], got[1])


BASE = [(0, 1), (0, 13), (1, 2), (2, 0), (2, 5), (4, 9), (5, 0)]


def rejected_lists():
    swapped = list(BASE)
    swapped[3], swapped[4] = swapped[4], swapped[3]
    return [
        ("stripe-is-n_stripes", BASE + [(NS, 0)], 7),
        ("shard-is-k+p", BASE[:5] + [(4, 14)] + BASE[6:], 5),
        ("shard-is-all-ones", BASE[:6] + [(5, 0xFFFFFFFF)], 6),
        ("duplicate", BASE[:2] + [BASE[1]] + BASE[2:], 2),
        ("descending-shards", swapped, 4),
        ("descending-stripes", [(0, 1), (1, 2), (0, 13)] + BASE[3:], 2),
        ("offender-first", [(NS + 3, 0)] + BASE, 0),
        ("offender-last", BASE + [(5, 0)], 7),
    ]


@pytest.mark.parametrize("reads,offender", [pytest.param(u, o, id=n)
                                            for n, u, o in rejected_lists()])
def test_rejected_lists_write_nothing(reads, offender):
    field, k, p, nbytes = 8, 10, 4, 1024
    r = codec(field, k, p)
    clean = clean_stripes(field, k, p, nbytes)
    present = flag_rows(k, p, np.random.default_rng(5))
    assert RM.first_offender(BASE, NS, k + p) is None
    model = RM.expected(field, k, p, clean, present, reads, NS)
    assert model[2] == [RM.REJECTED, offender]
    *got, _ = run(r, nbytes, clean, present, reads)
    assert got[2] == [1, offender]
    assert (got[0] == OUT_FILL).all(), "a rejected list wrote rows"
    assert (got[1] == STATUS_FILL).all(), "a rejected list wrote classes"
    check(got, model, len(reads), nbytes)


def with_grid(grid, fn):
    old = LIB.rse_get_option(GRID_X)
    assert LIB.rse_set_option(GRID_X, grid) == 0
    try:
        return fn()
    finally:
        LIB.rse_set_option(GRID_X, old)


@pytest.mark.parametrize("grid", [1, 3])
def test_grid_stride_over_many_runs(grid):
    """64 stripes of 10+4 x 16 B, a run in every stripe: with 1 or 3 workgroups
    each walks many runs."""
    field, k, p, nbytes, n = 8, 10, 4, 16, 64
    r = codec(field, k, p)
    clean = clean_stripes(field, k, p, nbytes, n)
    rng = np.random.default_rng(64)
    present = np.ones((n, k + p), np.uint8)
    reads = []
    for s in range(n):
        erased = rng.choice(k + p, int(rng.integers(0, p + 2)), replace=False)
        present[s, erased] = 0
        reads += [(s, int(i)) for i in sorted(rng.choice(k + p, int(rng.integers(1, 5)),
                                                         replace=False).tolist())]
    model = RM.expected(field, k, p, clean, present, reads, n)
    assert {RM.COPIED, RM.REBUILT, RM.LOST} == set(model[1])
    *got, name = with_grid(grid, lambda: run(r, nbytes, clean, present, reads, n_stripes=n))
    assert name == "read gf8 10+4 vec"
    check(got, model, len(reads), nbytes)


@pytest.mark.parametrize("grid", [1, 3])
def test_grid_stride_over_many_spans(grid):
    """One stripe of 10+4 x (40 spans + 37 B) with two shards erased: 41 spans,
    the last one of 37 bytes, walked by 1 or 3 workgroups."""
    field, k, p, nbytes, n = 8, 10, 4, 40 * 4096 + 37, 1
    r = codec(field, k, p)
    clean = clean_stripes(field, k, p, nbytes, n)
    present = np.ones((n, k + p), np.uint8)
    present[0, [3, 11]] = 0
    reads = [(0, 0), (0, 3), (0, 11)]
    model = RM.expected(field, k, p, clean, present, reads, n)
    assert model[1] == [RM.COPIED, RM.REBUILT, RM.REBUILT]
    *got, name = with_grid(grid, lambda: run(r, nbytes, clean, present, reads, n_stripes=n))
    assert name == "read gf8 10+4 bytes"
    check(got, model, len(reads), nbytes)


def test_two_streams_read_the_same_stripes():
    """Two calls with different lists queued on two streams over the SAME
    stripes, which nobody writes: both right."""
    field, k, p, nbytes = 8, 10, 4, 2 * 4096 + 48
    r = codec(field, k, p)
    clean = clean_stripes(field, k, p, nbytes)
    rng = np.random.default_rng(2)
    present = flag_rows(k, p, rng)
    lists = [make_list("mixed", k, p, present, rng), make_list("everything", k, p, present, rng)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    dev = torch.from_numpy(np.array(clean)).cuda()
    dpres = torch.from_numpy(present).cuda()
    bufs = []
    for reads in lists:
        n = len(reads)
        bufs.append((torch.tensor(reads, dtype=torch.int32, device="cuda"),
                     torch.full(((n + 1) * nbytes,), OUT_FILL, dtype=torch.uint8, device="cuda"),
                     torch.full((n + 1,), STATUS_FILL, dtype=torch.uint8, device="cuda"),
                     torch.full((2,), FILL32 - (1 << 32), dtype=torch.int32, device="cuda")))
    torch.cuda.synchronize()
    for (lst, out, status, result), reads, s in zip(bufs, lists, streams):
        assert LIB.rse_read_flat(r._h, dev.data_ptr(), nbytes, NS, dpres.data_ptr(),
                                 lst.data_ptr(), len(reads), out.data_ptr(), status.data_ptr(),
                                 result.data_ptr(), s.cuda_stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy(), clean)
    for (lst, out, status, result), reads in zip(bufs, lists):
        got = (out.cpu().numpy().reshape(len(reads) + 1, nbytes), status.cpu().numpy(),
               [int(v) & 0xFFFFFFFF for v in result.cpu().tolist()])
        check(got, RM.expected(field, k, p, clean, present, reads, NS), len(reads), nbytes)


def test_round_trip_of_a_failed_device():
    """Encode, lose data shard 3 of every stripe (garbage over its buffer, its
    flag 0), read it for every stripe: the rows are the original data, and the
    stripes with the rows copied back verify."""
    field, k, p, nbytes, lost = 8, 10, 4, 4096 + 16, 3
    r = codec(field, k, p)
    rng = np.random.default_rng(11)
    host = rng.integers(0, 256, (NS, k + p, nbytes), dtype=np.uint8)
    dev = torch.from_numpy(host).cuda()
    r.encode_flat(dev.view(-1), nbytes, NS)
    original = dev[:, lost].clone()
    dev[:, lost] = torch.from_numpy(rng.integers(0, 256, (NS, nbytes), dtype=np.uint8)).cuda()
    present = torch.ones((NS, k + p), dtype=torch.uint8, device="cuda")
    present[:, lost] = 0
    out, status, result = r.read_flat(dev.view(-1), nbytes, NS, present, [(s, lost) for s in range(NS)])
    torch.cuda.synchronize()
    assert result.cpu().tolist() == [R.READ_SERVED, 0]
    assert status.cpu().tolist() == [R.READ_REBUILT] * NS
    assert torch.equal(out.view(NS, nbytes), original)
    assert np.array_equal(original.cpu().numpy(), host[:, lost])
    assert r.verify_flat(dev.view(-1), nbytes, NS).tolist() == [False] * NS
    dev[:, lost] = out.view(NS, nbytes)
    assert r.verify_flat(dev.view(-1), nbytes, NS).tolist() == [True] * NS


@pytest.mark.parametrize("field", [8, 16])
def test_python_wrapper_host_list_and_device_tensor_agree(field):
    k, p, nbytes = 10, 4, 1040
    r = codec(field, k, p)
    elems = nbytes // (field // 8)
    clean = clean_stripes(field, k, p, nbytes)
    rng = np.random.default_rng(field)
    present = flag_rows(k, p, rng)
    reads = make_list("mixed", k, p, present, rng)
    model = RM.expected(field, k, p, clean, present, reads, NS)
    dev = torch.from_numpy(np.array(clean)).cuda()
    dpres = torch.from_numpy(present).cuda()
    dlist = torch.tensor(reads, dtype=torch.int32, device="cuda")
    mine = torch.full((len(reads) * nbytes,), OUT_FILL, dtype=torch.uint8, device="cuda")
    out_a, st_a, res_a = r.read_flat(dev.view(-1), elems, NS, dpres, reads, out=mine)
    out_b, st_b, res_b = r.read_flat(dev.view(-1), elems, NS, dpres, dlist)
    assert out_a is mine and out_b.numel() == len(reads) * nbytes and out_b.is_cuda
    assert st_a.shape == st_b.shape == (len(reads),) and st_a.dtype == torch.uint8
    assert res_a.shape == res_b.shape == (2,) and res_a.dtype == torch.int32
    torch.cuda.synchronize()
    assert res_a.cpu().tolist() == res_b.cpu().tolist() == model[2]
    assert st_a.cpu().tolist() == st_b.cpu().tolist() == model[1]
    a, b = out_a.cpu().numpy().reshape(-1, nbytes), out_b.cpu().numpy().reshape(-1, nbytes)
    for u, row in enumerate(model[0]):
        if row is not None:  # a lost entry's row of a fresh buffer holds anything
            assert np.array_equal(a[u], row) and np.array_equal(b[u], row)
        else:
            assert (a[u] == OUT_FILL).all()
    assert np.array_equal(dev.cpu().numpy(), clean)
    # a rejected list comes back in `result`, not as an exception
    _, _, bad = r.read_flat(dev.view(-1), elems, NS, dpres, [(1, 0), (0, 0)])
    torch.cuda.synchronize()
    assert bad.cpu().tolist() == [R.READ_REJECTED, 1]
    assert R.READ_SERVED == 0 and (R.READ_COPIED, R.READ_REBUILT, R.READ_LOST) == (0, 1, 2)
