"""rse_scrub_flat on the GPU: rse_correct_flat's repair behind the check pass
of rse_verify_flat, and the ascending list of the stripes that did not end
CLEAN.

Every case runs on both routes, forced with RSE_OPT_SCRUB_ROUTE (0 direct, 2
pre-filter), and rse_last_kernel() must name the route.  Expected bytes are the
oracle's clean stripes wherever the injection is within a column's capacity
2 nu + f <= p.  Past it every column is held to the definition
(check_definition: a column either stays as it was and is still no codeword,
or has become a codeword within the capacity of what it was -- over the
ORACLE's check matrix, no decoder), and for 10+4 to the brute-force model of
tests/correct_model.py as tests/test_gpu_correct.py does.  status, changed,
counts and the list follow from before -> after.  Equality with
rse_correct_flat on a copy of the same buffer is checked in addition (GF(2^8):
rse_correct_flat refuses GF(2^16)), never alone.

Batches as tests/test_gpu_correct.py: 5 stripes and a guard stripe that must
keep its bytes; status, changed, counts with a spare row of 0xA5;
bad_stripes filled with 0xA5, which everything from n_bad on must keep.  A
GF(2^16) stripe is handled as its bytes: 2 x shard_len per shard.
"""

import numpy as np
import pytest
import torch

import reed_solomon_erasure as R
from oracle import oracle as O
from reed_solomon_erasure._lib import load

import correct_model as CM
import locate_model as LM
from conftest import kernels_or_skip
from test_gpu_correct import erase
from test_gpu_locate import NS, corrupt_shards, disjoint_columns, reference

pytestmark = pytest.mark.gpu

LIB = load()
CLEAN, CORRECTED, UNCORRECTABLE = 0, 1, 2
SCRUB_ROUTE = 56  # RSE_OPT_SCRUB_ROUTE
ROUTES = [(0, "direct"), (2, "prefilter")]
FILL32 = 0xA5A5A5A5

# (field, k, p, shard_len in elements): what the check pass runs on
SHAPES = [
    (8, 10, 4, 17),                  # tables only, byte-wise sweep
    (8, 10, 4, 1024),                # the 1 KiB sub-chunk check
    (8, 10, 4, 4096),
    (8, 10, 4, 4096 + 37),           # odd shard addresses
    (8, 10, 4, 16384 + 4096 + 48),   # a 16 KiB chunk, a 4 KiB chunk and a table-coded tail
    (8, 12, 4, 4096 + 16),           # a run-time codec: its module may not be built
    (8, 16, 16, 2048),               # the FFT check
    (8, 100, 16, 4096 + 16),
    (16, 20, 8, 2048 + 8), (16, 20, 8, 9), (16, 10, 4, 2048 + 8), (16, 10, 4, 9),
]
CASES = [pytest.param(*shape, *route, id="gf%d-%d+%d-%d-%s" % (*shape, route[1]))
         for shape in SHAPES for route in ROUTES]

_REF16 = {}
_HC = {}


def codec(field, k, p):
    return (R.galois_16 if field == 16 else R.galois_8).ReedSolomon(k, p)


def clean_stripes(field, k, p, elems):
    """NS clean stripes and a guard stripe as bytes, (NS + 1, k + p, bytes per
    shard), parity by the ORACLE; computed once per shape, never modified."""
    if field == 8:
        return reference(k, p, elems)
    key = (k, p, elems)
    if key not in _REF16:
        rng = np.random.default_rng(16000 * k + 10 * p + elems)
        buf = rng.integers(0, 256, (NS + 1, k + p, 2 * elems), dtype=np.uint8)
        oracle = O.Codec(16, k, p)
        for s in range(NS):
            oracle.encode([buf[s, i] for i in range(k + p)])
        buf.setflags(write=False)
        _REF16[key] = buf
    return _REF16[key]


def check_matrix(k, p):
    if (k, p) not in _HC:
        _HC[k, p] = LM.check_matrix(k, p)
    return _HC[k, p]


def scrub(field, k, p, elems, route, host, present=None, n_stripes=NS, r=None):
    """rse_scrub_flat through the C entry on a copy of `host` (n_stripes + 1
    stripes of bytes) in HBM on the forced route; checks the route's name, what
    must not have been written, the list against status, and for GF(2^8)
    everything against rse_correct_flat on another copy.  Returns (stripes,
    status, changed, counts) of the batch."""
    r = r or codec(field, k, p)
    n = k + p
    stream = torch.cuda.current_stream()
    with torch.cuda.stream(stream):
        dev = torch.from_numpy(np.array(host)).cuda()
        status = torch.full((n_stripes + 1,), 0xA5, dtype=torch.uint8, device="cuda")
        changed = torch.full((n_stripes + 1, n), 0xA5, dtype=torch.uint8, device="cuda")
        counts = torch.full((n_stripes + 1, 2), FILL32 - (1 << 32), dtype=torch.int32,
                            device="cuda")
        bad = torch.full((n_stripes + 1,), FILL32 - (1 << 32), dtype=torch.int32, device="cuda")
        n_bad = torch.full((2,), FILL32 - (1 << 32), dtype=torch.int32, device="cuda")
        pres = None
        if present is not None:
            pres = torch.from_numpy(np.ascontiguousarray(present, dtype=np.uint8)).cuda()
            assert tuple(pres.shape) == (n_stripes, n)
    pres_ptr = pres.data_ptr() if pres is not None else None
    old = LIB.rse_get_option(SCRUB_ROUTE)
    assert LIB.rse_set_option(SCRUB_ROUTE, route[0]) == 0
    try:
        rc = LIB.rse_scrub_flat(r._h, dev.data_ptr(), elems, n_stripes, pres_ptr,
                                status.data_ptr(), changed.data_ptr(), counts.data_ptr(),
                                bad.data_ptr(), n_bad.data_ptr(), stream.cuda_stream)
    finally:
        LIB.rse_set_option(SCRUB_ROUTE, old)
    assert rc == 0
    scrub.last_kernel = R.core.last_kernel()
    if route[1] is not None:  # None: the caller looks at scrub.last_kernel, the rule's route
        assert scrub.last_kernel == "scrub gf%d %d+%d %s" % (field, k, p, route[1])
    stream.synchronize()
    got = dev.cpu().numpy()
    assert (got[n_stripes] == host[n_stripes]).all(), "guard stripe"
    status, changed = status.cpu().numpy(), changed.cpu().numpy()
    counts = counts.cpu().numpy().view(np.uint32)
    bad, n_bad = bad.cpu().numpy().view(np.uint32), n_bad.cpu().numpy().view(np.uint32)
    assert status[n_stripes] == 0xA5 and (changed[n_stripes] == 0xA5).all()
    assert (counts[n_stripes] == FILL32).all() and n_bad[1] == FILL32
    if pres is not None:
        assert (pres.cpu().numpy() == np.asarray(present, np.uint8)).all(), "present is only read"
    # the list: exactly the stripes that did not end CLEAN, ascending, nothing past them
    listed = np.nonzero(status[:n_stripes])[0]
    assert n_bad[0] == len(listed), (int(n_bad[0]), listed[:8].tolist())
    assert (bad[:len(listed)] == listed).all()
    assert (bad[len(listed):] == FILL32).all(), "entries from n_bad on are not written"
    if field == 8:  # in addition: rse_correct_flat on the same input
        with torch.cuda.stream(stream):
            dev2 = torch.from_numpy(np.array(host)).cuda()
            out2 = (torch.empty((n_stripes,), dtype=torch.uint8, device="cuda"),
                    torch.empty((n_stripes, n), dtype=torch.uint8, device="cuda"),
                    torch.empty((n_stripes, 2), dtype=torch.int32, device="cuda"))
        assert LIB.rse_correct_flat(r._h, dev2.data_ptr(), elems, n_stripes, pres_ptr,
                                    out2[0].data_ptr(), out2[1].data_ptr(), out2[2].data_ptr(),
                                    stream.cuda_stream) == 0
        stream.synchronize()
        assert (dev2.cpu().numpy() == got).all(), "bytes as rse_correct_flat leaves them"
        assert (out2[0].cpu().numpy() == status[:n_stripes]).all()
        assert (out2[1].cpu().numpy() == changed[:n_stripes]).all()
        assert (out2[2].cpu().numpy().view(np.uint32) == counts[:n_stripes]).all()
    return got[:n_stripes], status[:n_stripes], changed[:n_stripes], counts[:n_stripes]


def check_definition(k, p, before, result, erased=None):
    """Every stripe against the entry's definition, from before -> after alone.
    A column that is no codeword afterwards was left as it was; every other
    column is a codeword that differs from what it was in nu shards outside
    the erased ones with 2 nu + f <= p.  status, changed and counts are those
    of exactly that.  A stripe with f > p is untouched and UNCORRECTABLE."""
    got, status, changed, counts = result
    hc = check_matrix(k, p)
    for s in range(len(got)):
        era = sorted(erased[s]) if erased else []
        diff = got[s] != before[s]
        assert (changed[s] == diff.any(axis=1)).all(), (s, changed[s].tolist())
        assert counts[s][0] == diff.sum(), (s, counts[s].tolist(), int(diff.sum()))
        if len(era) > p:
            assert not diff.any() and status[s] == UNCORRECTABLE and counts[s][1] == 0, s
            continue
        left = LM.gf_matvec(hc, got[s]).any(axis=0)  # columns that are no codeword now
        assert not diff[:, left].any(), (s, "an undecodable column was written")
        outside = np.delete(diff, era, axis=0).sum(axis=0)
        assert (2 * outside + len(era) <= p).all(), (s, int(outside.max()))
        assert counts[s][1] == left.sum(), (s, counts[s].tolist(), int(left.sum()))
        want = UNCORRECTABLE if left.any() else (CORRECTED if diff.any() else CLEAN)
        assert status[s] == want, (s, int(status[s]), want)


@pytest.mark.parametrize("field,k,p,elems,route,name", CASES)
def test_all_clean(field, k, p, elems, route, name):
    ref = clean_stripes(field, k, p, elems)
    result = scrub(field, k, p, elems, (route, name), ref)  # n_bad == 0: checked there
    assert (result[0] == ref[:NS]).all()
    assert not result[1].any() and not result[2].any() and not result[3].any()


@pytest.mark.parametrize("field,k,p,elems,route,name", CASES)
def test_errors(field, k, p, elems, route, name):
    """Stripe 0: one wrong byte in the first column.  1: a whole bad shard.
    2: disjoint wrong shards in different columns, p + 1 shards between them.
    3: t + 1 wrong shards in every column.  4: one wrong byte in the last
    column of the last stripe."""
    n, t = k + p, p // 2
    rng = np.random.default_rng(41)
    ref = clean_stripes(field, k, p, elems)
    length = ref.shape[2]
    buf = ref.copy()
    corrupt_shards(buf, rng, 0, [0], cols=[0])
    corrupt_shards(buf, rng, 1, [k // 2])
    sets, cols = disjoint_columns(k, p, length, rng, p + 1)
    for shards, col in zip(sets, cols):
        corrupt_shards(buf, rng, 2, shards, cols=[col])
    corrupt_shards(buf, rng, 3, [int(q) for q in rng.permutation(n)[:t + 1]])
    corrupt_shards(buf, rng, 4, [n - 1], cols=[length - 1])
    result = scrub(field, k, p, elems, (route, name), buf)
    got, status, changed, counts = result
    check_definition(k, p, buf, result)
    for s in (0, 1, 2, 4):
        assert (got[s] == ref[s]).all(), (s, "repaired stripes equal the oracle's encode")
    assert status.tolist() == [CORRECTED, CORRECTED, CORRECTED, UNCORRECTABLE, CORRECTED]
    assert counts[:, 0].tolist()[:3] == [1, length, p + 1] and counts[4].tolist() == [1, 0]
    assert np.nonzero(changed[1])[0].tolist() == [k // 2] and changed[2].sum() == p + 1
    if p == 4:  # the model, on the first columns
        mc = min(length, 64)
        code, want, bad = CM.correct_stripe(k, p, buf[3][:, :mc], [])
        assert code == UNCORRECTABLE and bad >= 1
        assert (got[3][:, :mc] == want).all() and counts[3][1] >= bad


@pytest.mark.parametrize("field,k,p,elems,route,name", CASES)
def test_erasures(field, k, p, elems, route, name):
    """Stripe 0: p erasures alone.  1: p - 2 erasures beside a wholly wrong
    shard.  2: p + 1 erasures (not touched).  3: erased flags on a stripe
    whose bytes already are a codeword: visited on the pre-filter route, CLEAN,
    not listed.  4: p + 1 erased flags on such a stripe: passes the check, and
    is UNCORRECTABLE, untouched and listed all the same."""
    n = k + p
    rng = np.random.default_rng(43)
    ref = clean_stripes(field, k, p, elems)
    buf = ref.copy()
    present = np.ones((NS, n), np.uint8)
    erase(buf, present, 0, [0, n - 1] + [int(q) for q in rng.permutation(np.arange(1, n - 1))[:p - 2]])
    perm = [int(q) for q in rng.permutation(n)]
    erase(buf, present, 1, perm[:p - 2])
    corrupt_shards(buf, rng, 1, perm[p - 2:p - 1])
    erase(buf, present, 2, [int(q) for q in rng.permutation(n)[:p + 1]])
    present[3, [1, n - 2]] = 0  # flagged, bytes as encoded
    present[4, [int(q) for q in rng.permutation(n)[:p + 1]]] = 0
    erased = [np.nonzero(present[s] == 0)[0].tolist() for s in range(NS)]
    result = scrub(field, k, p, elems, (route, name), buf, present)
    got, status, changed, counts = result
    check_definition(k, p, buf, result, erased)
    for s in (0, 1, 3, 4):
        assert (got[s] == ref[s]).all(), (s, "repaired stripes equal the oracle's encode")
    assert status.tolist() == [CORRECTED, CORRECTED, UNCORRECTABLE, CLEAN, UNCORRECTABLE]
    assert changed[0].sum() == p and changed[1].sum() == p - 1


def tiny_batch(n_stripes, bad):
    """n_stripes stripes (and a guard) of 10+4 x 17 bytes, the oracle's; one
    wrong byte in shard s % 14, column s % 17 of every stripe s in `bad`."""
    ref = reference(10, 4, 17)
    clean = ref[np.arange(n_stripes + 1) % NS]
    buf = clean.copy()
    bad = np.asarray(sorted(bad), np.int64)
    buf[bad, bad % 14, bad % 17] ^= ((bad % 255) + 1).astype(np.uint8)
    return clean, buf


@pytest.mark.parametrize("route,name", ROUTES)
@pytest.mark.parametrize("n_stripes,bad", [
    (300, [0, 1, 150, 298, 299]),  # ascending order, adjacency, both ends
    (300, range(300)),
    (70000, range(70000)),         # more entries than the sweep has workgroups, and more
                                   # stripes than one trip of the check's grid
    (70000, [3, 65538]),           # state carried between trips
], ids=["300-five", "300-all", "70000-all", "70000-two"])
def test_the_list(n_stripes, bad, route, name):
    clean, buf = tiny_batch(n_stripes, bad)
    got, status, changed, counts = scrub(8, 10, 4, 17, (route, name), buf, n_stripes=n_stripes)
    assert (got == clean[:n_stripes]).all()
    want = np.zeros(n_stripes, np.uint8)
    want[list(bad)] = CORRECTED
    assert (status == want).all()  # the list equals nonzero(status): checked in scrub()
    assert (counts[:, 0] == want).all() and not counts[:, 1].any()
    assert (changed.sum(axis=1) == want).all()


@pytest.mark.parametrize("route,name", ROUTES)
def test_two_calls_on_one_stream(route, name):
    """Back to back on one stream, the second on a clean buffer: the verdict
    words and the count belong to a call."""
    clean, buf = tiny_batch(300, range(0, 300, 7))
    r = codec(8, 10, 4)
    old = LIB.rse_get_option(SCRUB_ROUTE)
    assert LIB.rse_set_option(SCRUB_ROUTE, route) == 0
    try:
        first = r.scrub_flat(torch.from_numpy(buf).cuda(), 17, 300)
        dev = torch.from_numpy(clean.copy()).cuda()
        status, changed, counts, bad, n_bad = r.scrub_flat(dev, 17, 300)
    finally:
        LIB.rse_set_option(SCRUB_ROUTE, old)
    assert R.core.last_kernel() == "scrub gf8 10+4 " + name
    torch.cuda.synchronize()
    assert first[4].cpu().tolist() == [43] and first[3][:43].cpu().tolist() == list(range(0, 300, 7))
    assert n_bad.cpu().tolist() == [0] and not status.cpu().numpy().any()
    assert not changed.cpu().numpy().any() and not counts.cpu().numpy().any()
    assert (dev.cpu().numpy() == clean).all()
    assert bad.dtype == torch.int32 and tuple(bad.shape) == (300,) and tuple(n_bad.shape) == (1,)


@pytest.mark.parametrize("route,name", ROUTES)
def test_non_default_stream(route, name):
    rng = np.random.default_rng(47)
    ref = clean_stripes(8, 10, 4, 4096)
    buf = ref.copy()
    corrupt_shards(buf, rng, 3, [5, 12])
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        got, status, changed, counts = scrub(8, 10, 4, 4096, (route, name), buf)
    assert (got == ref[:NS]).all()
    assert status.tolist() == [CLEAN, CLEAN, CLEAN, CORRECTED, CLEAN]
    assert np.nonzero(changed[3])[0].tolist() == [5, 12] and counts[3].tolist() == [2 * 4096, 0]


def test_the_rule_names_its_route_and_null_lists():
    """By the rule (the default): a compiled codec pre-filters 4 KiB shards and
    takes the direct route at 17 bytes and at odd addresses.  bad_stripes and
    n_bad may each be NULL alone."""
    rng = np.random.default_rng(53)
    r = codec(8, 10, 4)
    assert LIB.rse_get_option(SCRUB_ROUTE) == 1
    for elems, name in ((4096, "prefilter"), (17, "direct"), (4096 + 37, "direct")):
        ref = clean_stripes(8, 10, 4, elems)
        buf = ref.copy()
        corrupt_shards(buf, rng, 1, [3], cols=[elems - 1])
        corrupt_shards(buf, rng, 4, [13], cols=[0])
        for lists in ((True, True), (True, False), (False, True), (False, False)):
            dev = torch.from_numpy(buf).cuda()
            status = torch.full((NS,), 0xA5, dtype=torch.uint8, device="cuda")
            bad = torch.full((NS,), -1, dtype=torch.int32, device="cuda")
            n_bad = torch.full((1,), -1, dtype=torch.int32, device="cuda")
            rc = LIB.rse_scrub_flat(r._h, dev.data_ptr(), elems, NS, None, status.data_ptr(), None,
                                    None, bad.data_ptr() if lists[0] else None,
                                    n_bad.data_ptr() if lists[1] else None,
                                    torch.cuda.current_stream().cuda_stream)
            assert rc == 0 and R.core.last_kernel() == "scrub gf8 10+4 " + name
            torch.cuda.synchronize()
            assert (dev.cpu().numpy() == ref).all()
            assert status.cpu().tolist() == [CLEAN, CORRECTED, CLEAN, CLEAN, CORRECTED]
            assert bad.cpu().tolist() == ([1, 4, -1, -1, -1] if lists[0] else [-1] * NS)
            assert n_bad.cpu().tolist() == ([2] if lists[1] else [-1])


def test_the_rule_for_an_fft_codec():
    """By the rule, 16+16 pre-filters 2 KiB shards (the FFT check) and takes
    the direct route at 17 bytes."""
    rng = np.random.default_rng(59)
    for elems, name in ((2048, "prefilter"), (17, "direct")):
        ref = clean_stripes(8, 16, 16, elems)
        buf = ref.copy()
        corrupt_shards(buf, rng, 2, [0, 31], cols=[elems - 1])
        got, status, changed, counts = scrub(8, 16, 16, elems, (1, name), buf)
        assert (got == ref[:NS]).all()
        assert status.tolist() == [CLEAN, CLEAN, CORRECTED, CLEAN, CLEAN]


def test_scrubbing_alone_reaches_the_prefilter_route():
    """A run-time codec that nothing but rse_scrub_flat ever sees (11+3: no
    other test makes one).  Its first scrub, by the rule, requests its kernels
    and does not wait for them; once they are built the rule pre-filters.
    Right results on whichever route."""
    k, p, elems = 11, 3, 4096
    rng = np.random.default_rng(61)
    r = codec(8, k, p)
    assert r.kernel_kind() == "table"
    ref = clean_stripes(8, k, p, elems)
    buf = ref.copy()
    corrupt_shards(buf, rng, 2, [4], cols=[7])
    assert LIB.rse_get_option(SCRUB_ROUTE) == 1
    for again in (False, True):
        got, status, changed, counts = scrub(8, k, p, elems, (1, "prefilter" if again else None),
                                             buf, r=r)
        assert (got == ref[:NS]).all()
        assert status.tolist() == [CLEAN, CLEAN, CORRECTED, CLEAN, CLEAN]
        if not again:
            assert scrub.last_kernel in ("scrub gf8 11+3 direct", "scrub gf8 11+3 prefilter")
            assert r.kernel_kind() != "table", "the scrub alone requested the kernels"
            assert kernels_or_skip(r, "11+3") == "bitslice-specialised"


def test_python_entry_and_out_of_scope_codecs():
    buf = torch.zeros(260 * 16 * 2, dtype=torch.uint8, device="cuda")
    for r in (R.galois_16.ReedSolomon(250, 10), R.galois_8.ReedSolomon(10, 17),
              R.galois_8.ReedSolomon(240, 16)):
        with pytest.raises(R.DeviceError):
            r.scrub_flat(buf, 16, 1)
    with pytest.raises(R.RSError):
        codec(8, 10, 4).scrub_flat(buf, 0, 1)
    out = codec(16, 10, 4).scrub_flat(buf, 16, 0)
    assert [tuple(t.shape) for t in out] == [(0,), (0, 14), (0, 2), (0,), (1,)]
    assert out[4].cpu().tolist() == [0]
    with pytest.raises(R.RSError):  # flags of the wrong shape
        codec(8, 10, 4).scrub_flat(buf, 16, 2, np.ones((2, 13), np.uint8))
    # GF(2^16) through the Python entry, a host array of flags uploaded
    ref = clean_stripes(16, 10, 4, 9)
    host = ref.copy()
    present = np.ones((NS, 14), np.uint8)
    erase(host, present, 2, [0, 13])
    dev = torch.from_numpy(host).cuda()
    status, changed, counts, bad, n_bad = codec(16, 10, 4).scrub_flat(dev, 9, NS, present)
    torch.cuda.synchronize()
    assert (dev.cpu().numpy() == ref).all()
    assert status.cpu().tolist() == [CLEAN, CLEAN, CORRECTED, CLEAN, CLEAN]
    assert n_bad.cpu().tolist() == [1] and bad.cpu().tolist()[0] == 2
    assert np.nonzero(changed.cpu().numpy()[2])[0].tolist() == [0, 13]
