#!/usr/bin/env python3
"""rse_scrub_flat against rse_correct_flat: same process, same buffer.

Workloads: 10+4 x 1 MiB x 512 stripes and 100+16 x 64 KiB x 512 stripes, in
four states of the buffer:
  clean     every stripe a codeword;
  1pct      1 % of the stripes with one whole bad shard;
  all_t     every stripe with t = p // 2 whole bad shards;
  erasure   every stripe with one shard flagged missing (its bytes garbage) and
            one other whole bad shard.
Legs: `scrub` (rse_scrub_flat, its route by the rule), `direct`
(RSE_OPT_SCRUB_ROUTE 0), `correct` (rse_correct_flat: the path before the
entry existed) and, for orientation, `verify` (rse_verify_flat, which repairs
nothing and waits for its verdicts on the host).  The repairing legs leave the
buffer clean and verify leaves it damaged, so before every timed call the
buffer is copied from its clean copy and the damage injected again (on the
device, not timed), and after the first call of each repairing leg the buffer
is compared with its clean copy.  Times are HIP events around the call on the
current stream, after a warm-up of every leg, the legs alternating in order
from repetition to repetition; median and range of 20 repetitions.  The
run-time kernels of a codec are waited for before anything is timed.

Then GF(2^16) 20+8 x 4 MiB shards x 64 stripes, clean (rse_correct_flat refuses
the codec: `scrub`, `direct` and `verify` only), and the compaction's own time:
the direct route on clean 10+4 x 16-byte stripes with and without the two
lists, the difference of the medians, at 512 and 1,048,576 stripes.

  python tools/scrub_probe.py [--out FILE] [--stripes N]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reed-solomon-erasure_amd"))
os.environ.setdefault("RSE_TUNE", "1")  # RSE_OPT_SCRUB_ROUTE is a tuning key
import torch  # noqa: E402

import reed_solomon_erasure as R  # noqa: E402
from reed_solomon_erasure._lib import load  # noqa: E402
from reed_solomon_erasure.core import fill_splitmix, last_kernel  # noqa: E402

KiB, MiB = 1 << 10, 1 << 20
WORKLOADS = [(10, 4, 1 * MiB), (100, 16, 64 * KiB)]
SCRUB_ROUTE = 56
REPS = 20
LIB = load()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)  # ms


def on_route(route, fn):
    def run():
        LIB.rse_set_option(SCRUB_ROUTE, route)
        try:
            return fn()
        finally:
            LIB.rse_set_option(SCRUB_ROUTE, 1)
    return run


def measure(legs, inject, check, reps=REPS):
    """Warm-up of every leg (checked), then `reps` alternating rounds."""
    kernels = {}
    for name, fn in legs.items():
        inject()
        timed(fn)
        kernels[name] = last_kernel()
        check(name)
    times = {name: [] for name in legs}
    order = list(legs)
    for rep in range(reps):
        for name in (order if rep % 2 == 0 else order[::-1]):
            inject()
            times[name].append(timed(legs[name]))
    row = {"reps": reps, "kernels": kernels}
    for name, v in times.items():
        row[f"{name}_ms"] = sorted(v)[len(v) // 2]
        row[f"{name}_ms_min_max"] = [min(v), max(v)]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scrub", "scrub_probe.json"))
    ap.add_argument("--stripes", type=int, default=512)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    rows = []
    for k, p, length in WORKLOADS:
        n, t, stripes = k + p, p // 2, args.stripes
        r = R.galois_8.ReedSolomon(k, p)
        kind = r.kernel_kind(wait=True)
        print(f"# {k}+{p}: kernels {kind}", flush=True)
        buf = torch.empty((stripes, n, length), dtype=torch.uint8, device="cuda")
        flat = buf.view(-1)
        fill_splitmix(flat, 1, 0)
        r.encode_flat(flat, length, stripes)
        torch.cuda.synchronize()
        clean = buf.clone()
        bad_t = ([0, n - 1] + list(range(2, t)))[:t]  # t shards, both ends of the point shift
        flags = torch.ones((stripes, n), dtype=torch.uint8, device="cuda")
        flags[:, 1] = 0  # the erasure state's missing shard
        states = [("clean", slice(0, 0), [], None),
                  ("1pct", slice(0, stripes, 100), [3], None),
                  ("all_t", slice(None), bad_t, None),
                  ("erasure", slice(None), [1, n - 2], flags)]
        for state, which, shards, present in states:
            n_bad = len(range(*which.indices(stripes))) if shards else 0

            def inject():
                for q in shards:
                    buf[which, q] ^= 0x5A

            def scrub():
                return r.scrub_flat(flat, length, stripes, present)

            # verify repairs nothing: every call starts from the clean copy + the damage
            def inject_clean():
                buf.copy_(clean)
                inject()

            legs = {"scrub": scrub, "direct": on_route(0, scrub),
                    "correct": lambda: r.correct_flat(flat, length, stripes, present),
                    "verify": lambda: r.verify_flat(flat, length, stripes)}

            def check(name):
                if name != "verify":
                    assert torch.equal(buf, clean), (state, name, "the buffer is not repaired")

            inject_clean()
            status, changed, counts, bad, nb = scrub()
            torch.cuda.synchronize()
            assert int(nb[0]) == n_bad and bad[:n_bad].tolist() == \
                list(range(*which.indices(stripes)))[:n_bad], state
            assert int((status == R.CORRECT_CORRECTED).sum()) == n_bad, state
            assert int(counts[:, 0].sum()) == n_bad * len(shards) * length, state
            row = {"codec": f"{k}+{p}", "field": 8, "shard_bytes": length, "stripes": stripes,
                   "state": state, "bad_stripes": n_bad, "kernel_kind": kind}
            row.update(measure(legs, inject_clean, check))
            row["scrub_over_correct"] = row["scrub_ms"] / row["correct_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)
        del buf, flat, clean
        torch.cuda.empty_cache()

    # GF(2^16) 20+8 x 4 MiB, clean: no rse_correct_flat for it
    k, p, length, stripes = 20, 8, 4 * MiB, 64
    r = R.galois_16.ReedSolomon(k, p)
    kind = r.kernel_kind(wait=True)
    print(f"# gf16 {k}+{p}: kernels {kind}", flush=True)
    flat = torch.empty(stripes * (k + p) * length, dtype=torch.uint8, device="cuda")
    fill_splitmix(flat, 2, 0)
    r.encode_flat(flat, length // 2, stripes)
    torch.cuda.synchronize()

    def scrub16():
        return r.scrub_flat(flat, length // 2, stripes)

    clean = flat.clone()

    def check16(name):
        assert torch.equal(flat, clean), ("gf16", name, "a clean buffer was written")

    row = {"codec": f"{k}+{p}", "field": 16, "shard_bytes": length, "stripes": stripes,
           "state": "clean", "bad_stripes": 0, "kernel_kind": kind}
    row.update(measure({"scrub": scrub16, "direct": on_route(0, scrub16),
                        "verify": lambda: r.verify_flat(flat, length // 2, stripes)},
                       lambda: None, check16))
    rows.append(row)
    print(json.dumps(row), flush=True)
    del flat, clean
    torch.cuda.empty_cache()

    # the compaction alone: direct route, clean 16-byte stripes, lists on and off
    r = R.galois_8.ReedSolomon(10, 4)
    for stripes in (512, 1 << 20):
        flat = torch.empty(stripes * 14 * 16, dtype=torch.uint8, device="cuda")
        fill_splitmix(flat, 3, 0)
        r.encode_flat(flat, 16, stripes)
        status = torch.empty(stripes, dtype=torch.uint8, device="cuda")
        bad = torch.empty(stripes, dtype=torch.int32, device="cuda")
        nb = torch.empty(1, dtype=torch.int32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream

        def call(lists):
            rc = LIB.rse_scrub_flat(r._h, flat.data_ptr(), 16, stripes, None, status.data_ptr(),
                                    None, None, bad.data_ptr() if lists else None,
                                    nb.data_ptr() if lists else None, st)
            assert rc == 0

        def check_lists(name):
            torch.cuda.synchronize()
            assert not status.any() and (name == "without" or int(nb[0]) == 0)

        row = {"codec": "10+4", "field": 8, "shard_bytes": 16, "stripes": stripes,
               "state": "compaction", "bad_stripes": 0}
        row.update(measure({"with": on_route(0, lambda: call(True)),
                            "without": on_route(0, lambda: call(False))},
                           lambda: None, check_lists))
        row["compaction_ms"] = row["with_ms"] - row["without_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del flat

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")

    def cell(w, leg):
        if f"{leg}_ms" not in w:
            return f"{'':>29}"
        lo, hi = w[f"{leg}_ms_min_max"]
        return f"{w[f'{leg}_ms']:9.3f} ({lo:7.3f}-{hi:<7.3f}) "
    print(f"{'codec':>10} {'state':>10} " + "".join(f"{leg + ' ms (min-max)':>29}" for leg in
                                                     ("scrub", "direct", "correct", "verify")) +
          "  scrub/correct  route")
    for w in rows:
        if w["state"] == "compaction":
            print(f"{'10+4':>10} compaction at {w['stripes']} stripes: {w['compaction_ms']:.4f} ms "
                  f"(with lists {w['with_ms']:.4f}, without {w['without_ms']:.4f})")
            continue
        print(f"{'gf%d %s' % (w['field'], w['codec']):>10} {w['state']:>10} " +
              "".join(cell(w, leg) for leg in ("scrub", "direct", "correct", "verify")) +
              (f"{w['scrub_over_correct']:8.2f}" if "scrub_over_correct" in w else f"{'':>8}") +
              "       " + w["kernels"]["scrub"].split()[-1])


if __name__ == "__main__":
    main()
