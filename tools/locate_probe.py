#!/usr/bin/env python3
"""rse_locate_flat against rse_verify_flat: same process, same buffer.

Workloads: 10+4 x 1 MiB x 512 stripes and 100+16 x 64 KiB x 512 stripes, in
three states of the buffer:
  clean     every stripe a codeword (the locate kernel's fast path only);
  1pct      1 % of the stripes with one whole bad shard;
  all_bad   every stripe with t = p // 2 whole bad shards (the slow path --
            the column decoder -- runs in every wave).
Times are HIP events around each call on the current stream (verify_flat ends
in a stream synchronise, locate_flat does not; the events bracket the device
work of both), after a warm-up of both, the two calls alternating in order
from repetition to repetition.  Rates count the k + p shards read once.
Every state's status words are checked against what was injected.

  python tools/locate_probe.py [--out FILE] [--stripes N]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reed-solomon-erasure_amd"))
import torch  # noqa: E402

import reed_solomon_erasure as R  # noqa: E402
from reed_solomon_erasure.core import fill_splitmix, last_kernel  # noqa: E402

KiB, MiB = 1 << 10, 1 << 20
WORKLOADS = [(10, 4, 1 * MiB), (100, 16, 64 * KiB)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def measure(r, flat, length, stripes, budget_s=2.0):
    calls = {"locate": lambda: r.locate_flat(flat, length, stripes),
             "verify": lambda: r.verify_flat(flat, length, stripes)}
    first = {name: timed(fn) for name, fn in calls.items()}  # warm-up, and sizes the repetitions
    reps = max(2, min(20, int(budget_s / max(first.values()))))
    times = {name: [] for name in calls}
    for rep in range(reps):
        for name in (("locate", "verify") if rep % 2 == 0 else ("verify", "locate")):
            times[name].append(timed(calls[name]))
    return {name: sorted(v)[len(v) // 2] for name, v in times.items()}, \
           {name: (min(v), max(v)) for name, v in times.items()}, reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "locate", "locate_probe.json"))
    ap.add_argument("--stripes", type=int, default=512)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    rows = []
    for k, p, length in WORKLOADS:
        n, t, stripes = k + p, p // 2, args.stripes
        r = R.galois_8.ReedSolomon(k, p)
        buf = torch.empty((stripes, n, length), dtype=torch.uint8, device="cuda")
        flat = buf.view(-1)
        fill_splitmix(flat, 1, 0)
        r.encode_flat(flat, length, stripes)
        torch.cuda.synchronize()
        nbytes = stripes * n * length
        bad = [0, n - 1] + list(range(2, t))  # t shards, both ends of the point shift
        states = [("clean", None, 0),
                  ("1pct", (slice(0, stripes, 100), [3]), len(range(0, stripes, 100))),
                  ("all_bad", (slice(None), bad[:t]), stripes)]
        for state, where, n_bad in states:
            if where:
                for q in where[1]:
                    buf[where[0], q] ^= 0x5A
            med, spread, reps = measure(r, flat, length, stripes)
            present, status = r.locate_flat(flat, length, stripes)
            kernel = last_kernel()
            status = status.cpu()
            ok = r.verify_flat(flat, length, stripes)
            verify_kernel = last_kernel()
            assert int((status == R.LOCATE_LOCATED).sum()) == n_bad, state
            assert int((status == R.LOCATE_CLEAN).sum()) == stripes - n_bad, state
            assert int((~ok).sum()) == n_bad, state
            assert int((present == 0).sum()) == (len(where[1]) * n_bad if where else 0), state
            if where:  # XOR again: the clean buffer
                for q in where[1]:
                    buf[where[0], q] ^= 0x5A
            row = {"codec": f"{k}+{p}", "shard_bytes": length, "stripes": stripes, "state": state,
                   "reps": reps, "kernel": kernel, "verify_kernel": verify_kernel,
                   "locate_ms": med["locate"] * 1e3, "verify_ms": med["verify"] * 1e3,
                   "locate_ms_min_max": [x * 1e3 for x in spread["locate"]],
                   "verify_ms_min_max": [x * 1e3 for x in spread["verify"]],
                   "locate_GBps": nbytes / med["locate"] / 1e9,
                   "verify_GBps": nbytes / med["verify"] / 1e9,
                   "locate_over_verify": med["locate"] / med["verify"]}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del buf, flat
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
    print(f"{'codec':>7} {'state':>8} {'locate ms':>10} {'verify ms':>10} {'locate GB/s':>12} "
          f"{'verify GB/s':>12} {'ratio':>6}")
    for w in rows:
        print(f"{w['codec']:>7} {w['state']:>8} {w['locate_ms']:10.3f} {w['verify_ms']:10.3f} "
              f"{w['locate_GBps']:12.1f} {w['verify_GBps']:12.1f} {w['locate_over_verify']:6.2f}")


if __name__ == "__main__":
    main()
