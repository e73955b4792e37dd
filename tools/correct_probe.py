#!/usr/bin/env python3
"""rse_correct_flat against the two-call repair it replaces: same process, same buffer.

Workloads: 10+4 x 1 MiB x 512 stripes and 100+16 x 64 KiB x 512 stripes, in
four states of the buffer:
  clean     every stripe a codeword: correct_flat against locate_flat alone
            (both run the same fast path and write only flags);
  1pct      1 % of the stripes with one whole bad shard;
  all_t     every stripe with t = p // 2 whole bad shards;
  erasure   every stripe with one shard flagged missing (its bytes garbage) and
            one other whole bad shard.  The two-call path has no equivalent:
            locate_flat would spend two checks on the missing shard and cannot
            take flags, so this state is timed for correct_flat alone.
The baseline of the repair states is locate_flat + reconstruct_batch (the
device flags passed unchanged).  Both legs repair the buffer, so the damage is
injected again (XOR on the device, not timed) before every timed call, and
after every call of the first repetition the buffer is compared with its clean
copy.  Times are HIP events around the calls of a leg on the current stream,
after a warm-up of both legs, the legs alternating in order from repetition to
repetition; the median and the range are reported.  Rates count the k + p
shards once.

  python tools/correct_probe.py [--out FILE] [--stripes N]
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
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "correct", "correct_probe.json"))
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
        clean = buf.clone()
        nbytes = stripes * n * length
        bad_t = ([0, n - 1] + list(range(2, t)))[:t]  # t shards, both ends of the point shift
        flags = torch.ones((stripes, n), dtype=torch.uint8, device="cuda")
        flags[:, 1] = 0  # the erasure state's missing shard
        states = [("clean", slice(0, 0), [], None),
                  ("1pct", slice(0, stripes, 100), [3], None),
                  ("all_t", slice(None), bad_t, None),
                  ("erasure", slice(None), [1, n - 2], flags)]

        for state, which, shards, present in states:
            def inject():
                for q in shards:
                    buf[which, q] ^= 0x5A

            def correct():
                return r.correct_flat(flat, length, stripes, present)

            def parent():
                pres, status = r.locate_flat(flat, length, stripes)
                if state != "clean":
                    r.reconstruct_batch(flat, length, stripes, pres)
                return status

            legs = {"correct": correct}
            if present is None:
                legs["parent"] = parent
            n_bad = len(range(*which.indices(stripes))) if shards else 0
            kernels = {}
            first = {}
            for name, fn in legs.items():  # warm-up, checked, and sizes the repetitions
                inject()
                first[name] = timed(fn)
                kernels[name] = last_kernel()
                assert torch.equal(buf, clean), (state, name, "the buffer is not repaired")
            inject()
            status, changed, counts = correct()
            assert int((status == R.CORRECT_CORRECTED).sum()) == n_bad, state
            assert int((status == R.CORRECT_CLEAN).sum()) == stripes - n_bad, state
            assert int(changed.sum()) == n_bad * len(shards), state
            assert int(counts[:, 0].sum()) == n_bad * len(shards) * length, state
            reps = max(3, min(20, int(2.0 / max(first.values()))))
            times = {name: [] for name in legs}
            order = list(legs)
            for rep in range(reps):
                for name in (order if rep % 2 == 0 else order[::-1]):
                    inject()
                    times[name].append(timed(legs[name]))
            assert torch.equal(buf, clean), state
            row = {"codec": f"{k}+{p}", "shard_bytes": length, "stripes": stripes, "state": state,
                   "bad_stripes": n_bad, "bad_shards_per_stripe": len(shards), "reps": reps,
                   "kernels": kernels}
            for name, v in times.items():
                med = sorted(v)[len(v) // 2]
                row[f"{name}_ms"] = med * 1e3
                row[f"{name}_ms_min_max"] = [min(v) * 1e3, max(v) * 1e3]
                row[f"{name}_GBps"] = nbytes / med / 1e9
            if "parent" in times:
                row["correct_over_parent"] = row["correct_ms"] / row["parent_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)
        del buf, flat, clean
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
    print(f"{'codec':>7} {'state':>8} {'correct ms':>11} {'(min-max)':>17} {'parent ms':>10} "
          f"{'(min-max)':>17} {'ratio':>6}")
    for w in rows:
        lo, hi = w["correct_ms_min_max"]
        line = f"{w['codec']:>7} {w['state']:>8} {w['correct_ms']:11.3f} {lo:8.3f}-{hi:<8.3f}"
        if "parent_ms" in w:
            lo, hi = w["parent_ms_min_max"]
            line += (f" {w['parent_ms']:10.3f} {lo:8.3f}-{hi:<8.3f}"
                     f" {w['correct_over_parent']:6.2f}")
        else:
            line += "  (no parent equivalent)"
        print(line)


if __name__ == "__main__":
    main()
