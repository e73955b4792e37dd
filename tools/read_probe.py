#!/usr/bin/env python3
"""rse_read_flat against what there was before it: same process, same buffer.

Workload: 10+4 x 1 MiB shards x 512 stripes (and, beside it, x 1 KiB shards x
65536 stripes, where a span is a whole run and every work item loads new
tables), four read patterns:
  a  one erased data shard in every stripe, and that shard read: the traffic
     of a failed device;
  b  the same in every 16th stripe;
  c  one present shard per stripe: pure copy;
  d  four erased data shards per stripe, all four read.
Legs: `read` (rse_read_flat into a separate buffer) and, for a, b and d,
`recon` (rse_reconstruct_batch(data_only = 1) over the batch with the same
flags: the route a caller had, which rebuilds in place -- the same bytes moved
in a and d, the whole batch planned in b).  After the warm-up call of each leg
the bytes are checked: the stripes repaired by `recon` must verify, and every
row `read` wrote must equal the shard `recon` left in place; `status` and
`result` must say what the pattern means.  The erased buffers hold garbage
before the first call.  Times are HIP events around the call on the current
stream, after the warm-up of every leg, the legs alternating in order from
repetition to repetition; median and range of 20 repetitions.

Bytes by count, L = shard bytes: per stripe that rebuilds, k L
read and L written per rebuilt entry; per copied entry L read and L written.
The achieved rates are those bytes over the median time.

  python tools/read_probe.py [--out FILE]
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

MiB = 1 << 20
K, P = 10, 4
REPS = 20


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)  # ms


def measure(legs, check, reps=REPS):
    """Warm-up of every leg (checked), then `reps` alternating rounds."""
    kernels = {}
    for name, fn in legs.items():
        timed(fn)
        kernels[name] = last_kernel()
    check()
    times = {name: [] for name in legs}
    order = list(legs)
    for rep in range(reps):
        for name in (order if rep % 2 == 0 else order[::-1]):
            times[name].append(timed(legs[name]))
    row = {"reps": reps, "kernels": kernels}
    for name, v in times.items():
        row[f"{name}_ms"] = sorted(v)[len(v) // 2]
        row[f"{name}_ms_min_max"] = [min(v), max(v)]
    return row


def patterns(stripes):
    """(name, erased {stripe, shard}, read {stripe, shard})"""
    a = [(s, (3 * s) % K) for s in range(stripes)]
    b = [(s, (3 * s) % K) for s in range(0, stripes, 16)]
    c = [(s, (3 * s + 1) % K) for s in range(stripes)]
    d = sorted((s, (3 * s + j) % K) for s in range(stripes) for j in range(4))
    return [("a", a, a), ("b", b, b), ("c", a, c), ("d", d, d)]


def run_config(r, length, stripes, kind):
    n = K + P
    buf = torch.empty((stripes, n, length), dtype=torch.uint8, device="cuda")
    flat = buf.view(-1)
    shard_rows = buf.view(stripes * n, length)
    fill_splitmix(flat, 1, 0)
    r.encode_flat(flat, length, stripes)
    torch.cuda.synchronize()
    rows = []
    for pattern, erased, reads in patterns(stripes):
        lost = torch.tensor(erased, dtype=torch.int64, device="cuda")
        present = torch.ones((stripes, n), dtype=torch.uint8, device="cuda")
        present[lost[:, 0], lost[:, 1]] = 0
        lst = torch.tensor(reads, dtype=torch.int32, device="cuda")
        where = (lst[:, 0].long() * n + lst[:, 1].long()).contiguous()
        out = torch.empty((len(reads), length), dtype=torch.uint8, device="cuda")
        garbage = torch.empty((len(erased), length), dtype=torch.uint8, device="cuda")
        fill_splitmix(garbage.view(-1), 3, 0)
        shard_rows.index_copy_(0, lost[:, 0] * n + lost[:, 1], garbage)  # the erased buffers
        del garbage
        rebuilt = pattern != "c"
        assert not r.verify_flat(flat, length, stripes).all()
        results = []

        def read():
            results.append(r.read_flat(flat, length, stripes, present, lst, out=out.view(-1)))
            del results[:-1]

        def recon():
            r.reconstruct_batch(flat, length, stripes, present, data_only=True)

        def check():
            torch.cuda.synchronize()
            _, status, result = results[-1]
            assert result.tolist() == [R.READ_SERVED, 0], (pattern, result)
            want = R.READ_REBUILT if rebuilt else R.READ_COPIED
            assert bool((status == want).all()), (pattern, "status")
            if not rebuilt:  # the comparator is not a leg: it repairs the stripes for the check
                recon()
                torch.cuda.synchronize()
            assert r.verify_flat(flat, length, stripes).all(), (pattern, "does not verify")
            assert torch.equal(out, shard_rows.index_select(0, where)), (pattern, "rows differ")

        legs = {"read": read}
        if rebuilt:
            legs["recon"] = recon
        row = {"codec": f"{K}+{P}", "field": 8, "shard_bytes": length, "stripes": stripes,
               "pattern": pattern, "entries": len(reads), "kernel_kind": kind}
        row.update(measure(legs, check))
        touched = len({s for s, _ in reads})
        row["bytes"] = ((K * touched + len(reads)) if rebuilt else 2 * len(reads)) * length
        row["read_TBps"] = row["bytes"] / (row["read_ms"] * 1e-3) / 1e12
        if rebuilt:
            row["recon_TBps"] = row["bytes"] / (row["recon_ms"] * 1e-3) / 1e12
            row["read_over_recon"] = row["read_ms"] / row["recon_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del lost, present, lst, where, out
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "read", "read_probe.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    r = R.galois_8.ReedSolomon(K, P)
    kind = r.kernel_kind(wait=True)
    print(f"# {K}+{P}: kernels {kind}", flush=True)
    rows = run_config(r, 1 * MiB, 512, kind) + run_config(r, 1024, 65536, kind)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")

    print(f"{'shard':>8} {'pattern':>8} {'entries':>8} " +
          "".join(f"{leg + ' ms (min-max)':>31}{'TB/s':>7}" for leg in ("read", "recon")) +
          "  read/recon  route")
    for w in rows:
        cells = ""
        for leg in ("read", "recon"):
            if f"{leg}_ms" not in w:
                cells += " " * 38
                continue
            lo, hi = w[f"{leg}_ms_min_max"]
            cells += f"{w[f'{leg}_ms']:11.3f} ({lo:7.3f}-{hi:<7.3f}) {w[f'{leg}_TBps']:6.2f} "
        ratio = f"{w['read_over_recon']:10.2f}" if "read_over_recon" in w else " " * 10
        print(f"{w['shard_bytes']:>8} {w['pattern']:>8} {w['entries']:>8} {cells}{ratio}"
              f"  {w['kernels']['read'].split()[-1]}")


if __name__ == "__main__":
    main()
