#!/usr/bin/env python3
"""rse_update_flat against what there was before it: same process, same buffer.

Workload: 10+4 x 1 MiB shards x 512 stripes, three write patterns:
  dense    one data shard in every stripe;
  sparse   one data shard in every 16th stripe;
  full     all k data shards of every stripe (the pattern where update must lose:
           it reads old and new and reads the parity, re-encoding reads nothing
           it does not need).
Legs: `update` (rse_update_flat), `reencode` (a device scatter of the new
shards into place -- index_copy_ over the shard rows -- then rse_encode_flat
over the batch: the route a caller had) and, for orientation, `encode`
(rse_encode_flat over the batch alone: what re-encoding costs a caller whose
new shards are in place already, the floor under any scatter).  The legs leave
the same bytes, and a second application changes nothing, so the legs alternate
over one buffer;
after the warm-up call of each leg the written shards are compared with
new_data, every stripe must verify, and update's `result` must say
{applied, touched stripes}.  Times are HIP events around the call on the
current stream, after a warm-up of every leg, the legs alternating in order
from repetition to repetition; median and range of 20 repetitions.

Bytes by count, L = shard bytes: update moves 3 L per entry
(old and new read, new written) and 2 p L per touched stripe (parity read and
written); reencode moves 2 L per entry (the scatter) and (k + p) L per stripe
of the batch.  The achieved rates are those bytes over the median time.

  python tools/update_probe.py [--out FILE] [--stripes N]
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
K, P, LENGTH = 10, 4, 1 * MiB
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
        check(name)
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
    return [("dense", [(s, (3 * s) % K) for s in range(stripes)]),
            ("sparse", [(s, (3 * s) % K) for s in range(0, stripes, 16)]),
            ("full", [(s, i) for s in range(stripes) for i in range(K)])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update", "update_probe.json"))
    ap.add_argument("--stripes", type=int, default=512)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    stripes, n = args.stripes, K + P
    r = R.galois_8.ReedSolomon(K, P)
    kind = r.kernel_kind(wait=True)
    print(f"# {K}+{P}: kernels {kind}", flush=True)
    buf = torch.empty((stripes, n, LENGTH), dtype=torch.uint8, device="cuda")
    flat = buf.view(-1)
    shard_rows = buf.view(stripes * n, LENGTH)
    fill_splitmix(flat, 1, 0)
    r.encode_flat(flat, LENGTH, stripes)
    torch.cuda.synchronize()
    rows = []
    for pattern, entries in patterns(stripes):
        touched = len({s for s, _ in entries})
        upd = torch.tensor(entries, dtype=torch.int32, device="cuda")
        where = (upd[:, 0].long() * n + upd[:, 1].long()).contiguous()
        new = torch.empty((len(entries), LENGTH), dtype=torch.uint8, device="cuda")
        fill_splitmix(new.view(-1), 2, 0)
        results = []

        def update():
            results.append(r.update_flat(flat, LENGTH, stripes, upd, new))
            del results[:-1]

        def reencode():
            shard_rows.index_copy_(0, where, new)
            r.encode_flat(flat, LENGTH, stripes)

        def check(name):
            torch.cuda.synchronize()
            if name == "update":
                assert results[-1].tolist() == [R.UPDATE_APPLIED, touched], (pattern, results[-1])
            for u in sorted({0, len(entries) // 2, len(entries) - 1}):
                assert torch.equal(shard_rows[int(where[u])], new[u]), (pattern, name, u)
            assert r.verify_flat(flat, LENGTH, stripes).all(), (pattern, name, "does not verify")

        row = {"codec": f"{K}+{P}", "field": 8, "shard_bytes": LENGTH, "stripes": stripes,
               "pattern": pattern, "entries": len(entries), "touched_stripes": touched,
               "kernel_kind": kind}
        row.update(measure({"update": update, "reencode": reencode,
                            "encode": lambda: r.encode_flat(flat, LENGTH, stripes)}, check))
        row["update_bytes"] = (3 * len(entries) + 2 * P * touched) * LENGTH
        row["reencode_bytes"] = (2 * len(entries) + n * stripes) * LENGTH
        row["update_TBps"] = row["update_bytes"] / (row["update_ms"] * 1e-3) / 1e12
        row["reencode_TBps"] = row["reencode_bytes"] / (row["reencode_ms"] * 1e-3) / 1e12
        row["encode_bytes"] = n * stripes * LENGTH
        row["encode_TBps"] = row["encode_bytes"] / (row["encode_ms"] * 1e-3) / 1e12
        row["update_over_encode"] = row["update_ms"] / row["encode_ms"]
        row["update_over_reencode"] = row["update_ms"] / row["reencode_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del upd, where, new
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")

    print(f"{'pattern':>8} {'entries':>8} " +
          "".join(f"{leg + ' ms (min-max)':>31}{'TB/s':>7}"
                  for leg in ("update", "reencode", "encode")) +
          "  update/reencode  update/encode  path")
    for w in rows:
        cells = ""
        for leg in ("update", "reencode", "encode"):
            lo, hi = w[f"{leg}_ms_min_max"]
            cells += f"{w[f'{leg}_ms']:11.3f} ({lo:7.3f}-{hi:<7.3f}) {w[f'{leg}_TBps']:6.2f} "
        print(f"{w['pattern']:>8} {w['entries']:>8} {cells}{w['update_over_reencode']:12.2f}"
              f"{w['update_over_encode']:15.2f}       {w['kernels']['update'].split()[-1]}")


if __name__ == "__main__":
    main()
