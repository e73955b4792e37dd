#!/usr/bin/env python3
"""rse_scrub_shards against rse_scrub_flat: same process, same bytes.

Workloads: 10+4 with 512 blocks of 1 MiB per shard and 100+16 with 512 blocks
of 64 KiB per shard, in two states:
  clean     every block a codeword;
  1pct      1 % of the blocks with one bad shard.
Legs:
  shards    rse_scrub_shards on k + p separately allocated shards;
  flat      rse_scrub_flat on the same bytes laid flat, a block per stripe;
  gather    what a caller of the separately allocated shards had to do before
            the entry existed: gather them into a flat staging buffer,
            rse_scrub_flat, copy the shards back;
  skewed    `shards` again with shard r placed r x 4,352 bytes into a larger
            allocation of its own: the allocator puts equally sized shards at
            equal offsets of its 2 MiB granules, and the check kernel reads a
            block of all of them at once.
Both entries are called through the C ABI with the argument arrays and the
output tensors made beforehand, so the host does the same work inside every
timed pair of events.
Every leg repairs its buffer, so before every timed call the damage is injected
again (on the device, not timed), and after the first call of each leg its
buffer is compared with the clean copy.  Times are HIP events around the call
on the current stream, after a warm-up of every leg, the legs alternating in
order from repetition to repetition; median and range of 20 repetitions.  The
run-time kernels of a codec are waited for before anything is timed.

  python tools/scrub_shards_probe.py [--out FILE] [--blocks N]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reed-solomon-erasure_amd"))
import torch  # noqa: E402

import reed_solomon_erasure as R  # noqa: E402
from reed_solomon_erasure._lib import load  # noqa: E402
from reed_solomon_erasure.core import fill_splitmix, last_kernel  # noqa: E402

KiB, MiB = 1 << 10, 1 << 20
WORKLOADS = [(10, 4, 1 * MiB), (100, 16, 64 * KiB)]
REPS = 20
LEGS = ("shards", "flat", "gather", "skewed")
SKEW = 4352
LIB = load()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)  # ms


def measure(legs, inject, check, reps=REPS):
    """Warm-up of every leg (checked), then `reps` alternating rounds."""
    kernels = {}
    for name, fn in legs.items():
        inject(name)
        timed(fn)
        kernels[name] = last_kernel()
        check(name)
    times = {name: [] for name in legs}
    order = list(legs)
    for rep in range(reps):
        for name in (order if rep % 2 == 0 else order[::-1]):
            inject(name)
            times[name].append(timed(legs[name]))
    row = {"reps": reps, "kernels": kernels}
    for name, v in times.items():
        row[f"{name}_ms"] = sorted(v)[len(v) // 2]
        row[f"{name}_ms_min_max"] = [min(v), max(v)]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scrub_shards",
                                                  "scrub_shards_probe.json"))
    ap.add_argument("--blocks", type=int, default=512)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    rows = []
    for k, p, block in WORKLOADS:
        n, blocks = k + p, args.blocks
        r = R.galois_8.ReedSolomon(k, p)
        kind = r.kernel_kind(wait=True)
        print(f"# {k}+{p}: kernels {kind}", flush=True)
        # the clean bytes, made flat: a block per stripe
        clean = torch.empty((blocks, n, block), dtype=torch.uint8, device="cuda")
        fill_splitmix(clean.view(-1), 1, 0)
        r.encode_flat(clean.view(-1), block, blocks)
        flat = clean.clone()
        staging = torch.empty_like(flat)
        shards = [torch.empty(blocks * block, dtype=torch.uint8, device="cuda") for _ in range(n)]
        by_block = [s.view(blocks, block) for s in shards]
        roomy = [torch.empty(blocks * block + n * SKEW, dtype=torch.uint8, device="cuda")
                 for _ in range(n)]
        skewed = [a[q * SKEW:q * SKEW + blocks * block].view(blocks, block)
                  for q, a in enumerate(roomy)]
        for q in range(n):
            by_block[q].copy_(clean[:, q])
            skewed[q].copy_(clean[:, q])
        outs = (torch.empty((blocks,), dtype=torch.uint8, device="cuda"),
                torch.empty((blocks, n), dtype=torch.uint8, device="cuda"),
                torch.empty((blocks, 2), dtype=torch.int32, device="cuda"),
                torch.empty((blocks,), dtype=torch.int32, device="cuda"),
                torch.zeros((1,), dtype=torch.int32, device="cuda"))
        out_ptrs = [t.data_ptr() for t in outs]
        lens = (ctypes.c_size_t * n)(*[blocks * block] * n)
        ptrs = {"shards": (ctypes.c_void_p * n)(*[t.data_ptr() for t in by_block]),
                "skewed": (ctypes.c_void_p * n)(*[t.data_ptr() for t in skewed])}
        st = torch.cuda.current_stream().cuda_stream
        torch.cuda.synchronize()

        def scrub_shards(which_ptrs):
            rc = LIB.rse_scrub_shards(r._h, ptrs[which_ptrs], lens, n, block, None, *out_ptrs, st)
            assert rc == 0

        def scrub_flat(buf):
            rc = LIB.rse_scrub_flat(r._h, buf.data_ptr(), block, blocks, None, *out_ptrs, st)
            assert rc == 0

        for state, step, bad_shard in (("clean", 0, None), ("1pct", 100, 3)):
            which = slice(0, blocks, step) if step else slice(0, 0)
            n_bad = len(range(*which.indices(blocks)))

            def inject(name):
                if bad_shard is None:
                    return
                if name == "flat":
                    flat[which, bad_shard] ^= 0x5A
                elif name == "skewed":
                    skewed[bad_shard][which] ^= 0x5A
                else:
                    by_block[bad_shard][which] ^= 0x5A

            def gather():
                for q in range(n):
                    staging[:, q].copy_(by_block[q])
                scrub_flat(staging)
                for q in range(n):
                    by_block[q].copy_(staging[:, q])

            legs = {"shards": lambda: scrub_shards("shards"), "flat": lambda: scrub_flat(flat),
                    "gather": gather, "skewed": lambda: scrub_shards("skewed")}

            def check(name):
                if name == "flat":
                    assert torch.equal(flat, clean), (state, name, "the buffer is not repaired")
                else:
                    mine = skewed if name == "skewed" else by_block
                    for q in range(n):
                        assert torch.equal(mine[q], clean[:, q]), (state, name, q)

            for name in LEGS:  # the results of every leg, once
                inject(name)
                legs[name]()
                status, changed, counts, bad, nb = outs
                torch.cuda.synchronize()
                assert int(nb[0]) == n_bad, (state, name)
                assert bad[:n_bad].tolist() == list(range(*which.indices(blocks))), (state, name)
                assert int((status == R.CORRECT_CORRECTED).sum()) == n_bad, (state, name)
                assert int(counts[:, 0].sum()) == n_bad * block, (state, name)
            row = {"codec": f"{k}+{p}", "field": 8, "block_bytes": block, "blocks": blocks,
                   "state": state, "bad_blocks": n_bad, "kernel_kind": kind}
            row.update(measure(legs, inject, check))
            lo, hi = row["flat_ms_min_max"]
            row["shards_over_flat"] = row["shards_ms"] / row["flat_ms"]
            row["shards_within_flat_range"] = lo <= row["shards_ms"] <= hi
            row["gather_over_shards"] = row["gather_ms"] / row["shards_ms"]
            row["skewed_over_flat"] = row["skewed_ms"] / row["flat_ms"]
            row["skewed_within_flat_range"] = lo <= row["skewed_ms"] <= hi
            rows.append(row)
            print(json.dumps(row), flush=True)
        del clean, flat, staging, shards, by_block, roomy, skewed
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")

    def cell(w, leg):
        lo, hi = w[f"{leg}_ms_min_max"]
        return f"{w[f'{leg}_ms']:9.3f} ({lo:7.3f}-{hi:<7.3f}) "
    print(f"{'codec':>8} {'state':>6} " + "".join(f"{leg + ' ms (min-max)':>29}" for leg in LEGS) +
          "  shards/flat  in range  skewed/flat  in range  gather/shards  route")
    for w in rows:
        print(f"{w['codec']:>8} {w['state']:>6} " + "".join(cell(w, leg) for leg in LEGS) +
              f"{w['shards_over_flat']:10.3f} {str(w['shards_within_flat_range']):>9} "
              f"{w['skewed_over_flat']:10.3f} {str(w['skewed_within_flat_range']):>9} "
              f"{w['gather_over_shards']:12.2f}     " + w["kernels"]["shards"].split()[-1])


if __name__ == "__main__":
    main()
