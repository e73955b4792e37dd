#!/usr/bin/env python3
"""rse_read_shards against rse_read_flat: same process, same bytes.

Workload: 10+4 with 512 blocks of 1 MiB per shard, tools/read_probe.py's four
read patterns with a block for a stripe, and a fifth:
  a  one erased data shard in every block, and that shard read;
  b  the same in every 16th block;
  c  one present shard per block: pure copy;
  d  four erased data shards per block, all four read;
  e  one data shard with NO BUFFER (a NULL pointer, no flags) read whole: the
     rebuild of a failed device onto a spare.
Legs:
  shards    rse_read_shards on k + p separately allocated shards;
  flat      rse_read_flat on the same bytes laid flat, a block per stripe (for
            e: the shard's flag cleared in every stripe);
  gather    what a caller of the separately allocated shards had to do before
            the entry existed: gather them into a flat staging buffer (for e:
            the thirteen that are there), then rse_read_flat.
Both entries are called through the C ABI with the argument arrays, the list,
the flags, `out`, `status` and `result` made beforehand, so the host does the
same work inside every timed pair of events.  The erased ranges hold garbage
in every layout.  After the warm-up call of each leg its rows are compared with
the bytes that were there before the garbage (a rebuilt row is the original
data), and `status` and `result` must say what the pattern means.  Times are
HIP events around the call on the current stream, after a warm-up of every leg,
the legs alternating in order from repetition to repetition; median and range
of 20 repetitions.

  python tools/read_shards_probe.py [--out FILE] [--blocks N]
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

MiB = 1 << 20
K, P, BLOCK = 10, 4, 1 * MiB
REPS = 20
LEGS = ("shards", "flat", "gather")
NO_BUFFER = 3  # pattern e's shard
LIB = load()


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


def patterns(blocks):
    """(name, erased {block, shard}, read {block, shard}, shard without a buffer)"""
    a = [(b, (3 * b) % K) for b in range(blocks)]
    s16 = [(b, (3 * b) % K) for b in range(0, blocks, 16)]
    c = [(b, (3 * b + 1) % K) for b in range(blocks)]
    d = sorted((b, (3 * b + j) % K) for b in range(blocks) for j in range(4))
    e = [(b, NO_BUFFER) for b in range(blocks)]
    return [("a", a, a, None), ("b", s16, s16, None), ("c", a, c, None), ("d", d, d, None),
            ("e", e, e, NO_BUFFER)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "read_shards",
                                                  "read_shards_probe.json"))
    ap.add_argument("--blocks", type=int, default=512)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    blocks, n = args.blocks, K + P
    r = R.galois_8.ReedSolomon(K, P)
    kind = r.kernel_kind(wait=True)
    print(f"# {K}+{P}: kernels {kind}", flush=True)
    # the bytes, made flat: a block per stripe
    flat = torch.empty((blocks, n, BLOCK), dtype=torch.uint8, device="cuda")
    fill_splitmix(flat.view(-1), 1, 0)
    r.encode_flat(flat.view(-1), BLOCK, blocks)
    flat_rows = flat.view(blocks * n, BLOCK)
    staging = torch.empty_like(flat)
    shards = [torch.empty(blocks * BLOCK, dtype=torch.uint8, device="cuda") for _ in range(n)]
    by_block = [s.view(blocks, BLOCK) for s in shards]
    for q in range(n):
        by_block[q].copy_(flat[:, q])
    lens = (ctypes.c_size_t * n)(*[blocks * BLOCK] * n)
    status = torch.zeros((4 * blocks,), dtype=torch.uint8, device="cuda")
    result = torch.zeros((2,), dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    rows = []
    for pattern, erased, reads, no_buffer in patterns(blocks):
        lost = torch.tensor(erased, dtype=torch.int64, device="cuda")
        lst = torch.tensor(reads, dtype=torch.int32, device="cuda")
        where = (lst[:, 0].long() * n + lst[:, 1].long()).contiguous()
        want = flat_rows.index_select(0, where)        # the entries' bytes before the garbage
        lost_at = lost[:, 0] * n + lost[:, 1]
        kept = flat_rows.index_select(0, lost_at)      # put back after the pattern
        garbage = torch.empty((len(erased), BLOCK), dtype=torch.uint8, device="cuda")
        fill_splitmix(garbage.view(-1), 3, 0)
        flat_rows.index_copy_(0, lost_at, garbage)
        for u, (b, i) in enumerate(erased):
            by_block[i][b].copy_(garbage[u])
        del garbage
        present = torch.ones((blocks, n), dtype=torch.uint8, device="cuda")
        present[lost[:, 0], lost[:, 1]] = 0
        # pattern e: the flat layout needs the flags; the shards entry gets a NULL pointer alone
        flags_shards = None if no_buffer is not None else present.data_ptr()
        ptrs = (ctypes.c_void_p * n)(*[None if q == no_buffer else by_block[q].data_ptr()
                                       for q in range(n)])
        out = torch.empty((len(reads), BLOCK), dtype=torch.uint8, device="cuda")
        tail = (lst.data_ptr(), len(reads), out.data_ptr(), status.data_ptr(), result.data_ptr(), st)

        def read_shards():
            assert LIB.rse_read_shards(r._h, ptrs, lens, n, BLOCK, flags_shards, *tail) == 0

        def read_flat(buf):
            assert LIB.rse_read_flat(r._h, buf.data_ptr(), BLOCK, blocks, present.data_ptr(),
                                     *tail) == 0

        def gather():
            for q in range(n):
                if q != no_buffer:
                    staging[:, q].copy_(by_block[q])
            read_flat(staging)

        legs = {"shards": read_shards, "flat": lambda: read_flat(flat), "gather": gather}
        rebuilt = pattern != "c"

        def check(name):
            torch.cuda.synchronize()
            assert result.tolist() == [R.READ_SERVED, 0], (pattern, name, result)
            cls = R.READ_REBUILT if rebuilt else R.READ_COPIED
            assert bool((status[:len(reads)] == cls).all()), (pattern, name, "status")
            assert torch.equal(out, want), (pattern, name, "rows differ")
            out.zero_()
            status.fill_(0xEE)
            result.fill_(-1)

        row = {"codec": f"{K}+{P}", "field": 8, "block_bytes": BLOCK, "blocks": blocks,
               "pattern": pattern, "entries": len(reads), "kernel_kind": kind,
               "no_buffer": no_buffer}
        row.update(measure(legs, check))
        for name in LEGS:  # and once more after the timed rounds
            legs[name]()
            check(name)
        lo, hi = row["flat_ms_min_max"]
        slo, shi = row["shards_ms_min_max"]
        row["shards_over_flat"] = row["shards_ms"] / row["flat_ms"]
        row["shards_within_flat_range"] = lo <= row["shards_ms"] <= hi
        row["ranges_overlap"] = slo <= hi and lo <= shi
        row["gather_over_shards"] = row["gather_ms"] / row["shards_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        flat_rows.index_copy_(0, lost_at, kept)
        for u, (b, i) in enumerate(erased):
            by_block[i][b].copy_(kept[u])
        del lost, lst, where, want, kept, present, out
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")

    def cell(w, leg):
        lo, hi = w[f"{leg}_ms_min_max"]
        return f"{w[f'{leg}_ms']:9.3f} ({lo:7.3f}-{hi:<7.3f}) "
    print(f"{'pattern':>8} {'entries':>8} " + "".join(f"{leg + ' ms (min-max)':>29}" for leg in LEGS)
          + "  shards/flat  in range  overlap  gather/shards  route")
    for w in rows:
        print(f"{w['pattern']:>8} {w['entries']:>8} " + "".join(cell(w, leg) for leg in LEGS) +
              f"{w['shards_over_flat']:10.3f} {str(w['shards_within_flat_range']):>9} "
              f"{str(w['ranges_overlap']):>8} {w['gather_over_shards']:12.2f}     "
              + w["kernels"]["shards"].split()[-1])


if __name__ == "__main__":
    main()
