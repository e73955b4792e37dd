#!/usr/bin/env python3
"""rse_update_shards against rse_update_flat: same process, same bytes.

Workload: 10+4 with 512 blocks of 1 MiB per shard, tools/update_probe.py's three
write patterns with a block for a stripe:
  dense    one data shard in every block;
  sparse   one data shard in every 16th block;
  full     all k data shards of every block.
Legs:
  shards    rse_update_shards on k + p separately allocated shards (the
            allocator places them on 2 MiB boundaries);
  skewed    `shards` again with shard r placed r x 4,352 bytes into a larger
            allocation of its own, as tools/scrub_shards_probe.py does: equally
            sized allocations sit at equal offsets of the allocator's granules,
            and a work item reads a block of several of them at once;
  flat      rse_update_flat on the same bytes laid flat, a block per stripe;
  gather    what a caller of the separately allocated shards had to do before
            the entry existed: gather them into a flat staging buffer,
            rse_update_flat, copy the shards back.
Both entries are called through the C ABI with the argument arrays, the list,
new_data and `result` made beforehand, so the host does the same work inside
every timed pair of events.  A second application of a list changes nothing
(old = new), and moves the same bytes, so the legs alternate over their buffers
without anything being restored.  After the warm-up call of each leg the written
ranges are compared with new_data, the leg's bytes with the `flat` leg's, and
`result` must say {applied, touched blocks}; every block of the flat buffer must
verify.  Times are HIP events around the call on the current stream, after a
warm-up of every leg, the legs alternating in order from repetition to
repetition; median and range of 20 repetitions.

  python tools/update_shards_probe.py [--out FILE] [--blocks N]

Where a leg falls outside `flat`'s range, the kernel that differs is named by a
kernel trace, in a run of its own: `--trace N` makes N calls of shards, skewed
and flat in turn per pattern and times nothing, and `--summarise CSV` splits the
trace's dispatches by pattern and leg again:

  rocprofv3 --kernel-trace --output-format csv -d DIR -o trace -- \\
      python tools/update_shards_probe.py --trace 10
  python tools/update_shards_probe.py --summarise DIR/trace_kernel_trace.csv
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
LEGS = ("shards", "skewed", "flat", "gather")
TRACE_LEGS = ("shards", "skewed", "flat")
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


def summarise(path):
    """Per pattern, kernel and leg of a kernel trace of `--trace N`: calls,
    median and minimum duration in us.  The dispatches of one kernel come in
    the order of the calls: per pattern one call of every leg of LEGS (`gather`
    runs the flat kernel), then N rounds of TRACE_LEGS."""
    import csv
    by_kernel = {}
    for r in sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"])):
        name = r["Kernel_Name"]
        if "update_" in name:
            by_kernel.setdefault(name, []).append(
                (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    plan = next(v for kname, v in by_kernel.items() if "update_plan_kernel" in kname)
    per_pattern = len(plan) // 3            # calls of a pattern: 4 + N x 3
    rounds = (per_pattern - len(LEGS)) // len(TRACE_LEGS)
    assert per_pattern * 3 == len(plan) and 4 + rounds * 3 == per_pattern, len(plan)

    def cells(durs):
        med = ["%.1f" % sorted(d)[len(d) // 2] for d in durs]
        return f"median us: {med}  min: {['%.1f' % min(d) for d in durs]}"
    print(f"# rocprofv3 --kernel-trace of {rounds} calls each after one warm-up: rse_update_shards "
          f"on separate allocations, on allocations skewed by r x {SKEW} bytes, rse_update_flat "
          f"({K}+{P}, 512 blocks of 1 MiB); per pattern and kernel: median and minimum duration "
          "in us per leg")
    for i, (pattern, _) in enumerate(patterns(0)):
        calls = plan[i * per_pattern + len(LEGS):(i + 1) * per_pattern]
        print(f"{pattern:>7} update_plan_kernel            shards/skew/flat "
              + cells([calls[j::3] for j in range(3)]))
        for kname, v in by_kernel.items():
            if "update_plan_kernel" in kname:
                continue
            layout_shards = "UpdShards" in kname
            n_warm, n_timed = (2, 2 * rounds) if layout_shards else (2, rounds)
            mine = v[i * (n_warm + n_timed) + n_warm:(i + 1) * (n_warm + n_timed)]
            short = ("update_kernel<" + kname.split("update_kernel<")[-1].split(">")[0] + ">"
                     ).replace("rse::(anonymous namespace)::", "")
            if layout_shards:
                print(f"{pattern:>7} {short:<60} shards/skew " + cells([mine[0::2], mine[1::2]]))
            else:
                print(f"{pattern:>7} {short:<60} flat        " + cells([mine]))


def patterns(blocks):
    return [("dense", [(b, (3 * b) % K) for b in range(blocks)]),
            ("sparse", [(b, (3 * b) % K) for b in range(0, blocks, 16)]),
            ("full", [(b, i) for b in range(blocks) for i in range(K)])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_shards",
                                                  "update_shards_probe.json"))
    ap.add_argument("--blocks", type=int, default=512)
    ap.add_argument("--trace", type=int, default=0, metavar="N")
    ap.add_argument("--summarise", metavar="CSV")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)
    assert torch.cuda.is_available(), "needs a HIP device"
    blocks, n = args.blocks, K + P
    r = R.galois_8.ReedSolomon(K, P)
    kind = r.kernel_kind(wait=True)
    print(f"# {K}+{P}: kernels {kind}", flush=True)
    # the bytes, made flat: a block per stripe
    flat = torch.empty((blocks, n, BLOCK), dtype=torch.uint8, device="cuda")
    fill_splitmix(flat.view(-1), 1, 0)
    r.encode_flat(flat.view(-1), BLOCK, blocks)
    staging = torch.empty_like(flat)
    shards = [torch.empty(blocks * BLOCK, dtype=torch.uint8, device="cuda") for _ in range(n)]
    by_block = [s.view(blocks, BLOCK) for s in shards]
    roomy = [torch.empty(blocks * BLOCK + n * SKEW, dtype=torch.uint8, device="cuda")
             for _ in range(n)]
    skewed = [a[q * SKEW:q * SKEW + blocks * BLOCK].view(blocks, BLOCK)
              for q, a in enumerate(roomy)]
    for q in range(n):
        by_block[q].copy_(flat[:, q])
        skewed[q].copy_(flat[:, q])
    lens = (ctypes.c_size_t * n)(*[blocks * BLOCK] * n)
    ptrs = {"shards": (ctypes.c_void_p * n)(*[t.data_ptr() for t in by_block]),
            "skewed": (ctypes.c_void_p * n)(*[t.data_ptr() for t in skewed])}
    placement = {name: [int(v) % (2 * MiB) for v in ptrs[name]] for name in ptrs}
    result = torch.zeros((2,), dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    rows = []
    for pattern, entries in patterns(blocks):
        touched = len({b for b, _ in entries})
        upd = torch.tensor(entries, dtype=torch.int32, device="cuda")
        new = torch.empty((len(entries), BLOCK), dtype=torch.uint8, device="cuda")
        fill_splitmix(new.view(-1), 2, 0)
        args_tail = (upd.data_ptr(), new.data_ptr(), len(entries), result.data_ptr(), st)

        def update_shards(which):
            rc = LIB.rse_update_shards(r._h, ptrs[which], lens, n, BLOCK, *args_tail)
            assert rc == 0

        def update_flat(buf):
            rc = LIB.rse_update_flat(r._h, buf.data_ptr(), BLOCK, blocks, *args_tail)
            assert rc == 0

        def gather():
            for q in range(n):
                staging[:, q].copy_(by_block[q])
            update_flat(staging)
            for q in range(n):
                by_block[q].copy_(staging[:, q])

        legs = {"shards": lambda: update_shards("shards"),
                "skewed": lambda: update_shards("skewed"),
                "flat": lambda: update_flat(flat), "gather": gather}

        def check(name):
            torch.cuda.synchronize()
            assert result.tolist() == [R.UPDATE_APPLIED, touched], (pattern, name, result)
            result.fill_(-1)
            if name == "flat":
                assert r.verify_flat(flat.view(-1), BLOCK, blocks).all(), (pattern, "does not verify")
                return
            mine = skewed if name == "skewed" else by_block
            for u in sorted({0, len(entries) // 2, len(entries) - 1}):
                assert torch.equal(mine[entries[u][1]][entries[u][0]], new[u]), (pattern, name, u)

        def compare():  # every leg's bytes with the flat leg's, after all warm-ups
            for name, mine in (("shards", by_block), ("skewed", skewed)):
                for q in range(n):
                    assert torch.equal(mine[q], flat[:, q]), (pattern, name, q)

        row = {"codec": f"{K}+{P}", "field": 8, "block_bytes": BLOCK, "blocks": blocks,
               "pattern": pattern, "entries": len(entries), "touched_blocks": touched,
               "kernel_kind": kind, "pointer_mod_2MiB": placement}
        for name in LEGS:  # once each before the timed rounds, then the bytes compared
            legs[name]()
        compare()
        if args.trace:  # the calls alone, for a kernel trace: TRACE_LEGS in turn, nothing timed
            for _ in range(args.trace):
                for name in TRACE_LEGS:
                    legs[name]()
            torch.cuda.synchronize()
            continue
        row.update(measure(legs, check))
        compare()
        lo, hi = row["flat_ms_min_max"]
        row["shards_over_flat"] = row["shards_ms"] / row["flat_ms"]
        row["shards_within_flat_range"] = lo <= row["shards_ms"] <= hi
        row["skewed_over_flat"] = row["skewed_ms"] / row["flat_ms"]
        row["skewed_within_flat_range"] = lo <= row["skewed_ms"] <= hi
        row["gather_over_shards"] = row["gather_ms"] / row["shards_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del upd, new
        torch.cuda.empty_cache()

    if args.trace:
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")

    def cell(w, leg):
        lo, hi = w[f"{leg}_ms_min_max"]
        return f"{w[f'{leg}_ms']:9.3f} ({lo:7.3f}-{hi:<7.3f}) "
    print(f"{'pattern':>8} {'entries':>8} " + "".join(f"{leg + ' ms (min-max)':>29}" for leg in LEGS)
          + "  shards/flat  in range  skewed/flat  in range  gather/shards  route")
    for w in rows:
        print(f"{w['pattern']:>8} {w['entries']:>8} " + "".join(cell(w, leg) for leg in LEGS) +
              f"{w['shards_over_flat']:10.3f} {str(w['shards_within_flat_range']):>9} "
              f"{w['skewed_over_flat']:10.3f} {str(w['skewed_within_flat_range']):>9} "
              f"{w['gather_over_shards']:12.2f}     " + w["kernels"]["shards"].split()[-1])


if __name__ == "__main__":
    main()
