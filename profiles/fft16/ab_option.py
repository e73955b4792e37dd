"""GF(2^16) 1000+24 x 64 KiB: RSE_OPT_FFT16 (option 54) = 1 (the pruned-FFT
kernel, rse_fft16.hip) against 0, alternating in one process, medians of 5 (the
way tools/tune.py measures): encode_flat, verify_flat and reconstruct_data_flat
with 4 data shards lost.  Value 0 runs on whatever kernels the codec has when
the script starts: the chain of run-time modules if the process finds them in
the module cache, else the table kernels -- the script prints which, and with
`--build` builds the chain first (about two CPU-hours on an empty cache).

usage: ab_option.py [--build] [--stripes S] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("RSE_TUNE", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "reed-solomon-erasure_amd"))
import torch  # noqa: E402
import reed_solomon_erasure as R  # noqa: E402
from reed_solomon_erasure.core import last_kernel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--build", action="store_true")
ap.add_argument("--stripes", type=int, default=32)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                              "ab_option.json"))
args = ap.parse_args()

K, P = 1000, 24
T = K + P
NB = 64 * 1024          # bytes per shard
NE = NB // 2            # elements per shard
S = args.stripes
lib = R._lib.load()
assert lib.rse_get_option(54) == 0
t0 = time.time()
r = R.galois_16.ReedSolomon(K, P)
print(f"codec: {time.time() - t0:.1f} s", flush=True)
if args.build:
    lib.rse_set_option(9, 2)
    t0 = time.time()
    print(f"value 0 kernels: {r.kernel_kind(wait=True)} ({time.time() - t0:.1f} s)", flush=True)
else:
    print(f"value 0 kernels: {r.kernel_kind(wait=False)} (not built here)", flush=True)

a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
lost = [3, 250, 600, 999]
present = [i not in lost for i in range(T)]
out = {"stripes": S, "shard_bytes": NB}


def point(name, fn):
    buf = torch.randint(0, 256, (S * T * NB,), dtype=torch.uint8, device="cuda")
    r.encode_flat(buf, NE, S)
    torch.cuda.synchronize()
    res = {0: [], 1: []}
    kern = {}
    for rnd in range(5):
        for v in (1, 0):
            lib.rse_set_option(54, v)
            fn(buf)  # warm
            torch.cuda.synchronize()
            a.record()
            fn(buf)
            b.record()
            torch.cuda.synchronize()
            kern[v] = last_kernel()
            res[v].append(S * T * NB / (a.elapsed_time(b) * 1e-3) / 1e9)
    lib.rse_set_option(54, 0)
    row = {f"v{v}": {"median": round(statistics.median(x), 1), "min": round(min(x), 1),
                     "max": round(max(x), 1), "kernel": kern[v]} for v, x in res.items()}
    out[name] = row
    print(name, json.dumps(row), flush=True)
    del buf


point("encode", lambda buf: r.encode_flat(buf, NE, S))
point("verify", lambda buf: r.verify_flat(buf, NE, S))
point("rebuild_4_data", lambda buf: r.reconstruct_data_flat(buf, NE, S, present))
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
