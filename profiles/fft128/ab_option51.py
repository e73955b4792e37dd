"""GF(2^8) 128+128: option 51 = 2 (FFT kernel) against 1 (wide modules, built
first, RSE_OPT_JIT 2), alternating in one process, medians of 5 (the way
tools/tune.py measures)."""
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

K = 128
T = 256
lib = R._lib.load()
lib.rse_set_option(9, 2)
assert lib.rse_get_option(51) == 1
r = R.galois_8.ReedSolomon(K, K)
t0 = time.time()
kind = r.kernel_kind(wait=True)
print(f"value 1 kernels: {kind} ({time.time() - t0:.1f} s)", flush=True)

a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
present = [i >= K for i in range(T)]
out = {}


def point(name, L, S, fn, nbytes):
    buf = torch.randint(0, 256, (S * T * L,), dtype=torch.uint8, device="cuda")
    r.encode_flat(buf, L, S)
    torch.cuda.synchronize()
    res = {1: [], 2: []}
    kern = {}
    for rnd in range(5):
        for v in (2, 1):
            lib.rse_set_option(51, v)
            fn(buf, L, S)  # warm
            a.record()
            fn(buf, L, S)
            b.record()
            torch.cuda.synchronize()
            kern[v] = last_kernel()
            res[v].append(nbytes(L, S) / (a.elapsed_time(b) * 1e-3) / 1e9)
    lib.rse_set_option(51, 1)
    row = {f"v{v}": {"median": round(statistics.median(x), 1), "min": round(min(x), 1),
                     "max": round(max(x), 1), "kernel": kern[v]} for v, x in res.items()}
    out[name] = row
    print(name, json.dumps(row), flush=True)
    del buf


enc = lambda buf, L, S: r.encode_flat(buf, L, S)
ver = lambda buf, L, S: r.verify_flat(buf, L, S)
reb = lambda buf, L, S: r.reconstruct_data_flat(buf, L, S, present)
full = lambda L, S: S * T * L
point("encode_1KiB_x1024", 1024, 1024, enc, full)
point("encode_1KiB_x2048", 1024, 2048, enc, full)
point("encode_1MiB_x4", 1 << 20, 4, enc, full)
point("verify_1KiB_x2048", 1024, 2048, ver, full)
point("rebuild_all_data_1KiB_x2048", 1024, 2048, reb, full)
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "ab_option51.json"), "w") as f:
    json.dump(out, f, indent=1)
