"""One warm and one counted encode_flat of GF(2^16) 1000+24 x 64 KiB on the
pruned-FFT kernel (RSE_OPT_FFT16 1), for a counter pass of its own:

  rocprofv3 --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY \
      SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_LDS SQ_BUSY_CYCLES \
      --output-format csv -d OUT -- python profiles/fft16/pmc_encode.py [stripes]

(no tracing in the same run)."""
import os
import sys

os.environ.setdefault("RSE_TUNE", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "reed-solomon-erasure_amd"))
import torch  # noqa: E402
import reed_solomon_erasure as R  # noqa: E402
from reed_solomon_erasure.core import last_kernel  # noqa: E402

K, P, NB = 1000, 24, 64 * 1024
S = int(sys.argv[1]) if len(sys.argv) > 1 else 32
lib = R._lib.load()
assert lib.rse_set_option(54, 1) == 0
r = R.galois_16.ReedSolomon(K, P)
buf = torch.randint(0, 256, (S * (K + P) * NB,), dtype=torch.uint8, device="cuda")
for _ in range(2):
    r.encode_flat(buf, NB // 2, S)
    torch.cuda.synchronize()
print(last_kernel(), flush=True)
