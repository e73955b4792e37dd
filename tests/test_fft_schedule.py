"""The schedule of the additive-FFT kernels (rse_fft_sched.hpp: element <->
(wave, register) maps, levels per phase, twiddle templates -- what rse_fft.hip
instantiates), walked on scalar bytes by tests/native/fft_schedule.cpp for
k = p = 16, 32, 64 and 128, on the CPU:

- the parity bytes of fixed data columns equal the oracle's matrix encode
  (core.rs:430-436, 481-509);
- every butterfly's twiddle is s^_i(beta ^ j) (level i, block offset j; beta 0
  for the inverse transform, k for the forward one), and every level runs each
  of its k/2 butterflies exactly once, the inverse levels before the forward
  ones.

The GPU tests (test_gpu_fft.py, test_gpu_fft128.py) check the kernels built on
the same templates with the bit-plane networks in place of the byte multiply."""
import collections
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import oracle as O  # noqa: E402

CSRC = os.path.join(HERE, "..", "reed-solomon-erasure_amd", "csrc")
SRC = os.path.join(HERE, "native", "fft_schedule.cpp")
KS = [16, 32, 64, 128]


def gmul(a, b):  # GF(2^8) modulo 0x11D (build.rs:11)
    r = 0
    while b:
        if b & 1:
            r ^= a
        b >>= 1
        a <<= 1
        if a & 0x100:
            a ^= 0x11D
    return r


@functools.lru_cache(maxsize=None)
def ginv(a):
    return next(x for x in range(1, 256) if gmul(a, x) == 1)


@functools.lru_cache(maxsize=None)
def vanish(i, x):  # s_i(x) = prod over a in span(1, 2, .. 2^(i-1)) of (x + a)
    r = 1
    for a in range(1 << i):
        r = gmul(r, x ^ a)
    return r


@functools.lru_cache(maxsize=None)
def skew(i, x):  # s^_i(x) = s_i(x) / s_i(2^i)
    return gmul(vanish(i, x), ginv(vanish(i, 1 << i)))


def parse(text):
    """{K: {"head": {...}, "bfly": [(inv, level, j, c)], "cols": [(in, out)]}}"""
    runs, cur = {}, None
    for line in text.splitlines():
        f = line.split()
        if f[0] == "K":
            cur = {"head": {f[i]: int(f[i + 1]) for i in range(0, len(f), 2)}, "bfly": [],
                   "cols": []}
            runs[int(f[1])] = cur
        elif f[0] == "bfly":
            cur["bfly"].append((f[1] == "inv", int(f[2]), int(f[3]), int(f[4])))
        elif f[0] == "in":
            cur["cols"].append([[int(v) for v in f[1:]]])
        elif f[0] == "out":
            cur["cols"][-1].append([int(v) for v in f[1:]])
    return runs


def build_and_run(tmp_path, name, flags):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-I", CSRC, *flags, SRC, "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    return parse(build_and_run(tmp_path_factory.mktemp("fft_schedule"), "fft_schedule", ["-O1"]))


@pytest.mark.parametrize("k", KS)
def test_schedule_parity_equals_the_oracle(walk, k):
    run = walk[k]
    assert len(run["cols"]) == 4
    oc = O.Codec(8, k, k)
    cols = np.asarray([c[0] for c in run["cols"]], np.uint8)  # [column][shard]
    assert cols.shape == (4, k) and cols[1:].any()
    sh = [cols[:, i].copy() for i in range(k)] + [np.zeros(4, np.uint8) for _ in range(k)]
    oc.encode(sh)
    for b, (_, out) in enumerate(run["cols"]):
        assert out == [int(sh[k + j][b]) for j in range(k)], (k, b)


@pytest.mark.parametrize("k", KS)
def test_schedule_twiddles_and_levels(walk, k):
    run = walk[k]
    h = run["head"]
    m = k.bit_length() - 1
    assert h["M"] == m and h["E"] * h["W"] == k and h["G"] * h["GPW"] == h["E"]
    assert h["E"] == (16 if k == 128 else 8) and (1 << h["LA"]) == h["E"]
    bf = run["bfly"]
    assert len(bf) == 2 * m * (k // 2)  # 128: 2 x 448
    for inv, i, j, c in bf:
        assert 0 <= i < m and j % (2 << i) == 0 and 0 <= j < k
        assert c == skew(i, (0 if inv else k) ^ j), (inv, i, j, c)
    # each level: every block offset j, 2^i butterflies each
    count = collections.Counter((inv, i, j) for inv, i, j, _ in bf)
    for inv in (True, False):
        for i in range(m):
            for j in range(0, k, 2 << i):
                assert count[(inv, i, j)] == 1 << i, (inv, i, j)
    # a level's butterflies depend on the level before: the walk is phase by
    # phase over all waves, so the phases must come in order -- A (inverse
    # levels < LA), B (levels >= LA, per wave), C (forward levels < LA)
    def phase(inv, i):
        return 1 if i >= h["LA"] else 0 if inv else 2
    ph = [phase(inv, i) for inv, i, _, _ in bf]
    assert ph == sorted(ph)


def test_schedule_walk_is_clean_under_sanitizers(tmp_path, walk):
    """The same stand-alone program under ASan + UBSan (host code only): every
    register and slot index of the maps stays inside its array."""
    out = build_and_run(tmp_path, "fft_schedule_san",
                        ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert parse(out) == walk
