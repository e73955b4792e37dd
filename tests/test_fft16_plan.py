"""The host tables of the GF(2^16) pruned-FFT kernel (rse_fft16_plan.hpp: block
twiddles, H[q], the encode matrix, a pattern's matrix), walked for 500+12 by
tests/native/fft16_plan.cpp on the CPU and compared with the oracle:

- the parity rows the plan derives from its tables are the codec's matrix rows
  (core.rs:430-436), so whatever the tables code is the reference's encode;
- the parity of a fixed data column, computed as the kernel does (pruned block
  transforms, then the encode matrix), equals the oracle's encode;
- for a mixed data + parity erasure pattern, the values rebuilt with the
  pattern's matrix, and with its plain rows over the valid inputs, equal the
  oracle's reconstruct (core.rs:733-923);
- the 16 x 16 bit matrix of a constant multiplies as the field does.

The same program also runs under ASan + UBSan (host code only)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import oracle as O  # noqa: E402

CSRC = os.path.join(HERE, "..", "reed-solomon-erasure_amd", "csrc")
SRC = os.path.join(HERE, "native", "fft16_plan.cpp")
K, P = 500, 12


def parse(text):
    out = {}
    for line in text.splitlines():
        f = line.split()
        if f[0] == "plan":
            out["plan"] = {f[i]: int(f[i + 1]) for i in range(1, len(f), 2)}
        else:
            out.setdefault(f[0], []).append([int(v) for v in f[1:]])
    return out


def build_and_run(tmp_path, name, flags):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-I", CSRC, *flags, SRC, "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    return parse(build_and_run(tmp_path_factory.mktemp("fft16_plan"), "fft16_plan", ["-O1"]))


@pytest.fixture(scope="module")
def codec():
    return O.Codec(16, K, P)


def shard(v):  # one element -> the reference's [u8; 2] (galois_16.rs:49-51)
    return np.array([v >> 8, v & 255], np.uint8)


def value(s):
    return (int(s[0]) << 8) | int(s[1])


def test_plan_shape(walk):
    assert walk["plan"] == {"k": K, "p": P, "n": 512, "u": 12, "nblk": 16}
    assert len(walk["enc"]) == P and all(len(r) == 12 for r in walk["enc"])


def test_plan_parity_rows_are_the_codec_matrix(walk, codec):
    m = codec.matrix()[K:].astype(np.int64)
    want = (m[:, :, 0] << 8) | m[:, :, 1]
    assert (np.asarray(walk["row"], np.int64) == want).all()


def test_plan_parity_of_a_column_equals_the_oracle(walk, codec):
    data, parity = walk["data"][0], walk["parity"][0]
    assert len(data) == K and len(parity) == P and any(data)
    sh = [shard(v) for v in data] + [np.zeros(2, np.uint8) for _ in range(P)]
    codec.encode(sh)
    assert parity == [value(s) for s in sh[K:]]


def test_plan_pattern_rebuilds_what_the_oracle_rebuilds(walk, codec):
    data, parity = walk["data"][0], walk["parity"][0]
    lost = walk["lost"][0]
    assert lost == [3, 77, 499, K + 1, K + 11]
    assert len(walk["pat"]) == len(lost)
    sh = [shard(v) for v in data + parity]
    for q in lost:
        sh[q][:] = 0
    codec.reconstruct(sh, [i not in lost for i in range(K + P)])
    want = [value(sh[q]) for q in lost]
    assert want == [(data + parity)[q] for q in lost]
    assert walk["rebuilt"][0] == want
    assert walk["rebuilt_rows"][0] == want


def test_plan_bit_matrix_multiplies_as_the_field(walk):
    got, want = walk["bitmul"][0]
    assert got == want and want != 0


def test_plan_walk_is_clean_under_sanitizers(tmp_path, walk):
    out = build_and_run(tmp_path, "fft16_plan_san",
                        ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert parse(out) == walk
