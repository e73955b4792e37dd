"""The host plan and the column decoder of rse_locate_flat
(rse_locate_plan.hpp), walked on the CPU by tests/native/locate_plan.cpp -- the
decoder is the very code the kernel runs -- and compared with the oracle:

- the check matrix H of every codec annihilates the oracle's encoding matrix
  (H M = 0) and T [P | I] = H, with P the oracle's parity rows: the syndromes
  the kernel forms from d = P data ^ parity are those of the column;
- for seeded columns of 3+2, 6+4 and 4+5 with 0 .. p wrong shards, every column
  a brute-force model (tests/locate_model.py: position sets and ranks, no
  Berlekamp-Massey) finds decodable gets exactly the model's bad shards, and
  with at most t wrong shards those are the injected ones;
- columns with more than t wrong shards: decoder and model agree, and both
  outcomes occur -- undecodable columns, and columns within t of ANOTHER
  codeword (the inherent limit: innocent shards are named);
- errors at the ends of the point shift: shard 0, shard n-1, shard 254;
- for codecs of every parity count 6 .. 16 a seeded grid of 0 .. t wrong
  shards: the decoder names exactly the injected shards, ascending.  The
  expected value is the injection's, checked in the program; it prints only
  failures.

The same program also runs under ASan + UBSan (host code only)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import oracle as O  # noqa: E402
import locate_model as LM  # noqa: E402

CSRC = os.path.join(HERE, "..", "reed-solomon-erasure_amd", "csrc")
SRC = os.path.join(HERE, "native", "locate_plan.cpp")
# every parity count 6 .. 16 (and 3): k = 1, one chunk of the kernel's tables
# (k <= 128 at p > 8) and more than one, the widest codec
GRID = [(20, 8), (6, 9), (30, 15), (12, 12), (5, 6), (7, 7), (40, 10), (200, 11), (50, 13),
        (60, 14), (1, 16), (128, 16), (129, 16), (100, 16), (239, 16), (2, 3)]
PLANS = [(10, 4), (3, 2), (4, 5), (17, 3), (1, 1)] + GRID
GRID_COLS = 40  # per group, as tests/native/locate_plan.cpp
SMALL = [(3, 2), (6, 4), (4, 5)]
BAD = 255


def parse(text):
    out = {}
    for line in text.splitlines():
        f = line.split()
        k, p, idx = int(f[1]), int(f[2]), int(f[3])
        out.setdefault((f[0], k, p), {})[idx] = [int(v) for v in f[4:]]
    return out


def build_and_run(tmp_path, name, flags):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, *flags, SRC, "-o",
                    str(exe)], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    return parse(build_and_run(tmp_path_factory.mktemp("locate_plan"), "locate_plan", ["-O1"]))


def rows(walk, tag, k, p):
    d = walk[(tag, k, p)]
    return np.array([d[i] for i in range(len(d))], np.uint8)


@pytest.mark.parametrize("k,p", PLANS)
def test_plan_matrices_against_the_oracle(walk, k, p):
    m = O.Codec(8, k, p).matrix()
    P, T, H = rows(walk, "P", k, p), rows(walk, "T", k, p), rows(walk, "H", k, p)
    assert P.shape == (p, k) and T.shape == (p, p) and H.shape == (p, k + p)
    assert (P == m[k:]).all()
    assert not O.matrix_multiply(8, H, m).any()  # H is a check matrix of the codec
    hc = np.concatenate([m[k:], np.eye(p, dtype=np.uint8)], axis=1)
    assert (O.matrix_multiply(8, T, hc) == H).all()
    # p independent checks: T is invertible (H has full rank)
    assert (O.matrix_multiply(8, T, O.matrix_invert(8, T)) == np.eye(p, dtype=np.uint8)).all()


def verdicts(walk, k, p):
    """(injected, decoder's result, model's result) of every seeded column."""
    hc = LM.check_matrix(k, p)
    rx, inj, res = walk[("rx", k, p)], walk[("inj", k, p)], walk[("res", k, p)]
    out = []
    for idx in sorted(rx):
        if idx >= 1000:
            continue
        d = LM.gf_matvec(hc, np.array(rx[idx], np.uint8))
        model = LM.column_bad_shards(hc, d, p // 2)
        got = None if res[idx][0] == BAD else tuple(sorted(res[idx][1:]))
        if got is not None:
            assert len(got) == res[idx][0]
        out.append((tuple(sorted(inj[idx])), got, model))
    return out


@pytest.fixture(scope="module")
def small(walk):
    return {kp: verdicts(walk, *kp) for kp in SMALL}


@pytest.mark.parametrize("k,p", SMALL)
def test_decodable_columns_get_the_models_bad_shards(small, k, p):
    t = p // 2
    v = small[(k, p)]
    assert len(v) == 40 * (p + 1)
    decodable = [(inj, got, model) for inj, got, model in v if model is not None]
    assert len(decodable) >= 40 * (t + 1)
    for inj, got, model in decodable:
        assert got == model, (inj, got, model)
        if len(inj) <= t:
            assert model == inj
    # a corrupted column is never called clean
    assert all(got != () for inj, got, _ in v if inj)
    # every column with at most t wrong shards is decodable
    assert all(model is not None for inj, _, model in v if len(inj) <= t)


def test_over_capacity_columns(small):
    mis = []
    for (k, p), v in small.items():
        t = p // 2
        over = [(inj, got, model) for inj, got, model in v if len(inj) > t]
        assert len(over) == 40 * (p - t)
        for inj, got, model in over:
            assert got == model, (k, p, inj, got, model)
        assert any(model is None for _, _, model in over)  # undecodable
        mis += [(inj, model) for inj, _, model in over if model is not None]
    # within t of ANOTHER codeword (rare: the program's seed was chosen so that the
    # group holds one): shards are named, and they are not the injected ones
    assert mis and all(model != inj for inj, model in mis)


def test_edge_positions(walk):
    for (k, p), cases in {(10, 4): {1000: [0], 1001: [13], 1002: [0, 13]},
                          (239, 16): {1000: [0], 1001: [254], 1002: [0, 254],
                                      1003: [0, 1, 100, 238, 239, 240, 253, 254],
                                      1004: []}}.items():
        for idx, want in cases.items():
            assert walk[("inj", k, p)][idx] == want
            res = walk[("res", k, p)][idx]
            assert res[0] == len(want) and sorted(res[1:]) == want, (k, p, idx, res)


@pytest.mark.parametrize("k,p", GRID)
def test_grid_up_to_t_wrong_shards_are_named(walk, k, p):
    assert ("gridfail", k, p) not in walk, sorted(walk[("gridfail", k, p)].items())[:8]
    assert walk[("grid", k, p)][0] == [GRID_COLS * (p // 2 + 1), 0]


def test_walk_is_clean_under_sanitizers(tmp_path, walk):
    out = build_and_run(tmp_path, "locate_plan_san",
                        ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert parse(out) == walk
