"""The column decoder of rse_correct_flat (rse_correct_plan.hpp: error values
by Forney's formula, erasures through the erasure locator), walked on the CPU by
tests/native/correct_plan.cpp -- the decoder is the very code the kernel runs --
and compared with a brute-force model (tests/correct_model.py: position sets
and Gaussian elimination over the ORACLE's matrix; no syndromes, no
Berlekamp-Massey):

- the plan's 1 / u_r times the u_r of the check matrix is 1 for every shard;
- for seeded columns of 3+2, 6+4 and 4+5 with nu wrong and f erased shards
  (every pair with nu <= p, f <= p + 1, nu + f <= n; erased shards hold
  arbitrary bytes): the decoder's verdict and corrected bytes are the model's,
  and whenever 2 nu + f <= p they are the original codeword;
- past that capacity both outcomes occur: undecodable columns, and columns
  decoded to ANOTHER codeword (the inherent limit);
- the ends of the point shift (shards 0, n-1, 254) and the limits of the
  capacity on 10+4 and 239+16;
- for codecs of every parity count 6 .. 16 (NO = 8 and NO = 16 of the kernel,
  full and partly filled) a seeded grid of every (f, nu) with 2 nu + f <= p:
  the decoded column is the codeword the column was made from.  The expected
  value is the injection's, checked in the program; it prints only failures.

The same program also runs under ASan + UBSan (host code only)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from oracle import oracle as O  # noqa: E402
import correct_model as CM  # noqa: E402

CSRC = os.path.join(HERE, "..", "reed-solomon-erasure_amd", "csrc")
SRC = os.path.join(HERE, "native", "correct_plan.cpp")
# every parity count 6 .. 16 (and 3): k = 1, one chunk of the kernel's tables
# (k <= 128 at p > 8) and more than one, the widest codec
GRID = [(20, 8), (6, 9), (30, 15), (12, 12), (5, 6), (7, 7), (40, 10), (200, 11), (50, 13),
        (60, 14), (1, 16), (128, 16), (129, 16), (100, 16), (239, 16), (2, 3)]
PLANS = [(10, 4), (3, 2), (4, 5), (17, 3), (1, 1)] + GRID
GRID_COLS = 40  # per group, as tests/native/correct_plan.cpp
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
    return parse(build_and_run(tmp_path_factory.mktemp("correct_plan"), "correct_plan", ["-O1"]))


@pytest.mark.parametrize("k,p", PLANS)
def test_inverse_of_u(walk, k, p):
    mul = O.gf8_tables()[2]
    iu, u = walk[("iu", k, p)][0], walk[("u", k, p)][0]
    assert len(iu) == len(u) == k + p
    assert all(int(mul[a, b]) == 1 for a, b in zip(iu, u))


def columns(walk, k, p, pick):
    """(original codeword, received, erased, injected, decoder's column or None)."""
    out = []
    for idx in sorted(walk[("rx", k, p)]):
        if not pick(idx):
            continue
        res = walk[("res", k, p)][idx]
        got = None if res[0] == BAD else res[1:]
        assert got is None or len(got) == k + p
        out.append((walk[("cw", k, p)][idx], walk[("rx", k, p)][idx], walk[("era", k, p)][idx],
                    walk[("inj", k, p)][idx], got))
    return out


@pytest.fixture(scope="module")
def small(walk):
    """Per codec: every seeded column with the model's corrected column beside it."""
    out = {}
    for k, p in SMALL:
        hc = CM.check_matrix(k, p)
        out[(k, p)] = [(cw, rx, era, inj, got, CM.correct_column(hc, rx, era, p))
                       for cw, rx, era, inj, got in columns(walk, k, p, lambda i: i < 100000)]
    return out


def groups(k, p):
    n = k + p
    return [(nu, f) for nu in range(p + 1) for f in range(p + 2) if nu + f <= n]


@pytest.mark.parametrize("k,p", SMALL)
def test_decoder_equals_the_model(small, k, p):
    v = small[(k, p)]
    g = groups(k, p)
    assert len(v) == 40 * len(g)
    for i, (cw, rx, era, inj, got, model) in enumerate(v):
        assert (len(inj), len(era)) == g[i // 40]
        assert got == model, (rx, era, inj, got, model)
        if 2 * len(inj) + len(era) <= p:
            assert got == cw, (rx, era, inj, got)
        if len(era) > p:
            assert got is None


@pytest.mark.parametrize("k,p", SMALL)
def test_past_capacity_both_outcomes_occur(small, k, p):
    over = [(cw, got) for cw, rx, era, inj, got, model in small[(k, p)]
            if 2 * len(inj) + len(era) > p and len(era) <= p]
    assert over
    assert any(got is None for _, got in over)                      # undecodable
    assert any(got is not None and got != cw for cw, got in over)   # another codeword


@pytest.mark.parametrize("k,p", [(10, 4), (239, 16)])
def test_edges(walk, k, p):
    n, t = k + p, p // 2
    hc = CM.check_matrix(k, p)
    edge = columns(walk, k, p, lambda i: i >= 100000)
    assert len(edge) == 12
    cases = dict(zip(range(100000, 100012), edge))
    assert cases[100000][3] == [0] and cases[100001][3] == [n - 1]
    assert cases[100002][3] == [0, n - 1]
    assert len(cases[100003][3]) == t and {0, n - 1} <= set(cases[100003][3])
    assert len(cases[100004][2]) == p and len(cases[100005][2]) == p
    assert len(cases[100006][2]) == p - 2 and len(cases[100007][2]) == p - 2
    assert len(cases[100008][2]) == p - 1 and len(cases[100008][3]) == 1
    assert len(cases[100009][2]) == p + 1
    assert len(cases[100010][2]) == 2 and len(cases[100010][3]) == (p - 2) // 2
    for idx, (cw, rx, era, inj, got) in cases.items():
        if 2 * len(inj) + len(era) <= p:
            assert got == cw, (idx, era, inj)
        if len(inj) <= 1:  # the model's search stays small: nu <= 1
            assert got == CM.correct_column(hc, rx, era, p), idx
    assert cases[100009][4] is None  # more erasures than checks


@pytest.mark.parametrize("k,p", GRID)
def test_grid_inside_capacity_decodes_to_the_codeword(walk, k, p):
    groups = sum(1 for f in range(p + 1) for nu in range(p + 1) if 2 * nu + f <= p)
    assert ("gridfail", k, p) not in walk, sorted(walk[("gridfail", k, p)].items())[:8]
    assert walk[("grid", k, p)][0] == [GRID_COLS * groups, 0]


def test_walk_is_clean_under_sanitizers(tmp_path, walk):
    out = build_and_run(tmp_path, "correct_plan_san",
                        ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert parse(out) == walk
