"""The host-side plan of rse_read_flat (rse_read_plan.hpp: the scope and
in-order predicates the entry and the device list pass call, the output groups,
the 16-byte-path decision, the grid, and read_plan_run -- the function the
device planner runs per touched stripe), walked on the CPU by
tests/native/read_plan.cpp.  The program checks every list of 1..4 entries over
stripe values 0..3 and shard values 0..5 (n_stripes = 3, k + p = 5) against a
brute-force restatement; the run planner for every flag row of 3+2, 4+3, 5+4
and 2+6 and for 200 seeded flag rows each of 100+28 and 128+128, every shard
wanted, against Matrix<Gf8Field>: M[r] (M[first k present])^-1; the groups for
1..256 entries; spans, lanes, the vector decision and the grid.  It prints
failures only; the totals are recomputed here.

The same program also runs under ASan + UBSan (host code only)."""
import itertools
import math
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "reed-solomon-erasure_amd", "csrc")
SRC = os.path.join(HERE, "native", "read_plan.cpp")
SPAN = 256 * 16  # bytes of a shard one work item covers


def build_and_run(tmp_path, name, flags):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, *flags, SRC, "-o",
                    str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    return res.stdout


def class_totals(k, p, erased_counts):
    """(copied, rebuilt, lost) over flag rows with the given numbers of erased
    shards, every shard wanted: the present ones are copied, the erased ones
    rebuilt where at most p are erased."""
    copied = rebuilt = lost = 0
    for erased in erased_counts:
        copied += k + p - erased
        if erased <= p:
            rebuilt += erased
        else:
            lost += erased
    return copied, rebuilt, lost


def expected_summary():
    lists = sum(24 ** n for n in range(1, 5))
    # accepted lists are the ascending selections of distinct in-range entries
    entries = [(s, h) for s in range(3) for h in range(5)]
    accepted = runs = 0
    for n in range(1, 5):
        for pick in itertools.combinations(entries, n):
            accepted += 1
            runs += len({s for s, _ in pick})
    rows = 0
    small = [0, 0, 0]
    for k, p in ((3, 2), (4, 3), (5, 4), (2, 6)):
        T = k + p
        rows += 2 ** T
        counts = [e for e in range(T + 1) for _ in range(math.comb(T, e))]
        small = [a + b for a, b in zip(small, class_totals(k, p, counts))]
    seeded = [0, 0, 0]
    for k, p in ((100, 28), (128, 128)):
        seeded = [a + b for a, b in zip(seeded, class_totals(k, p, [n % (p + 2) for n in range(200)]))]
    groups = sum(-(-n // 16) for n in range(1, 257))
    lengths = [b for b in range(1, 70001) if b % 16 in (0, 1, 15)]
    spans = sum(-(-b // SPAN) for b in lengths)
    # per shard length: both bases aligned once, then either base off by 1, 8, 16
    vec_lengths = (1, 8, 15, 16, 17, 32, 48, 1024, 4096 + 37, 16384 + 48)
    vec_cases = len(vec_lengths) * 7
    vec_on = sum(3 for b in vec_lengths if b % 16 == 0)  # aligned, and each base off by 16
    return ("lists %d accepted %d runs %d rows %d copied %d rebuilt %d lost %d seeded 400 copied %d "
            "rebuilt %d lost %d groups %d lengths %d spans %d vec %d of %d failures 0"
            % (lists, accepted, runs, rows, *small, *seeded, groups, len(lengths), spans, vec_on,
               vec_cases))


def test_walk(tmp_path):
    out = build_and_run(tmp_path, "read_plan", ["-O1"])
    assert out.strip() == expected_summary()


def test_walk_is_clean_under_sanitizers(tmp_path):
    out = build_and_run(tmp_path, "read_plan_san",
                        ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert out.strip() == expected_summary()
