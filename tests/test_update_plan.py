"""The host-side plan of rse_update_flat (rse_update_plan.hpp: the in-order
predicate the device pre-pass also calls, the run heads, the parity-row groups,
the 16-byte-path decision, the spans and lanes of a work item, the workgroup
count), walked on the CPU by tests/native/update_plan.cpp.  The program checks
every list of 1..4 entries over stripe and shard values 0..3 (n_stripes = 3,
k = 3) against a brute-force restatement, the row groups for p = 1..255, the
spans for the multiples of 16 up to 70,000 and their neighbours, the vector
decision on base pairs with one base off by 1, 8 and 16, and the grid.  It
prints failures only; the totals are recomputed here.

The same program also runs under ASan + UBSan (host code only)."""
import itertools
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "reed-solomon-erasure_amd", "csrc")
SRC = os.path.join(HERE, "native", "update_plan.cpp")
SPAN = 256 * 16  # bytes of a shard one work item covers


def build_and_run(tmp_path, name, flags):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, *flags, SRC, "-o",
                    str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    return res.stdout


def expected_summary():
    lists = sum(16 ** n for n in range(1, 5))
    # accepted lists are the ascending selections of distinct in-range entries
    entries = [(s, h) for s in range(3) for h in range(3)]
    accepted = runs = 0
    for n in range(1, 5):
        for pick in itertools.combinations(entries, n):
            accepted += 1
            runs += len({s for s, _ in pick})
    groups = sum(-(-p // 16) for p in range(1, 256))
    lengths = [b for b in range(1, 70001) if b % 16 in (0, 1, 15)]
    spans = sum(-(-b // SPAN) for b in lengths)
    # per shard length: both bases aligned once, then either base off by 1, 8, 16
    vec_lengths = (1, 8, 15, 16, 17, 32, 48, 1024, 4096 + 37, 16384 + 48)
    vec_cases = len(vec_lengths) * 7
    vec_on = sum(3 for b in vec_lengths if b % 16 == 0)  # aligned, and each base off by 16
    return ("lists %d accepted %d runs %d groups %d lengths %d spans %d vec %d of %d failures 0"
            % (lists, accepted, runs, groups, len(lengths), spans, vec_on, vec_cases))


def test_walk(tmp_path):
    out = build_and_run(tmp_path, "update_plan", ["-O1"])
    assert out.strip() == expected_summary()


def test_walk_is_clean_under_sanitizers(tmp_path):
    out = build_and_run(tmp_path, "update_plan_san",
                        ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert out.strip() == expected_summary()
