"""What rse_read_shards adds to the host-side plan of rse_read_flat
(rse_read_plan.hpp): read_shards_vec, the 16-byte decision over the pointers
that are there; the run bytes, spans and lanes of a shorter last block
(rse_update_plan.hpp over the cut of rse_scrub_shards_plan.hpp); and
read_plan_run -- the function the device planner runs per touched block -- with
a set of shards that have no buffer, for every flag row and every such set of
3+2 and 4+3 against the same function without the set on the row with those
flags cleared.  Walked on the CPU by tests/native/read_shards_plan.cpp, which
prints failures only; the totals are recomputed here.

The same program also runs under ASan + UBSan (host code only, a stand-alone
binary).  tests/test_read_plan.py, unchanged, is the check that the planner
without such a set is what it was."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "reed-solomon-erasure_amd", "csrc")
SRC = os.path.join(HERE, "native", "read_shards_plan.cpp")
SPAN = 256 * 16  # bytes of a shard one work item covers

# {block bytes, shard bytes} of the vector walk; {len, block_len} of the cut walk
VEC_LENGTHS = [(16, 48), (16, 40), (1024, 4096 + 48), (1024, 2048 + 8), (17, 34), (8, 16),
               (4112, 3 * 4112 + 32), (48, 96), (64, 64), (1, 1)]
CUT_SHAPES = [(1, 0), (17, 5), (4096 + 48, 1024), (3 * 4112 + 32, 4112), (2 * 1024 + 8, 1024),
              (64, 100), (16, 16), (3 * 272, 272), (96, 48), (18, 8), (4128, 2064),
              (2 * 8192 + 4097, 8192), (70000, 69999), (12288 + 1, 12288)]


def build_and_run(tmp_path, name, flags):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, *flags, SRC, "-o",
                    str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    return res.stdout


def expected_summary():
    # per length pair: 16 NULL subsets of aligned pointers; each of 4 pointers off
    # by 1, 8, 16 with one of the others (or none) NULL; `out` off by 1, 8, 16
    vec_cases = len(VEC_LENGTHS) * (16 + 4 * 3 * 4 + 3)
    vec_on = sum(16 + 4 * 4 + 1 for b, n in VEC_LENGTHS if b % 16 == 0 and n % 16 == 0)
    blocks = spans = empty = 0
    for length, block_len in CUT_SHAPES:
        b = length if block_len == 0 or block_len > length else block_len
        per_block = -(-b // SPAN)
        for first in range(0, length, b):
            run = min(b, length - first)
            blocks += 1
            spans += -(-run // SPAN)
            empty += per_block - -(-run // SPAN)
    rows = flagless = copied = rebuilt = lost = 0
    for k, p in ((3, 2), (4, 3)):
        T = k + p
        for bits in range(1 << T):
            for null_set in range(1 << T):
                times = 2 if bits == (1 << T) - 1 else 1  # `present` == NULL as well
                there = bin(bits & ~null_set).count("1")
                rows += times
                flagless += times - 1
                copied += times * there
                if there >= k:
                    rebuilt += times * (T - there)
                else:
                    lost += times * (T - there)
    return ("vec %d of %d shapes %d blocks %d spans %d empty %d rows %d flagless %d copied %d "
            "rebuilt %d lost %d failures 0"
            % (vec_on, vec_cases, len(CUT_SHAPES), blocks, spans, empty, rows, flagless, copied,
               rebuilt, lost))


def test_walk(tmp_path):
    out = build_and_run(tmp_path, "read_shards_plan", ["-O1"])
    assert out.strip() == expected_summary()


def test_walk_is_clean_under_sanitizers(tmp_path):
    out = build_and_run(tmp_path, "read_shards_plan_san",
                        ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert out.strip() == expected_summary()
