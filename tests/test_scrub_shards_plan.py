"""The host-side block plan of rse_scrub_shards (rse_scrub_shards_plan.hpp: B,
the block counts, the last block's bytes, whether the repair sweep may read 16
bytes per lane, whether the block length admits the pre-filter), walked on the
CPU by tests/native/scrub_shards_plan.cpp.  For every len in 1..70 and
block_len in 0..72 at element sizes 1 and 2 the program checks that the blocks
tile [0, len) exactly and in order, that only the last block is short, the
counts against ceil(len / min(block_len, len)), and the vector path against
"every pointer and the block's bytes are multiples of 16" on pointer sets with
one entry off by 1, by 8 and by 16; then the lengths that admit the
pre-filter, block_len 0 and block_len > len as one block, and 2^33 blocks.  It
prints failures only; the totals are recomputed here.

The same program also runs under ASan + UBSan (host code only)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "reed-solomon-erasure_amd", "csrc")
SRC = os.path.join(HERE, "native", "scrub_shards_plan.cpp")


def build_and_run(tmp_path, name, flags):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, *flags, SRC, "-o",
                    str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    return res.stdout


def expected_summary():
    plans = vec = 0
    for esize in (1, 2):
        for length in range(1, 71):
            for block_len in range(0, 73):
                b = length if block_len == 0 or block_len > length else block_len
                plans += 10  # pointer sets: aligned; one of three entries off by 1, 8, 16
                if (b * esize) % 16 == 0:
                    vec += 4  # the aligned set and the three with an entry off by 16
    # 7 lengths x 2 block lengths x sub-chunks off / on, and the 2^33-block plan
    plans += 7 * 2 * 2 + 1
    pre = 2 * (2 * 1 + 3 * 2)  # 1 KiB, 2 KiB with sub-chunks; 4096, 4096 + 16, 1 MiB always
    return "plans %d vec %d prefilter %d failures 0" % (plans, vec, pre)


def test_walk(tmp_path):
    out = build_and_run(tmp_path, "scrub_shards_plan", ["-O1"])
    assert out.strip() == expected_summary()


def test_walk_is_clean_under_sanitizers(tmp_path):
    out = build_and_run(tmp_path, "scrub_shards_plan_san",
                        ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert out.strip() == expected_summary()
