"""What rse_update_plan.hpp adds for rse_update_shards -- the 16-byte-path
decision over every shard pointer, new_data, a block's bytes and a shard's
bytes; a run's byte length in its block; the spans of a run counted in spans of
a full block, those past a shorter last block's end empty -- walked on the CPU
by tests/native/update_shards_plan.cpp over the cut of
rse_scrub_shards_plan.hpp.  The program checks the vector decision with one of
several pointers, or new_data, off by 1, 8 and 16 and with B x esize or len x
esize off a multiple of 16, and every run's bytes, spans and lanes against a
brute-force restatement for every (len, block_len) with len <= 70 and
block_len <= len + 1 and for sizes around 4096 and 8192; then the grid.  It
prints failures only; the totals are recomputed here.

The same program also runs under ASan + UBSan (host code only)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "reed-solomon-erasure_amd", "csrc")
SRC = os.path.join(HERE, "native", "update_shards_plan.cpp")
SPAN = 256 * 16  # bytes of a shard one work item covers


def build_and_run(tmp_path, name, flags):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, *flags, SRC, "-o",
                    str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    return res.stdout


def run_shapes():
    """(len, block_len, esize) of the run walk, in the program's order."""
    for esize in (1, 2):
        for length in range(1, 71):
            for block_len in range(0, length + 2):
                yield length, block_len, esize
    for block_len in (4095, 4096, 4097, 4112, 8191, 8192, 8193):
        for tail in (0, 1, 15, 16, 32, 4095, 4096, 4097, 8192):
            if tail < block_len:
                yield 2 * block_len + tail, block_len, 1
    for block_len in (2047, 2048, 2049, 4096):
        for tail in (0, 1, 8, 2047, 2048):
            if tail < block_len:
                yield block_len + tail, block_len, 2


def expected_summary():
    # per shape: all aligned once, then new_data and three pointers off by 1, 8, 16;
    # on for the aligned set and the four with an offset of 16
    vec_shapes = [(64, 16), (64, 0), (64, 100), (64, 24), (72, 16), (17, 5), (2056, 1024),
                  (4144, 1024), (1, 0)]
    vec_cases = vec_on = 0
    for esize in (1, 2):
        for length, block_len in vec_shapes:
            b = length if block_len == 0 or block_len > length else block_len
            vec_cases += 13
            if (b * esize) % 16 == 0 and (length * esize) % 16 == 0:
                vec_on += 5
    shapes = blocks = spans = empty = 0
    for length, block_len, esize in run_shapes():
        b = length if block_len == 0 or block_len > length else block_len
        n_blocks = -(-length // b)
        per_run = -(-(b * esize) // SPAN)
        shapes += 1
        blocks += n_blocks
        spans += n_blocks * per_run
        tail = (length % b) * esize
        if tail:
            empty += per_run - -(-tail // SPAN)
    return ("vec %d of %d shapes %d blocks %d spans %d empty %d failures 0"
            % (vec_on, vec_cases, shapes, blocks, spans, empty))


def test_walk(tmp_path):
    out = build_and_run(tmp_path, "update_shards_plan", ["-O1"])
    assert out.strip() == expected_summary()


def test_walk_is_clean_under_sanitizers(tmp_path):
    out = build_and_run(tmp_path, "update_shards_plan_san",
                        ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert out.strip() == expected_summary()
