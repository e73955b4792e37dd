// What rse_update_plan.hpp adds for rse_update_shards, walked on the CPU over
// the cut of rse_scrub_shards_plan.hpp.
//  * The 16-byte path is on exactly when every shard pointer, new_data, a
//    block's bytes and a shard's bytes are multiples of 16: pointer sets of 14
//    with one entry (first, middle, last) or new_data off by 1, 8 and 16, over
//    (len, block_len) pairs whose B x esize or len x esize leave a multiple of 16.
//  * A run's byte length, its spans and its lanes, against a brute-force
//    restatement -- byte x of block b of a shard of `bytes` bytes exists iff
//    b * block_bytes + x < bytes, x < block_bytes: the items of a run, counted
//    in spans of a FULL block, must cover exactly those bytes, each once, 16 per
//    lane with only the last lane short, and the spans past a short block's end
//    must be empty.  Every (len, block_len) with len <= 70 and block_len <=
//    len + 1 at element sizes 1 and 2, then sizes around 4096 and 8192.
//  * The workgroup count is update_grid over the entries and a full block's
//    bytes.
// Prints one line per failure and a summary line; exit status 1 on a failure.
// Built and run by tests/test_update_shards_plan.py, also under ASan + UBSan.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rse_scrub_shards_plan.hpp"
#include "rse_update_plan.hpp"

namespace {

int g_fail = 0;

void fail(const char* what, uint64_t a, uint64_t b, uint64_t got, uint64_t want) {
  std::printf("fail %s at %llu / %llu got %llu want %llu\n", what, (unsigned long long)a,
              (unsigned long long)b, (unsigned long long)got, (unsigned long long)want);
  ++g_fail;
}

#define CHECK_EQ(what, a, b, got, want)                                          \
  do {                                                                           \
    if ((uint64_t)(got) != (uint64_t)(want))                                     \
      fail(what, (uint64_t)(a), (uint64_t)(b), (uint64_t)(got), (uint64_t)(want)); \
  } while (0)

uint64_t walk_vec(uint64_t* cases) {
  uint64_t on = 0;
  const uintptr_t base = 0x10000, nd = 0x80000;
  // {len, block_len} in bytes (esize 1) and in 2-byte elements (esize 2)
  const uint64_t shapes[][2] = {{64, 16}, {64, 0},  {64, 100}, {64, 24}, {72, 16},
                                {17, 5},  {2056, 1024}, {4144, 1024}, {1, 0}};
  for (uint64_t esize = 1; esize <= 2; ++esize)
    for (const auto& sh : shapes)
      for (int at = -2; at < 14; ++at) {  // -2: all aligned; -1: new_data off; else that pointer
        if (!(at < 1 || at == 7 || at == 13)) continue;
        for (uintptr_t off : {uintptr_t(1), uintptr_t(8), uintptr_t(16)}) {
          if (at == -2 && off != 1) continue;  // all aligned: once
          std::vector<const void*> p;
          for (int i = 0; i < 14; ++i)
            p.push_back(reinterpret_cast<const void*>(base + 0x1000u * i + (i == at ? off : 0)));
          const void* const new_data = reinterpret_cast<const void*>(nd + (at == -1 ? off : 0));
          const rse::ScrubShardsPlan pl =
              rse::scrub_shards_plan(sh[0], sh[1], esize, p.data(), p.size(), false);
          const bool got = rse::update_shards_vec(p.data(), p.size(), new_data, pl.block_bytes,
                                                  sh[0] * esize);
          const uint64_t B = sh[1] == 0 || sh[1] > sh[0] ? sh[0] : sh[1];
          const bool want = (at == -2 || off % 16 == 0) && (B * esize) % 16 == 0 &&
                            (sh[0] * esize) % 16 == 0;
          CHECK_EQ("vec", sh[0] * 1000 + sh[1], at * 100 + (int)off, got, want);
          // where it is on, the shorter last block ends on a boundary too
          if (got) CHECK_EQ("vec tail", sh[0], sh[1], pl.tail_bytes % 16, 0);
          ++*cases;
          on += got ? 1 : 0;
        }
      }
  return on;
}

struct RunTotals {
  uint64_t shapes = 0, blocks = 0, spans = 0, empty = 0;
};

// One (len, block_len, esize): every block's run against the restatement.
void walk_shape(uint64_t len, uint64_t block_len, uint64_t esize, RunTotals& t) {
  const rse::ScrubShardsPlan pl = rse::scrub_shards_plan(len, block_len, esize, nullptr, 0, false);
  const uint64_t bytes = len * esize;
  ++t.shapes;
  CHECK_EQ("n_full fits", len, block_len, pl.n_full + (pl.tail_bytes != 0 ? 1 : 0), pl.n_blocks);
  const uint64_t n_spans = rse::update_spans(pl.block_bytes);  // of every run's items
  std::vector<uint8_t> hit(pl.block_bytes);
  for (uint64_t b = 0; b < pl.n_blocks; ++b) {
    ++t.blocks;
    const uint64_t run =
        rse::update_run_bytes(pl.block_bytes, pl.tail_bytes, (uint32_t)pl.n_full, (uint32_t)b);
    // the restatement: the bytes of block b that exist
    uint64_t want = 0;
    for (uint64_t x = 0; x < pl.block_bytes; ++x) want += b * pl.block_bytes + x < bytes ? 1 : 0;
    CHECK_EQ("run bytes", len * 1000 + block_len, b, run, want);
    CHECK_EQ("run bytes, the cut's", len * 1000 + block_len, b, run,
             rse::scrub_block_len(pl, len, b) * esize);
    hit.assign(pl.block_bytes, 0);
    for (uint64_t s = 0; s < n_spans; ++s) {
      const uint64_t sl = rse::update_run_span_len(run, s);
      ++t.spans;
      if (sl == 0) {  // sat out: the run ends at or before this span
        ++t.empty;
        if (rse::update_span_first(s) < run) fail("empty span", len, s, rse::update_span_first(s), run);
      }
      if (sl > rse::kUpdSpanBytes) fail("span length", len, s, sl, rse::kUpdSpanBytes);
      bool ended = false;
      for (uint32_t lane = 0; lane < rse::kUpdBlock; ++lane) {
        const uint32_t n = rse::update_lane_len(sl, lane);
        if (n == 0) {
          ended = true;
          continue;
        }
        if (ended) fail("lane after the end", len, lane, n, 0);
        if (n > 16) fail("lane length", len, lane, n, 16);
        const uint64_t off = rse::update_span_first(s) + (uint64_t)lane * rse::kUpdLaneBytes;
        for (uint32_t x = 0; x < n; ++x) {
          // in bounds of the shard, and no byte twice
          if (off + x >= pl.block_bytes || b * pl.block_bytes + off + x >= bytes)
            fail("out of bounds", len * 1000 + block_len, b, off + x, run);
          else
            ++hit[off + x];
        }
      }
    }
    for (uint64_t x = 0; x < pl.block_bytes; ++x)
      CHECK_EQ("covered once", len * 1000 + block_len, x, hit[x], x < want ? 1 : 0);
  }
}

void walk_runs(RunTotals& t) {
  for (uint64_t esize = 1; esize <= 2; ++esize)
    for (uint64_t len = 1; len <= 70; ++len)
      for (uint64_t block_len = 0; block_len <= len + 1; ++block_len)
        walk_shape(len, block_len, esize, t);
  // around one and two spans: the block, and a tail on either side of a span's end
  for (uint64_t block_len : {4095u, 4096u, 4097u, 4112u, 8191u, 8192u, 8193u})
    for (uint64_t tail : {0u, 1u, 15u, 16u, 32u, 4095u, 4096u, 4097u, 8192u})
      if (tail < block_len) walk_shape(2 * block_len + tail, block_len, 1, t);
  for (uint64_t block_len : {2047u, 2048u, 2049u, 4096u})
    for (uint64_t tail : {0u, 1u, 8u, 2047u, 2048u})
      if (tail < block_len) walk_shape(block_len + tail, block_len, 2, t);
}

void walk_grid() {
  // a full block's bytes count the items, whatever the tail is
  const rse::ScrubShardsPlan pl = rse::scrub_shards_plan(3 * 4112 + 32, 4112, 1, nullptr, 0, false);
  CHECK_EQ("grid items", 0, 0, rse::update_grid(256, 0, 3, pl.block_bytes), 6);
  CHECK_EQ("grid fill", 0, 1, rse::update_grid(256, 0, 5000, pl.block_bytes), 256 * rse::kUpdPerCu);
  CHECK_EQ("grid option", 0, 2, rse::update_grid(256, 3, 5000, pl.block_bytes), 3);
  const rse::ScrubShardsPlan one = rse::scrub_shards_plan(64, 100, 2, nullptr, 0, false);
  CHECK_EQ("grid one block", 0, 3, rse::update_grid(256, 0, 2, one.block_bytes), 2);
}

}  // namespace

int main() {
  uint64_t vec_cases = 0;
  const uint64_t vec_on = walk_vec(&vec_cases);
  RunTotals t;
  walk_runs(t);
  walk_grid();
  std::printf("vec %llu of %llu shapes %llu blocks %llu spans %llu empty %llu failures %d\n",
              (unsigned long long)vec_on, (unsigned long long)vec_cases,
              (unsigned long long)t.shapes, (unsigned long long)t.blocks,
              (unsigned long long)t.spans, (unsigned long long)t.empty, g_fail);
  return g_fail == 0 ? 0 : 1;
}
