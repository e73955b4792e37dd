// The block plan of rse_scrub_shards (rse_scrub_shards_plan.hpp) walked on the
// CPU: for every len in 1..70 and block_len in 0..72 at element sizes 1 and 2
// the blocks must tile [0, len) in order with only the last one short, the
// counts must match the formula of include/rse_hip.h, and the 16-byte path must
// be on exactly when every pointer and the block's bytes are multiples of 16.
// Prints one line per failure and a summary line; exit status 1 on a failure.
// Built and run by tests/test_scrub_shards_plan.py, also under ASan + UBSan.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rse_scrub_shards_plan.hpp"

namespace {

int g_fail = 0;

void fail(const char* what, uint64_t len, uint64_t block_len, uint64_t esize, uint64_t got,
          uint64_t want) {
  std::printf("fail %s len %llu block_len %llu esize %llu got %llu want %llu\n", what,
              (unsigned long long)len, (unsigned long long)block_len, (unsigned long long)esize,
              (unsigned long long)got, (unsigned long long)want);
  ++g_fail;
}

#define CHECK_EQ(what, got, want)                                                  \
  do {                                                                             \
    if ((uint64_t)(got) != (uint64_t)(want))                                       \
      fail(what, len, block_len, esize, (uint64_t)(got), (uint64_t)(want));        \
  } while (0)

// Pointer sets of 14 entries: all aligned, then one entry (first, middle,
// last) off by 1, by 8 and by 16.
struct PtrSet {
  std::vector<const void*> p;
  bool aligned;
};

std::vector<PtrSet> pointer_sets() {
  const uintptr_t base = 0x10000;
  std::vector<PtrSet> out;
  const auto make = [&](int at, uintptr_t off) {
    PtrSet s;
    for (int i = 0; i < 14; ++i)
      s.p.push_back(reinterpret_cast<const void*>(base + 0x1000u * i + (i == at ? off : 0)));
    s.aligned = off % 16 == 0;
    return s;
  };
  out.push_back(make(-1, 0));
  for (int at : {0, 7, 13})
    for (uintptr_t off : {uintptr_t(1), uintptr_t(8), uintptr_t(16)}) out.push_back(make(at, off));
  return out;
}

}  // namespace

int main() {
  const std::vector<PtrSet> sets = pointer_sets();
  uint64_t plans = 0, vec_on = 0, pre_on = 0;
  for (uint64_t esize = 1; esize <= 2; ++esize)
    for (uint64_t len = 1; len <= 70; ++len)
      for (uint64_t block_len = 0; block_len <= 72; ++block_len) {
        const uint64_t B = block_len == 0 || block_len > len ? len : block_len;
        for (const PtrSet& s : sets) {
          const rse::ScrubShardsPlan pl =
              rse::scrub_shards_plan(len, block_len, esize, s.p.data(), s.p.size(), true);
          ++plans;
          CHECK_EQ("block_len", pl.block_len, B);
          CHECK_EQ("n_blocks", pl.n_blocks, (len + B - 1) / B);
          CHECK_EQ("n_full", pl.n_full, len / B);
          CHECK_EQ("block_bytes", pl.block_bytes, B * esize);
          CHECK_EQ("tail_bytes", pl.tail_bytes, (len % B) * esize);
          CHECK_EQ("short blocks", pl.n_blocks - pl.n_full, pl.tail_bytes != 0 ? 1 : 0);
          // the blocks tile [0, len) exactly, in order; only the last is short
          uint64_t next = 0;
          for (uint64_t b = 0; b < pl.n_blocks; ++b) {
            CHECK_EQ("first", rse::scrub_block_first(pl, b), next);
            const uint64_t bl = rse::scrub_block_len(pl, len, b);
            if (b + 1 < pl.n_blocks) CHECK_EQ("full block", bl, B);
            if (bl == 0 || bl > B) fail("block length", len, block_len, esize, bl, B);
            if (b + 1 == pl.n_blocks && pl.tail_bytes != 0) CHECK_EQ("tail", bl * esize, pl.tail_bytes);
            next += bl;
          }
          CHECK_EQ("tiling", next, len);
          const bool vec = s.aligned && (B * esize) % 16 == 0;
          CHECK_EQ("vec", pl.vec, vec);
          vec_on += pl.vec ? 1 : 0;
          // lengths up to 144 bytes never admit the pre-filter
          CHECK_EQ("len_prefilters", pl.len_prefilters, false);
        }
      }
  // the lengths the pre-filter admits: 1 KiB and 2 KiB with sub-chunks only, 4 KiB and more in
  // multiples of 16; block_len 0 and block_len > len are one block
  const uint64_t esize = 1;
  for (uint64_t len : {1024u, 2048u, 3072u, 4096u, 4096u + 8u, 4096u + 16u, 1u << 20})
    for (uint64_t block_len : {uint64_t(0), uint64_t(1) << 40})
      for (bool sub : {false, true}) {
        const rse::ScrubShardsPlan pl =
            rse::scrub_shards_plan(len, block_len, esize, sets[0].p.data(), 14, sub);
        ++plans;
        CHECK_EQ("one block", pl.n_blocks, 1);
        CHECK_EQ("one block, full", pl.n_full, 1);
        CHECK_EQ("one block, no tail", pl.tail_bytes, 0);
        const bool want = len % 16 == 0 && (len >= 4096 || (sub && (len == 1024 || len == 2048)));
        CHECK_EQ("len_prefilters", pl.len_prefilters, want);
        pre_on += pl.len_prefilters ? 1 : 0;
      }
  {  // 2^33 blocks: the count is not truncated
    const uint64_t len = uint64_t(1) << 33, block_len = 1;
    const rse::ScrubShardsPlan pl =
        rse::scrub_shards_plan(len, block_len, 2, sets[0].p.data(), 14, true);
    ++plans;
    CHECK_EQ("2^33 blocks", pl.n_blocks, len);
  }
  std::printf("plans %llu vec %llu prefilter %llu failures %d\n", (unsigned long long)plans,
              (unsigned long long)vec_on, (unsigned long long)pre_on, g_fail);
  return g_fail == 0 ? 0 : 1;
}
