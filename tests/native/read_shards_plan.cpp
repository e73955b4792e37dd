// What rse_read_shards adds to the plan of rse_read_flat (rse_read_plan.hpp),
// walked on the CPU.
//  * read_shards_vec: four shard pointers, each of them in turn off by 1, 8 or
//    16 bytes or NULL, every NULL subset of the aligned pointers, `out` off by
//    the same amounts, over block and shard lengths with and without a tail
//    that is a multiple of 16.  The 16-byte path is on exactly when every
//    non-NULL pointer, `out`, the block's bytes and the shard's bytes are
//    multiples of 16: a NULL pointer decides nothing.
//  * The cut (rse_scrub_shards_plan.hpp) and the run bytes, spans and lanes
//    the read kernel derives from it (rse_update_plan.hpp), for shards whose
//    last block is shorter: every block's run bytes are the block's own length,
//    the spans of a full block tile the run with empty spans after its end,
//    and the lanes tile every span.
//  * read_plan_run with a set of shards that have no buffer, for EVERY flag row
//    and EVERY such set of 3+2 and 4+3, every shard wanted in one run: the
//    recoverable verdict, the valid set, the classes and the coefficients must
//    equal those of read_plan_run without such a set on the flag row with
//    those flags cleared (which tests/native/read_plan.cpp checks against
//    matrix inversion) -- and no shard of the set may be in the valid set or
//    be copied.  Where the flag row is all ones, the NULL row (`present` ==
//    NULL) is walked as well.
// Prints one line per failure and a summary line; exit status 1 on a failure.
// Built and run by tests/test_read_shards_plan.py, also under ASan + UBSan.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rse_field.hpp"
#include "rse_read_plan.hpp"
#include "rse_scrub_shards_plan.hpp"

namespace {

int g_fail = 0;

void fail(const char* what, uint64_t a, uint64_t b, uint64_t got, uint64_t want) {
  if (g_fail < 50)
    std::printf("fail %s at %llu / %llu got %llu want %llu\n", what, (unsigned long long)a,
                (unsigned long long)b, (unsigned long long)got, (unsigned long long)want);
  ++g_fail;
}

#define CHECK_EQ(what, a, b, got, want)                                          \
  do {                                                                           \
    if ((uint64_t)(got) != (uint64_t)(want))                                     \
      fail(what, (uint64_t)(a), (uint64_t)(b), (uint64_t)(got), (uint64_t)(want)); \
  } while (0)

// ---- the 16-byte decision

struct VecTotals {
  uint64_t cases = 0, on = 0;
};

void check_vec(const uintptr_t* p, size_t n, uintptr_t out, uint64_t block, uint64_t len,
               VecTotals& t) {
  std::vector<const void*> ptrs(n);
  bool want = out % 16 == 0 && block % 16 == 0 && len % 16 == 0;
  for (size_t i = 0; i < n; ++i) {
    ptrs[i] = reinterpret_cast<const void*>(p[i]);
    if (p[i] != 0) want = want && p[i] % 16 == 0;
  }
  const bool got =
      rse::read_shards_vec(ptrs.data(), n, reinterpret_cast<const void*>(out), block, len);
  CHECK_EQ("vec", block, len, got, want);
  ++t.cases;
  t.on += got ? 1 : 0;
}

void walk_vec(VecTotals& t) {
  constexpr size_t n = 4;
  const uintptr_t base[n] = {0x10000, 0x20040, 0x30000, 0x7f0010}, out = 0x900000;
  // {block bytes, shard bytes}
  const uint64_t lengths[][2] = {{16, 48},     {16, 40},        {1024, 4096 + 48}, {1024, 2048 + 8},
                                 {17, 34},     {8, 16},         {4112, 3 * 4112 + 32},
                                 {48, 96},     {64, 64},        {1, 1}};
  for (const auto& l : lengths) {
    for (uint32_t null_set = 0; null_set < (1u << n); ++null_set) {  // aligned pointers, NULLs
      uintptr_t p[n];
      for (size_t i = 0; i < n; ++i) p[i] = (null_set >> i) & 1u ? 0 : base[i];
      check_vec(p, n, out, l[0], l[1], t);
    }
    for (size_t which = 0; which < n; ++which)
      for (uintptr_t off : {uintptr_t(1), uintptr_t(8), uintptr_t(16)})
        for (size_t null_at = 0; null_at <= n; ++null_at) {  // n: no NULL beside it
          if (null_at == which) continue;
          uintptr_t p[n];
          for (size_t i = 0; i < n; ++i) p[i] = i == null_at ? 0 : base[i] + (i == which ? off : 0);
          check_vec(p, n, out, l[0], l[1], t);
        }
    for (uintptr_t off : {uintptr_t(1), uintptr_t(8), uintptr_t(16)}) {
      uintptr_t p[n] = {base[0], 0, base[2], base[3]};
      check_vec(p, n, out + off, l[0], l[1], t);
    }
  }
}

// ---- the cut, and a run's bytes, spans and lanes

struct CutTotals {
  uint64_t shapes = 0, blocks = 0, spans = 0, empty_spans = 0;
};

void walk_cut(CutTotals& t) {
  // {len, block_len} in bytes (element size 1)
  const uint64_t shapes[][2] = {{1, 0},         {17, 5},          {4096 + 48, 1024},
                                {3 * 4112 + 32, 4112}, {2 * 1024 + 8, 1024}, {64, 100},
                                {16, 16},       {3 * 272, 272},   {96, 48},
                                {18, 8},        {4128, 2064},     {2 * 8192 + 4097, 8192},
                                {70000, 69999}, {12288 + 1, 12288}};
  const void* none[1] = {nullptr};
  for (const auto& s : shapes) {
    ++t.shapes;
    const uint64_t len = s[0];
    const rse::ScrubShardsPlan pl = rse::scrub_shards_plan(len, s[1], 1, none, 1, false);
    const uint64_t n_spans = rse::update_spans(pl.block_bytes);
    uint64_t covered = 0;
    for (uint64_t b = 0; b < pl.n_blocks; ++b) {
      ++t.blocks;
      const uint64_t run =
          rse::update_run_bytes(pl.block_bytes, pl.tail_bytes, (uint32_t)pl.n_full, (uint32_t)b);
      CHECK_EQ("run bytes", len, b, run, rse::scrub_block_len(pl, len, b));
      CHECK_EQ("block first", len, b, rse::scrub_block_first(pl, b), covered);
      uint64_t next = 0;
      for (uint64_t sp = 0; sp < n_spans; ++sp) {
        const uint64_t sl = rse::update_run_span_len(run, sp);
        if (sl == 0) {
          ++t.empty_spans;
          if (next != run) fail("span gap", len, sp, next, run);
          for (uint32_t lane = 0; lane < rse::kUpdBlock; ++lane)
            CHECK_EQ("lane of an empty span", len, lane, rse::update_lane_len(sl, lane), 0);
          continue;
        }
        ++t.spans;
        CHECK_EQ("span first", len, sp, rse::update_span_first(sp), next);
        if (sl > rse::kUpdSpanBytes) fail("span length", len, sp, sl, rse::kUpdSpanBytes);
        uint64_t lane_next = 0;
        for (uint32_t lane = 0; lane < rse::kUpdBlock; ++lane) {
          const uint32_t ln = rse::update_lane_len(sl, lane);
          if (ln > rse::kUpdLaneBytes) fail("lane length", len, lane, ln, rse::kUpdLaneBytes);
          if (ln != 0) CHECK_EQ("lane first", len, lane, (uint64_t)lane * rse::kUpdLaneBytes, lane_next);
          lane_next += ln;
        }
        CHECK_EQ("lanes tile", len, sp, lane_next, sl);
        next += sl;
      }
      CHECK_EQ("spans tile", len, b, next, run);  // the last byte a lane touches is the run's last
      covered += run;
    }
    CHECK_EQ("blocks tile", len, pl.n_blocks, covered, len);
  }
}

// ---- the run planner with shards that have no buffer

using Mat = rse::Matrix<rse::Gf8Field>;

std::vector<uint8_t> parity_rows(uint32_t k, uint32_t p) {
  const Mat v = Mat::vandermonde(k + p, k);
  Mat top(k, k), inv;
  for (uint32_t r = 0; r < k; ++r)
    for (uint32_t c = 0; c < k; ++c) top.at(r, c) = v.at(r, c);
  if (!top.invert(inv)) fail("codec matrix", k, p, 0, 1);
  const Mat m = v.multiply(inv);
  std::vector<uint8_t> P((size_t)p * k);
  for (uint32_t r = 0; r < p; ++r)
    for (uint32_t c = 0; c < k; ++c) P[(size_t)r * k + c] = (uint8_t)m.at(k + r, c);
  return P;
}

struct HostEmit {
  std::vector<int> cls_of;
  std::vector<int> coef_of;  // -1: not handed out
  uint32_t k;
  HostEmit(uint32_t n, uint32_t k_) : cls_of(n, -1), coef_of((size_t)n * k_, -1), k(k_) {}
  void cls(uint32_t j, uint8_t c) {
    if (cls_of[j] != -1) fail("class handed out twice", j, c, cls_of[j], -1);
    cls_of[j] = c;
  }
  void coef(uint32_t j, uint32_t i, uint8_t c) {
    if (coef_of[(size_t)j * k + i] != -1) fail("coefficient handed out twice", j, i, c, -1);
    coef_of[(size_t)j * k + i] = c;
  }
};

struct Work {
  std::vector<uint8_t> fl, where, valid, S, R, A, D;
  uint32_t sc[4];
  rse::ReadRunWork w;
  Work()
      : fl(rse::kReadMaxShards), where(rse::kReadMaxShards), valid(rse::kReadMaxShards),
        S(rse::kReadMaxP), R(rse::kReadMaxP), A(rse::kReadWorkA), D(rse::kReadWorkD),
        w{fl.data(), where.data(), valid.data(), S.data(), R.data(), A.data(), D.data(), sc} {}
};

struct PlanTotals {
  uint64_t rows = 0, copied = 0, rebuilt = 0, lost = 0, null_rows = 0;
};

void walk_null_sets(uint32_t k, uint32_t p, PlanTotals& t) {
  const uint32_t T = k + p;
  const std::vector<uint8_t> P = parity_rows(k, p);
  const uint8_t* lg = rse::Gf8::log_table();
  const uint8_t* ex = rse::Gf8::exp_table();
  Work with, without;
  uint8_t buffer = 0;  // what a shard's pointer points at, where it has one
  std::vector<uint32_t> entries;
  for (uint32_t m = 0; m < T; ++m) {
    entries.push_back(5);  // the block: not the planner's business
    entries.push_back(m);
  }
  std::vector<uint8_t> flags(T), cleared(T);
  std::vector<const uint8_t*> ptr(T);
  for (uint32_t bits = 0; bits < (1u << T); ++bits)
    for (uint32_t null_set = 0; null_set < (1u << T); ++null_set) {
      const bool all = bits == (1u << T) - 1;
      for (int flagless = 0; flagless < (all ? 2 : 1); ++flagless) {
        const uint64_t tag = ((uint64_t)k << 40) | ((uint64_t)bits << 16) | null_set;
        for (uint32_t r = 0; r < T; ++r) {
          flags[r] = (bits >> r) & 1u ? (uint8_t)(1 + r) : 0;  // non-zero = present
          ptr[r] = (null_set >> r) & 1u ? nullptr : &buffer;
          cleared[r] = ptr[r] ? flags[r] : 0;
        }
        ++t.rows;
        t.null_rows += flagless;
        HostEmit got(T, k), want(T, k);
        rse::read_plan_run(lg, ex, P.data(), k, p, flagless ? nullptr : flags.data(), entries.data(),
                           T, with.w, got, 0, 1, rse::ReadNoSync(), rse::ReadNullShards{ptr.data()});
        rse::read_plan_run(lg, ex, P.data(), k, p, cleared.data(), entries.data(), T, without.w,
                           want, 0, 1, rse::ReadNoSync());
        CHECK_EQ("recoverable", tag, 0, with.sc[3] != 0, without.sc[3] != 0);
        uint32_t there = 0;
        for (uint32_t r = 0; r < T; ++r) there += cleared[r] ? 1 : 0;
        CHECK_EQ("recoverable by count", tag, there, with.sc[3] != 0, there >= k);
        if (with.sc[3])
          for (uint32_t i = 0; i < k; ++i) {
            CHECK_EQ("valid set", tag, i, with.valid[i], without.valid[i]);
            if (!ptr[with.valid[i]]) fail("a shard without a buffer in the valid set", tag, i, 0, 1);
          }
        for (uint32_t m = 0; m < T; ++m) {
          CHECK_EQ("class", tag, m, got.cls_of[m], want.cls_of[m]);
          if (!ptr[m] && got.cls_of[m] == rse::kReadCopied)
            fail("a shard without a buffer copied", tag, m, got.cls_of[m], rse::kReadRebuilt);
          t.copied += got.cls_of[m] == rse::kReadCopied;
          t.rebuilt += got.cls_of[m] == rse::kReadRebuilt;
          t.lost += got.cls_of[m] == rse::kReadLost;
          for (uint32_t i = 0; i < k; ++i)
            CHECK_EQ("coefficient", tag, m * 1000 + i, got.coef_of[(size_t)m * k + i],
                     want.coef_of[(size_t)m * k + i]);
        }
      }
    }
}

}  // namespace

int main() {
  VecTotals vec;
  walk_vec(vec);
  CutTotals cut;
  walk_cut(cut);
  PlanTotals plan;
  walk_null_sets(3, 2, plan);
  walk_null_sets(4, 3, plan);
  std::printf("vec %llu of %llu shapes %llu blocks %llu spans %llu empty %llu rows %llu flagless "
              "%llu copied %llu rebuilt %llu lost %llu failures %d\n",
              (unsigned long long)vec.on, (unsigned long long)vec.cases,
              (unsigned long long)cut.shapes, (unsigned long long)cut.blocks,
              (unsigned long long)cut.spans, (unsigned long long)cut.empty_spans,
              (unsigned long long)plan.rows, (unsigned long long)plan.null_rows,
              (unsigned long long)plan.copied, (unsigned long long)plan.rebuilt,
              (unsigned long long)plan.lost, g_fail);
  return g_fail == 0 ? 0 : 1;
}
