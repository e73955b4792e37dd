// The plan of rse_update_flat (rse_update_plan.hpp) walked on the CPU.
//  * Every list of 1..4 entries over stripe values 0..3 and shard values 0..3
//    with n_stripes = 3, k = 3 (so out-of-range values occur): the in-order
//    verdict and the first offender against a brute-force restatement (a
//    prefix is good iff every entry is in range and every PAIR of entries is
//    strictly ascending as (stripe, shard)); for accepted lists the run heads
//    (no earlier entry names the stripe) and the run count (distinct stripes).
//  * The row groups tile 0..p for p = 1..255, none larger than 16.
//  * The spans tile [0, bytes) for the multiples of 16 up to 70,000 and both
//    neighbours of each (which covers both neighbours of every span boundary),
//    and the lanes tile every span.
//  * The 16-byte path is on exactly when both bases and the shard's bytes are
//    multiples of 16, on base pairs with one base off by 1, by 8 and by 16.
//  * The workgroup count: RSE_OPT_GRID_X outright, else what the device holds,
//    capped by the items there can be.
// Prints one line per failure and a summary line; exit status 1 on a failure.
// Built and run by tests/test_update_plan.py, also under ASan + UBSan.
#include <cstdint>
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

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

constexpr uint32_t kStripes = 3, kData = 3, kValues = 4;

// the brute-force restatement: is the prefix [0, n) of the list good?
bool prefix_good(const std::vector<uint32_t>& upd, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    if (upd[2 * i] >= kStripes || upd[2 * i + 1] >= kData) return false;
    for (size_t j = i + 1; j < n; ++j) {
      const std::pair<uint32_t, uint32_t> a{upd[2 * i], upd[2 * i + 1]}, b{upd[2 * j], upd[2 * j + 1]};
      if (!(a < b)) return false;
    }
  }
  return true;
}

struct ListTotals {
  uint64_t lists = 0, accepted = 0, runs = 0;
};

void walk_lists(ListTotals& t) {
  for (size_t n = 1; n <= 4; ++n) {
    uint64_t combos = 1;
    for (size_t i = 0; i < 2 * n; ++i) combos *= kValues;
    std::vector<uint32_t> upd(2 * n);
    for (uint64_t code = 0; code < combos; ++code) {
      uint64_t c = code;
      for (size_t i = 0; i < 2 * n; ++i, c /= kValues) upd[i] = (uint32_t)(c % kValues);
      ++t.lists;
      // the header's verdict: the lowest entry that is not in order
      uint64_t got = n;
      for (size_t u = 0; u < n; ++u)
        if (!rse::update_in_order(upd.data(), u, kStripes, kData)) {
          got = u;
          break;
        }
      uint64_t want = n;
      for (size_t u = 0; u < n; ++u)
        if (!prefix_good(upd, u + 1)) {
          want = u;
          break;
        }
      CHECK_EQ("first offender", code, n, got, want);
      if (want != n) continue;
      ++t.accepted;
      std::set<uint32_t> seen;
      uint64_t heads = 0;
      for (size_t u = 0; u < n; ++u) {
        const bool head = seen.insert(upd[2 * u]).second;  // no earlier entry names the stripe
        CHECK_EQ("run head", code, u, rse::update_run_head(upd.data(), u), head);
        heads += rse::update_run_head(upd.data(), u) ? 1 : 0;
      }
      CHECK_EQ("run count", code, n, heads, seen.size());
      t.runs += heads;
    }
  }
}

uint64_t walk_groups() {
  uint64_t groups = 0;
  for (uint32_t p = 1; p <= 255; ++p) {
    const uint32_t n = rse::update_row_groups(p);
    uint32_t next = 0;
    for (uint32_t g = 0; g < n; ++g) {
      CHECK_EQ("group first", p, g, rse::update_group_first(g), next);
      const uint32_t rows = rse::update_group_rows(p, g);
      if (rows == 0 || rows > 16) fail("group rows", p, g, rows, 16);
      next += rows;
    }
    CHECK_EQ("groups tile", p, n, next, p);
    groups += n;
  }
  return groups;
}

uint64_t walk_spans(uint64_t* lengths) {
  uint64_t spans = 0;
  for (uint64_t bytes = 1; bytes <= 70000; ++bytes) {
    if (!(bytes % 16 == 0 || bytes % 16 == 1 || bytes % 16 == 15)) continue;
    ++*lengths;
    const uint64_t n = rse::update_spans(bytes);
    uint64_t next = 0;
    for (uint64_t s = 0; s < n; ++s) {
      CHECK_EQ("span first", bytes, s, rse::update_span_first(s), next);
      const uint64_t len = rse::update_span_len(bytes, s);
      if (s + 1 < n) CHECK_EQ("full span", bytes, s, len, rse::kUpdSpanBytes);
      if (len == 0 || len > rse::kUpdSpanBytes) fail("span length", bytes, s, len, rse::kUpdSpanBytes);
      // the lanes tile the span, 16 bytes each, only the last one short, none after it
      uint64_t lane_next = 0;
      for (uint32_t t = 0; t < rse::kUpdBlock; ++t) {
        const uint32_t ln = rse::update_lane_len(len, t);
        if (ln > 16) fail("lane length", bytes, t, ln, 16);
        if (ln != 0) CHECK_EQ("lane first", bytes, t, (uint64_t)t * 16, lane_next);
        if (ln == 0 && lane_next != len) fail("lane gap", bytes, t, lane_next, len);
        lane_next += ln;
      }
      CHECK_EQ("lanes tile", bytes, s, lane_next, len);
      next += len;
    }
    CHECK_EQ("spans tile", bytes, n, next, bytes);
    spans += n;
  }
  return spans;
}

uint64_t walk_vec(uint64_t* cases) {
  uint64_t on = 0;
  const uintptr_t a = 0x10000, b = 0x80000;
  for (uint64_t bytes : {1u, 8u, 15u, 16u, 17u, 32u, 48u, 1024u, 4096u + 37u, 16384u + 48u})
    for (int which = -1; which < 2; ++which)
      for (uintptr_t off : {uintptr_t(1), uintptr_t(8), uintptr_t(16)}) {
        if (which < 0 && off != 1) continue;  // both bases aligned: once
        const uintptr_t pa = a + (which == 0 ? off : 0), pb = b + (which == 1 ? off : 0);
        const bool got = rse::update_vec(reinterpret_cast<const void*>(pa),
                                         reinterpret_cast<const void*>(pb), bytes);
        const bool want = pa % 16 == 0 && pb % 16 == 0 && bytes % 16 == 0;
        CHECK_EQ("vec", bytes, off, got, want);
        ++*cases;
        on += got ? 1 : 0;
      }
  return on;
}

void walk_grid() {
  // the option sets the count outright
  for (int64_t opt : {int64_t(1), int64_t(3), int64_t(4096)})
    CHECK_EQ("grid option", opt, 0, rse::update_grid(256, opt, 1000, 1 << 20), opt);
  // else what the device holds at once, and no more than the items
  CHECK_EQ("grid fill", 256, 0, rse::update_grid(256, 0, 1000, 1 << 20), 256 * rse::kUpdPerCu);
  CHECK_EQ("grid items", 256, 1, rse::update_grid(256, 0, 3, 48), 3);
  CHECK_EQ("grid items", 256, 2, rse::update_grid(256, 0, 3, 4097), 6);
  CHECK_EQ("grid one", 0, 3, rse::update_grid(0, 0, 1, 1), 1);
  CHECK_EQ("grid saturates", 256, 4,
           rse::update_grid(256, 0, 0xffffffffull, uint64_t(1) << 62), 256 * rse::kUpdPerCu);
}

}  // namespace

int main() {
  ListTotals t;
  walk_lists(t);
  const uint64_t groups = walk_groups();
  uint64_t lengths = 0, vec_cases = 0;
  const uint64_t spans = walk_spans(&lengths);
  const uint64_t vec_on = walk_vec(&vec_cases);
  walk_grid();
  std::printf("lists %llu accepted %llu runs %llu groups %llu lengths %llu spans %llu vec %llu of "
              "%llu failures %d\n",
              (unsigned long long)t.lists, (unsigned long long)t.accepted,
              (unsigned long long)t.runs, (unsigned long long)groups, (unsigned long long)lengths,
              (unsigned long long)spans, (unsigned long long)vec_on,
              (unsigned long long)vec_cases, g_fail);
  return g_fail == 0 ? 0 : 1;
}
