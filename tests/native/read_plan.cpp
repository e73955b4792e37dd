// The plan of rse_read_flat (rse_read_plan.hpp) walked on the CPU.
//  * Every list of 1..4 entries over stripe values 0..3 and shard values 0..5
//    with n_stripes = 3, k + p = 5 (so out-of-range values occur): the in-order
//    verdict and the first offender against a brute-force restatement (a
//    prefix is good iff every entry is in range and every PAIR of entries is
//    strictly ascending as (stripe, shard)); for accepted lists the run heads
//    (no earlier entry names the stripe) and the run count (distinct stripes).
//  * The run planner, read_plan_run, for EVERY flag row of 3+2, 4+3, 5+4 and
//    2+6, every shard wanted in one run and each shard wanted alone, and for
//    200 seeded flag rows each of 100+28 and 128+128 (row n has n mod (p + 2)
//    shards erased, so stripes past repair occur), every shard wanted.  The
//    brute force is Matrix<Gf8Field> (rse_field.hpp): the codec's matrix M =
//    V (V[0..k])^-1, and for a flag row M[r] (M[first k present])^-1 -- a unit
//    row for a present shard of the valid set, lost where fewer than k are
//    present.  Classes and coefficient rows must be equal.
//  * The output groups tile 1..256 entries, none larger than 16.
//  * Spans and lanes (the update plan's, which the read kernel uses) tile
//    [0, bytes) for the multiples of 16 up to 70,000 and both neighbours of
//    each; the 16-byte path is on exactly when both bases and the shard's bytes
//    are multiples of 16; the workgroup count: RSE_OPT_GRID_X outright, else
//    what the device holds, capped by the items there can be.
// Prints one line per failure and a summary line; exit status 1 on a failure.
// Built and run by tests/test_read_plan.py, also under ASan + UBSan.
#include <cstdint>
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "rse_field.hpp"
#include "rse_read_plan.hpp"

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

constexpr uint32_t kStripes = 3, kTotal = 5, kStripeValues = 4, kShardValues = 6;

// the brute-force restatement: is the prefix [0, n) of the list good?
bool prefix_good(const std::vector<uint32_t>& rd, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    if (rd[2 * i] >= kStripes || rd[2 * i + 1] >= kTotal) return false;
    for (size_t j = i + 1; j < n; ++j) {
      const std::pair<uint32_t, uint32_t> a{rd[2 * i], rd[2 * i + 1]}, b{rd[2 * j], rd[2 * j + 1]};
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
    for (size_t i = 0; i < n; ++i) combos *= kStripeValues * kShardValues;
    std::vector<uint32_t> rd(2 * n);
    for (uint64_t code = 0; code < combos; ++code) {
      uint64_t c = code;
      for (size_t i = 0; i < n; ++i) {
        rd[2 * i] = (uint32_t)(c % kStripeValues);
        c /= kStripeValues;
        rd[2 * i + 1] = (uint32_t)(c % kShardValues);
        c /= kShardValues;
      }
      ++t.lists;
      uint64_t got = n;
      for (size_t u = 0; u < n; ++u)
        if (!rse::read_in_order(rd.data(), u, kStripes, kTotal)) {
          got = u;
          break;
        }
      uint64_t want = n;
      for (size_t u = 0; u < n; ++u)
        if (!prefix_good(rd, u + 1)) {
          want = u;
          break;
        }
      CHECK_EQ("first offender", code, n, got, want);
      if (want != n) continue;
      ++t.accepted;
      std::set<uint32_t> seen;
      uint64_t heads = 0;
      for (size_t u = 0; u < n; ++u) {
        const bool head = seen.insert(rd[2 * u]).second;  // no earlier entry names the stripe
        CHECK_EQ("run head", code, u, rse::update_run_head(rd.data(), u), head);
        heads += rse::update_run_head(rd.data(), u) ? 1 : 0;
      }
      CHECK_EQ("run count", code, n, heads, seen.size());
      t.runs += heads;
    }
  }
}

// ---- the run planner

using Mat = rse::Matrix<rse::Gf8Field>;

struct Codec {
  uint32_t k, p;
  Mat m;                   // (k + p) x k, systematic
  std::vector<uint8_t> P;  // its parity rows as bytes
  Codec(uint32_t k_, uint32_t p_) : k(k_), p(p_) {
    const Mat v = Mat::vandermonde(k + p, k);
    Mat top(k, k), inv;
    for (uint32_t r = 0; r < k; ++r)
      for (uint32_t c = 0; c < k; ++c) top.at(r, c) = v.at(r, c);
    if (!top.invert(inv)) fail("codec matrix", k, p, 0, 1);
    m = v.multiply(inv);
    for (uint32_t r = 0; r < k; ++r)
      for (uint32_t c = 0; c < k; ++c) CHECK_EQ("systematic", r, c, m.at(r, c), r == c ? 1 : 0);
    P.resize((size_t)p * k);
    for (uint32_t r = 0; r < p; ++r)
      for (uint32_t c = 0; c < k; ++c) P[(size_t)r * k + c] = (uint8_t)m.at(k + r, c);
  }
};

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
  uint64_t rows = 0, copied = 0, rebuilt = 0, lost = 0;
};

// one flag row: the brute force, then the plan for `wanted` in one run
void check_row(const Codec& c, const std::vector<uint8_t>& flags, bool each_alone, Work& work,
               PlanTotals& t, uint64_t tag) {
  const uint32_t k = c.k, T = c.k + c.p;
  ++t.rows;
  std::vector<uint32_t> valid;
  for (uint32_t r = 0; r < T && valid.size() < k; ++r)
    if (flags[r]) valid.push_back(r);
  const bool recoverable = valid.size() == k;
  Mat rows_of;  // T x k: M (M[valid])^-1
  if (recoverable) {
    Mat sub(k, k), inv;
    for (uint32_t i = 0; i < k; ++i)
      for (uint32_t col = 0; col < k; ++col) sub.at(i, col) = c.m.at(valid[i], col);
    if (!sub.invert(inv)) fail("singular valid set", tag, 0, 0, 1);
    rows_of = c.m.multiply(inv);
    for (uint32_t i = 0; i < k; ++i)  // a present shard of the valid set: a unit row
      for (uint32_t col = 0; col < k; ++col)
        CHECK_EQ("unit row", tag, valid[i], rows_of.at(valid[i], col), i == col ? 1 : 0);
  }
  auto check = [&](const std::vector<uint32_t>& wanted, bool count) {
    std::vector<uint32_t> entries;
    for (uint32_t m : wanted) {
      entries.push_back(7);  // the stripe: not the planner's business
      entries.push_back(m);
    }
    HostEmit emit((uint32_t)wanted.size(), k);
    // all flags set is also what "no flags" means: take that route every other time
    bool all = true;
    for (uint32_t r = 0; r < T; ++r) all = all && flags[r];
    rse::read_plan_run(rse::Gf8::log_table(), rse::Gf8::exp_table(), c.P.data(), k, c.p,
                       all && (tag & 1) ? nullptr : flags.data(), entries.data(),
                       (uint32_t)wanted.size(), work.w, emit, 0, 1, rse::ReadNoSync());
    CHECK_EQ("recoverable", tag, 0, work.sc[3] != 0, recoverable);
    if (recoverable)
      for (uint32_t i = 0; i < k; ++i) CHECK_EQ("valid set", tag, i, work.valid[i], valid[i]);
    for (size_t j = 0; j < wanted.size(); ++j) {
      const uint32_t m = wanted[j];
      const int want = flags[m] ? rse::kReadCopied : recoverable ? rse::kReadRebuilt : rse::kReadLost;
      CHECK_EQ("class", tag, m, emit.cls_of[j], want);
      if (count) {
        t.copied += want == rse::kReadCopied;
        t.rebuilt += want == rse::kReadRebuilt;
        t.lost += want == rse::kReadLost;
      }
      for (uint32_t i = 0; i < k; ++i) {
        const int got = emit.coef_of[j * k + i];
        if (want == rse::kReadRebuilt)
          CHECK_EQ("coefficient", tag, m * 1000 + i, got, rows_of.at(m, i));
        else
          CHECK_EQ("coefficient of a row that is not rebuilt", tag, m * 1000 + i, got, -1);
      }
    }
  };
  std::vector<uint32_t> every(T);
  for (uint32_t r = 0; r < T; ++r) every[r] = r;
  check(every, true);
  if (each_alone)
    for (uint32_t r = 0; r < T; ++r) check({r}, false);
}

void walk_small(uint32_t k, uint32_t p, Work& work, PlanTotals& t) {
  const Codec c(k, p);
  const uint32_t T = k + p;
  std::vector<uint8_t> flags(T);
  for (uint32_t bits = 0; bits < (1u << T); ++bits) {
    for (uint32_t r = 0; r < T; ++r) flags[r] = (bits >> r) & 1u ? (uint8_t)(1 + r) : 0;  // non-zero
    check_row(c, flags, true, work, t, ((uint64_t)k << 40) | bits);
  }
}

void walk_seeded(uint32_t k, uint32_t p, Work& work, PlanTotals& t) {
  const Codec c(k, p);
  const uint32_t T = k + p;
  uint64_t x = 0x9E3779B97F4A7C15ull * (k + 1) + p;
  std::vector<uint8_t> flags(T);
  std::vector<uint32_t> order(T);
  for (uint32_t n = 0; n < 200; ++n) {
    const uint32_t erased = n % (p + 2);
    for (uint32_t r = 0; r < T; ++r) order[r] = r;
    for (uint32_t r = 0; r < T; ++r) flags[r] = 1;
    for (uint32_t i = 0; i < erased; ++i) {  // a partial shuffle: `erased` distinct shards
      x = x * 6364136223846793005ull + 1442695040888963407ull;
      const uint32_t j = i + (uint32_t)((x >> 33) % (T - i));
      std::swap(order[i], order[j]);
      flags[order[i]] = 0;
    }
    check_row(c, flags, false, work, t, ((uint64_t)k << 40) | n);
  }
}

uint64_t walk_groups() {
  uint64_t groups = 0;
  for (uint32_t entries = 1; entries <= 256; ++entries) {
    const uint32_t n = rse::read_groups(entries);
    uint32_t next = 0;
    for (uint32_t g = 0; g < n; ++g) {
      CHECK_EQ("group first", entries, g, rse::read_group_first(g), next);
      const uint32_t rows = rse::read_group_entries(entries, g);
      if (rows == 0 || rows > rse::kReadRows) fail("group entries", entries, g, rows, 16);
      if (g + 1 < n) CHECK_EQ("full group", entries, g, rows, rse::kReadRows);
      next += rows;
    }
    CHECK_EQ("groups tile", entries, n, next, entries);
    groups += n;
  }
  CHECK_EQ("longest run", 3, 14, rse::read_max_run(3, 14), 3);
  CHECK_EQ("longest run", 512, 14, rse::read_max_run(512, 14), 14);
  CHECK_EQ("longest run", 0xffffffffull, 256, rse::read_max_run(0xffffffffull, 256), 256);
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
        const bool got = rse::read_vec(reinterpret_cast<const void*>(pa),
                                       reinterpret_cast<const void*>(pb), bytes);
        const bool want = pa % 16 == 0 && pb % 16 == 0 && bytes % 16 == 0;
        CHECK_EQ("vec", bytes, off, got, want);
        ++*cases;
        on += got ? 1 : 0;
      }
  return on;
}

void walk_grid() {
  for (int64_t opt : {int64_t(1), int64_t(3), int64_t(4096)})
    CHECK_EQ("grid option", opt, 0, rse::read_grid(256, opt, 1000, 1 << 20), opt);
  CHECK_EQ("grid fill", 256, 0, rse::read_grid(256, 0, 1000, 1 << 20), 256 * rse::kUpdPerCu);
  CHECK_EQ("grid items", 256, 1, rse::read_grid(256, 0, 3, 48), 3);
  CHECK_EQ("grid items", 256, 2, rse::read_grid(256, 0, 3, 4097), 6);
  CHECK_EQ("grid one", 0, 3, rse::read_grid(0, 0, 1, 1), 1);
  CHECK_EQ("grid saturates", 256, 4, rse::read_grid(256, 0, 0xffffffffull, uint64_t(1) << 62),
           256 * rse::kUpdPerCu);
}

void walk_scope() {
  CHECK_EQ("scope", 8, 0, rse::read_in_scope(8, 10, 4), 1);
  CHECK_EQ("scope", 8, 1, rse::read_in_scope(8, 128, 128), 1);
  CHECK_EQ("scope", 8, 2, rse::read_in_scope(8, 4, 200), 0);
  CHECK_EQ("scope", 8, 3, rse::read_in_scope(8, 127, 129), 0);
  CHECK_EQ("scope", 16, 0, rse::read_in_scope(16, 100, 28), 1);
  CHECK_EQ("scope", 16, 1, rse::read_in_scope(16, 300, 20), 0);
  CHECK_EQ("scope", 16, 2, rse::read_in_scope(16, 250, 7), 0);
  CHECK_EQ("scope", 4, 0, rse::read_in_scope(4, 10, 4), 0);
}

}  // namespace

int main() {
  ListTotals t;
  walk_lists(t);
  Work work;
  PlanTotals small, seeded;
  walk_small(3, 2, work, small);
  walk_small(4, 3, work, small);
  walk_small(5, 4, work, small);
  walk_small(2, 6, work, small);
  walk_seeded(100, 28, work, seeded);
  walk_seeded(128, 128, work, seeded);
  const uint64_t groups = walk_groups();
  uint64_t lengths = 0, vec_cases = 0;
  const uint64_t spans = walk_spans(&lengths);
  const uint64_t vec_on = walk_vec(&vec_cases);
  walk_grid();
  walk_scope();
  std::printf("lists %llu accepted %llu runs %llu rows %llu copied %llu rebuilt %llu lost %llu "
              "seeded %llu copied %llu rebuilt %llu lost %llu groups %llu lengths %llu spans %llu "
              "vec %llu of %llu failures %d\n",
              (unsigned long long)t.lists, (unsigned long long)t.accepted,
              (unsigned long long)t.runs, (unsigned long long)small.rows,
              (unsigned long long)small.copied, (unsigned long long)small.rebuilt,
              (unsigned long long)small.lost, (unsigned long long)seeded.rows,
              (unsigned long long)seeded.copied, (unsigned long long)seeded.rebuilt,
              (unsigned long long)seeded.lost, (unsigned long long)groups,
              (unsigned long long)lengths, (unsigned long long)spans, (unsigned long long)vec_on,
              (unsigned long long)vec_cases, g_fail);
  return g_fail == 0 ? 0 : 1;
}
