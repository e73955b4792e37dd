// Walks rse_correct_plan.hpp (the column decoder of rse_correct_flat with its
// error values and erasures; the code the kernel runs) on the CPU:
//  - 1 / u_r of the device plan and the row H[0] = u_r of several codecs;
//  - seeded byte columns of three small codecs for every pair (nu wrong
//    shards, f erased shards): the codeword, the received column (erased
//    shards hold arbitrary bytes), both position sets and the decoder's result;
//  - columns with errors and erasures at the ends of the point shift and at
//    the limits of the capacity, for 10+4 and 239+16;
//  - a seeded grid inside the capacity for codecs of every parity count 6 .. 16
//    (and 2+3): every (f, nu) with 2 nu + f <= p, checked here against the
//    injection itself -- only a count and the failures are printed.
// tests/test_correct_plan.py compares all of it with a brute-force model.
//
// Lines: "<tag> k p idx ..." with integers only.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rse_correct_plan.hpp"

using rse::Gf8;
using rse::LocatePlan;

static uint64_t g_rng;
static uint32_t rnd() {  // xorshift64*
  g_rng ^= g_rng >> 12;
  g_rng ^= g_rng << 25;
  g_rng ^= g_rng >> 27;
  return (uint32_t)((g_rng * 0x2545F4914F6CDD1Dull) >> 32);
}

static void print_row(const char* tag, const LocatePlan& pl, size_t idx, const uint8_t* v,
                      size_t n) {
  std::printf("%s %u %u %zu", tag, pl.k, pl.p, idx);
  for (size_t i = 0; i < n; ++i) std::printf(" %u", (unsigned)v[i]);
  std::printf("\n");
}

struct Codec {
  LocatePlan pl;
  std::vector<uint8_t> consts;
  explicit Codec(uint32_t k, uint32_t p) : pl(rse::make_locate_plan(k, p)) {
    consts.resize(rse::kCorConstsBytes);
    rse::correct_consts(pl, consts.data());
  }
};

// A random codeword of the codec
static std::vector<uint8_t> codeword(const LocatePlan& pl) {
  const uint32_t k = pl.k, p = pl.p;
  std::vector<uint8_t> col(pl.n, 0);
  for (uint32_t i = 0; i < k; ++i) col[i] = (uint8_t)rnd();
  for (uint32_t r = 0; r < p; ++r)
    for (uint32_t i = 0; i < k; ++i) col[k + r] ^= Gf8::mul(pl.P[(size_t)r * k + i], col[i]);
  return col;
}

// The received column `col` with the shards `era` erased, decoded in place as
// the kernel does: a stripe with more than p erasures is skipped, a column
// with d = P data ^ parity = 0 is left alone, any other goes through S = T d
// and the column decoder.  Returns the decoder's m (0 for a column left alone),
// kLocateBad for an undecodable column.
static uint32_t decode(const Codec& c, std::vector<uint8_t>& col,
                       const std::vector<uint32_t>& era) {
  const LocatePlan& pl = c.pl;
  const uint32_t k = pl.k, p = pl.p, n = pl.n;
  const uint8_t* lg = c.consts.data() + rse::kLocLogOff;
  const uint8_t* ex = c.consts.data() + rse::kLocExpOff;
  uint8_t epos[16] = {0};
  uint32_t emask[8] = {0}, gamma[rse::kCorGammaWords] = {1u, 0u, 0u, 0u, 0u};
  const uint32_t f = (uint32_t)era.size();
  for (uint32_t i = 0; i < f; ++i) {
    if (i < 16) epos[i] = (uint8_t)era[i];
    emask[era[i] >> 5] |= 1u << (era[i] & 31u);
  }
  if (f <= p) rse::correct_gamma(lg, ex, epos, f, gamma);
  const rse::CorrectErasures er{f, epos, gamma, emask};

  uint32_t d[4] = {0, 0, 0, 0}, S[4], pos[4], val[4];
  bool any = false;
  for (uint32_t r = 0; r < p; ++r) {
    uint8_t v = col[k + r];
    for (uint32_t i = 0; i < k; ++i) v ^= Gf8::mul(pl.P[(size_t)r * k + i], col[i]);
    rse::pk_set(d, r, v);
    any = any || v != 0;
  }
  uint32_t m = 0;
  if (f > p) {
    m = rse::kLocateBad;
  } else if (any) {
    rse::locate_syndromes(lg, ex, c.consts.data() + rse::kLocTOff, d, p, S);
    m = rse::correct_column(lg, ex, c.consts.data() + rse::kCorInvUOff, S, p, n, er, pos, val);
  }
  if (m != rse::kLocateBad)
    for (uint32_t i = 0; i < m; ++i) col[rse::pk_get(pos, i)] ^= (uint8_t)rse::pk_get(val, i);
  return m;
}

// A random codeword with the shards `era` erased (arbitrary bytes in their
// place) and the shards `err` made wrong, decoded and printed.
static void column(const Codec& c, size_t idx, const std::vector<uint32_t>& era,
                   const std::vector<uint32_t>& err) {
  const LocatePlan& pl = c.pl;
  const uint32_t n = pl.n;
  std::vector<uint8_t> col = codeword(pl);
  print_row("cw", pl, idx, col.data(), n);
  for (uint32_t q : era) col[q] = (uint8_t)rnd();
  for (uint32_t q : err) col[q] ^= (uint8_t)(1u + rnd() % 255u);
  print_row("rx", pl, idx, col.data(), n);
  std::vector<uint8_t> e8(era.begin(), era.end()), i8(err.begin(), err.end());
  print_row("era", pl, idx, e8.data(), e8.size());
  print_row("inj", pl, idx, i8.data(), i8.size());
  const uint32_t m = decode(c, col, era);
  std::vector<uint8_t> res;
  res.push_back((uint8_t)m);  // 255: undecodable
  if (m != rse::kLocateBad) res.insert(res.end(), col.begin(), col.end());
  print_row("res", pl, idx, res.data(), res.size());
}

// `count` distinct shard indices
static std::vector<uint32_t> pick(uint32_t n, uint32_t count) {
  std::vector<uint32_t> all(n);
  for (uint32_t i = 0; i < n; ++i) all[i] = i;
  for (uint32_t i = 0; i < count; ++i) std::swap(all[i], all[i + rnd() % (n - i)]);
  all.resize(count);
  return all;
}

static std::vector<uint32_t> range(uint32_t a, uint32_t b) {
  std::vector<uint32_t> v;
  for (uint32_t i = a; i < b; ++i) v.push_back(i);
  return v;
}

// The limits of the capacity with both ends of the point shift involved:
// erasures are taken from shard 1 up (and the last shard), errors sit on
// shard 0 and, where there are more, on the shards before the last.
static void edges(uint32_t k, uint32_t p, uint64_t seed) {
  const Codec c(k, p);
  const uint32_t n = k + p, t = p / 2;
  g_rng = seed;
  column(c, 100000, {}, {0});
  column(c, 100001, {}, {n - 1});
  column(c, 100002, {}, {0, n - 1});
  {  // t errors, both ends among them
    std::vector<uint32_t> err = range(n - t, n);
    err[0] = 0;
    column(c, 100003, {}, err);
  }
  column(c, 100004, range(n - p, n), {});             // p erasures, no error
  column(c, 100005, range(0, p), {});                 // the same at the other end
  column(c, 100006, range(1, p - 1), {0});            // p - 2 erasures + 1 error
  column(c, 100007, range(n - p + 2, n), {n - p});    // the same at the other end
  column(c, 100008, range(1, p), {0});                // p - 1 erasures + 1 error: past capacity
  column(c, 100009, range(n - p - 1, n), {});         // p + 1 erasures
  column(c, 100010, {0, n - 1}, range(1, 1 + (p - 2) / 2));  // 2 erasures + (p - 2) / 2 errors
  column(c, 100011, {}, {});
}

// Inside the capacity the decoded column is the codeword it was made from:
// kGridCols seeded columns for every (f, nu) with 2 nu + f <= p.  Prints
// "gridfail k p idx f nu" per column that is not, then "grid k p 0 columns
// failures".
constexpr int kGridCols = 40;
static void grid(uint32_t k, uint32_t p, uint64_t seed) {
  const Codec c(k, p);
  const uint32_t n = c.pl.n;
  g_rng = seed * 0x9E3779B97F4A7C15ull + k * 131u + p;
  size_t idx = 0, fails = 0;
  for (uint32_t f = 0; f <= p; ++f)
    for (uint32_t nu = 0; 2 * nu + f <= p; ++nu)
      for (int q = 0; q < kGridCols; ++q, ++idx) {
        const std::vector<uint32_t> all = pick(n, nu + f);
        const std::vector<uint32_t> era(all.begin(), all.begin() + f);
        const std::vector<uint8_t> cw = codeword(c.pl);
        std::vector<uint8_t> col = cw;
        for (uint32_t s : era) col[s] = (uint8_t)rnd();
        for (uint32_t i = f; i < nu + f; ++i) col[all[i]] ^= (uint8_t)(1u + rnd() % 255u);
        const uint32_t m = decode(c, col, era);
        if (m == rse::kLocateBad || m > p || col != cw) {
          const uint8_t fn[2] = {(uint8_t)f, (uint8_t)nu};
          print_row("gridfail", c.pl, idx, fn, 2);
          ++fails;
        }
      }
  std::printf("grid %u %u 0 %zu %zu\n", k, p, idx, fails);
}

int main(int argc, char** argv) {
  // The default seed was chosen on the CPU so that the columns past capacity
  // hold both outcomes for every codec (tests/test_correct_plan.py).
  const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 0) : 1;
  const uint32_t plans[][2] = {{10, 4}, {3, 2},  {4, 5},   {17, 3},  {1, 1},    {100, 16},
                               {239, 16}, {20, 8}, {6, 9},   {30, 15},  {12, 12},  {5, 6},
                               {7, 7},    {40, 10}, {200, 11}, {50, 13}, {60, 14}, {1, 16},
                               {128, 16}, {129, 16}, {2, 3}};
  for (auto& kp : plans) {
    const Codec c(kp[0], kp[1]);
    print_row("iu", c.pl, 0, c.consts.data() + rse::kCorInvUOff, c.pl.n);
    print_row("u", c.pl, 0, c.pl.H.data(), c.pl.n);  // H[0][r] = u_r
    // the locate layout is the prefix of the plan
    std::vector<uint8_t> loc(rse::locate_consts_bytes(c.pl));
    rse::locate_consts(c.pl, loc.data());
    for (size_t i = 0; i < loc.size(); ++i)
      if (loc[i] != c.consts[i]) return 1;
  }

  // seeded columns: 40 for each (nu, f)
  const uint32_t small[][2] = {{3, 2}, {6, 4}, {4, 5}};
  for (auto& kp : small) {
    const Codec c(kp[0], kp[1]);
    const uint32_t p = c.pl.p, n = c.pl.n;
    g_rng = seed * 0x9E3779B97F4A7C15ull + kp[0] * 131u + kp[1];
    size_t idx = 0;
    for (uint32_t nu = 0; nu <= p; ++nu)
      for (uint32_t f = 0; f <= p + 1 && nu + f <= n; ++f)
        for (int q = 0; q < 40; ++q) {
          const std::vector<uint32_t> all = pick(n, nu + f);
          column(c, idx++, std::vector<uint32_t>(all.begin(), all.begin() + f),
                 std::vector<uint32_t>(all.begin() + f, all.end()));
        }
  }

  edges(10, 4, seed + 1);
  edges(239, 16, seed + 2);

  // every parity count 6 .. 16, single-chunk and multi-chunk k, k = 1
  const uint32_t wide[][2] = {{20, 8},  {6, 9},   {30, 15}, {12, 12},  {5, 6},    {7, 7},
                              {40, 10}, {200, 11}, {50, 13}, {60, 14},  {1, 16},   {128, 16},
                              {129, 16}, {100, 16}, {239, 16}, {2, 3}};
  for (auto& kp : wide) grid(kp[0], kp[1], seed);
  return 0;
}
