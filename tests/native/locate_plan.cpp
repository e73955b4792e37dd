// Walks rse_locate_plan.hpp (the host plan and the column decoder of
// rse_locate_flat; the decoder is the code the kernel runs) on the CPU:
//  - the plan matrices P, T and H of several codecs;
//  - seeded byte columns with 0 .. p wrong shards for three small codecs: the
//    received column, the injected positions and the decoder's verdict;
//  - columns with errors at the ends of the point shift (shard 0, shard n-1,
//    and shard 254 of 239+16);
//  - a seeded grid of 0 .. t wrong shards for codecs of every parity count
//    6 .. 16, checked here against the injection itself -- only a count and the
//    failures are printed.
// tests/test_locate_plan.py compares all of it with the oracle's matrices and
// a brute-force statement of what "decodable" means.
//
// Lines: "<tag> k p ..." with integers only.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rse_locate_plan.hpp"

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

static void print_plan(const LocatePlan& pl) {
  for (uint32_t r = 0; r < pl.p; ++r) print_row("P", pl, r, &pl.P[(size_t)r * pl.k], pl.k);
  for (uint32_t j = 0; j < pl.p; ++j) print_row("T", pl, j, &pl.T[(size_t)j * 16], pl.p);
  for (uint32_t j = 0; j < pl.p; ++j) print_row("H", pl, j, &pl.H[(size_t)j * pl.n], pl.n);
}

// A random codeword with the shards `pos` made wrong, decoded as the kernel
// does: d = P data ^ parity, S = T d, then the column decoder.
static void column(const LocatePlan& pl, const uint8_t* consts, size_t idx,
                   const std::vector<uint32_t>& pos) {
  const uint32_t k = pl.k, p = pl.p, n = pl.n;
  std::vector<uint8_t> col(n, 0);
  for (uint32_t i = 0; i < k; ++i) col[i] = (uint8_t)rnd();
  for (uint32_t r = 0; r < p; ++r)
    for (uint32_t i = 0; i < k; ++i) col[k + r] ^= Gf8::mul(pl.P[(size_t)r * k + i], col[i]);
  for (uint32_t q : pos) col[q] ^= (uint8_t)(1u + rnd() % 255u);
  print_row("rx", pl, idx, col.data(), n);
  std::vector<uint8_t> inj(pos.begin(), pos.end());
  print_row("inj", pl, idx, inj.data(), inj.size());

  uint32_t d[4] = {0, 0, 0, 0}, S[4], roots[2];
  for (uint32_t r = 0; r < p; ++r) {
    uint8_t v = col[k + r];
    for (uint32_t i = 0; i < k; ++i) v ^= Gf8::mul(pl.P[(size_t)r * k + i], col[i]);
    rse::pk_set(d, r, v);
  }
  const uint8_t* lg = consts + rse::kLocLogOff;
  const uint8_t* ex = consts + rse::kLocExpOff;
  rse::locate_syndromes(lg, ex, consts + rse::kLocTOff, d, p, S);
  const uint32_t L = rse::locate_column(lg, ex, S, p, n, roots);
  std::vector<uint8_t> res;
  res.push_back((uint8_t)L);  // 255: undecodable
  for (uint32_t i = 0; L != rse::kLocateBad && i < L; ++i)
    res.push_back((uint8_t)rse::pk_get(roots, i));
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

// With at most t wrong shards the decoder names exactly those, ascending:
// kGridCols seeded columns for every count 0 .. t.  Prints "gridfail k p idx
// nu" per column where it does not, then "grid k p 0 columns failures".
constexpr int kGridCols = 40;
static void grid(uint32_t k, uint32_t p, uint64_t seed) {
  const LocatePlan pl = rse::make_locate_plan(k, p);
  std::vector<uint8_t> consts(rse::locate_consts_bytes(pl));
  rse::locate_consts(pl, consts.data());
  const uint8_t* lg = consts.data() + rse::kLocLogOff;
  const uint8_t* ex = consts.data() + rse::kLocExpOff;
  g_rng = seed * 0x9E3779B97F4A7C15ull + k * 131u + p;
  size_t idx = 0, fails = 0;
  for (uint32_t nu = 0; nu <= pl.t; ++nu)
    for (int q = 0; q < kGridCols; ++q, ++idx) {
      std::vector<uint32_t> pos = pick(pl.n, nu);
      std::vector<uint8_t> col(pl.n, 0);
      for (uint32_t i = 0; i < k; ++i) col[i] = (uint8_t)rnd();
      for (uint32_t r = 0; r < p; ++r)
        for (uint32_t i = 0; i < k; ++i) col[k + r] ^= Gf8::mul(pl.P[(size_t)r * k + i], col[i]);
      for (uint32_t s : pos) col[s] ^= (uint8_t)(1u + rnd() % 255u);
      uint32_t d[4] = {0, 0, 0, 0}, S[4], roots[2];
      for (uint32_t r = 0; r < p; ++r) {
        uint8_t v = col[k + r];
        for (uint32_t i = 0; i < k; ++i) v ^= Gf8::mul(pl.P[(size_t)r * k + i], col[i]);
        rse::pk_set(d, r, v);
      }
      rse::locate_syndromes(lg, ex, consts.data() + rse::kLocTOff, d, p, S);
      const uint32_t L = rse::locate_column(lg, ex, S, p, pl.n, roots);
      std::sort(pos.begin(), pos.end());
      bool ok = L == nu;
      for (uint32_t i = 0; ok && i < nu; ++i) ok = rse::pk_get(roots, i) == pos[i];
      if (!ok) {
        const uint8_t b = (uint8_t)nu;
        print_row("gridfail", pl, idx, &b, 1);
        ++fails;
      }
    }
  std::printf("grid %u %u 0 %zu %zu\n", k, p, idx, fails);
}

int main(int argc, char** argv) {
  // The default seed was chosen on the CPU so that the columns with more than
  // t wrong shards hold both outcomes (tests/test_locate_plan.py).
  const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 0) : 4;
  const uint32_t plans[][2] = {{10, 4}, {3, 2},  {4, 5},   {17, 3},  {1, 1},    {100, 16},
                               {239, 16}, {20, 8}, {6, 9},   {30, 15},  {12, 12},  {5, 6},
                               {7, 7},    {40, 10}, {200, 11}, {50, 13}, {60, 14}, {1, 16},
                               {128, 16}, {129, 16}, {2, 3}};
  for (auto& kp : plans) {
    if (!rse::locate_in_scope(8, kp[0], kp[1])) return 1;
    print_plan(rse::make_locate_plan(kp[0], kp[1]));
  }
  if (rse::locate_in_scope(16, 10, 4) || rse::locate_in_scope(8, 10, 17) ||
      rse::locate_in_scope(8, 200, 56) || rse::locate_in_scope(8, 10, 0))
    return 1;

  // seeded columns: 40 for each error count 0 .. p
  const uint32_t small[][2] = {{3, 2}, {6, 4}, {4, 5}};
  for (auto& kp : small) {
    const LocatePlan pl = rse::make_locate_plan(kp[0], kp[1]);
    std::vector<uint8_t> consts(rse::locate_consts_bytes(pl));
    rse::locate_consts(pl, consts.data());
    g_rng = seed * 0x9E3779B97F4A7C15ull + kp[0] * 131u + kp[1];
    size_t idx = 0;
    for (uint32_t ne = 0; ne <= pl.p; ++ne)
      for (int c = 0; c < 40; ++c) column(pl, consts.data(), idx++, pick(pl.n, ne));
  }

  // the ends of the point shift
  {
    const LocatePlan pl = rse::make_locate_plan(10, 4);
    std::vector<uint8_t> consts(rse::locate_consts_bytes(pl));
    rse::locate_consts(pl, consts.data());
    g_rng = seed + 1;
    column(pl, consts.data(), 1000, {0});
    column(pl, consts.data(), 1001, {13});
    column(pl, consts.data(), 1002, {0, 13});
  }
  {
    const LocatePlan pl = rse::make_locate_plan(239, 16);
    std::vector<uint8_t> consts(rse::locate_consts_bytes(pl));
    rse::locate_consts(pl, consts.data());
    g_rng = seed + 2;
    column(pl, consts.data(), 1000, {0});
    column(pl, consts.data(), 1001, {254});
    column(pl, consts.data(), 1002, {0, 254});
    column(pl, consts.data(), 1003, {0, 1, 100, 238, 239, 240, 253, 254});
    column(pl, consts.data(), 1004, {});
  }

  // every parity count 6 .. 16, single-chunk and multi-chunk k, k = 1
  const uint32_t wide[][2] = {{20, 8},  {6, 9},   {30, 15}, {12, 12},  {5, 6},    {7, 7},
                              {40, 10}, {200, 11}, {50, 13}, {60, 14},  {1, 16},   {128, 16},
                              {129, 16}, {100, 16}, {239, 16}, {2, 3}};
  for (auto& kp : wide) grid(kp[0], kp[1], seed);
  return 0;
}
