// Walks rse_fft16_plan.hpp (the host tables of rse_fft16.hip) on the CPU for
// 500+12: prints the encode matrix, the matrix of a fixed erasure pattern, the
// parity rows, the parity of a fixed data column computed with the tables as
// the kernel does (pruned block transforms, then the matrix), and the rebuilt
// values of the pattern.  tests/test_fft16_plan.py compares all of it with the
// oracle.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rse_fft16_plan.hpp"

using rse::Fft16Pattern;
using rse::Fft16Plan;
using rse::Gf16Field;

static void print_row(const char* tag, const uint16_t* v, size_t n) {
  std::printf("%s", tag);
  for (size_t i = 0; i < n; ++i) std::printf(" %u", (unsigned)v[i]);
  std::printf("\n");
}

// out[r] = sum_c mat[r][c] coef[c]
static std::vector<uint16_t> apply(const std::vector<uint16_t>& mat, const uint16_t* coef,
                                   uint32_t u) {
  std::vector<uint16_t> out(mat.size() / u, 0);
  for (size_t r = 0; r < out.size(); ++r)
    for (uint32_t c = 0; c < u; ++c) out[r] ^= Gf16Field::mul(mat[r * u + c], coef[c]);
  return out;
}

int main() {
  const uint32_t k = 500, p = 12;
  Fft16Plan pl;
  if (!rse::fft16_make_plan(k, p, pl)) return 1;
  std::printf("plan k %u p %u n %u u %u nblk %u\n", pl.k, pl.p, pl.n, pl.u, pl.nblk);
  for (uint32_t r = 0; r < p; ++r) print_row("enc", &pl.enc[(size_t)r * pl.u], pl.u);
  for (uint32_t r = 0; r < p; ++r) print_row("row", &pl.rows[(size_t)r * k], k);

  // a fixed data column and its parity
  std::vector<uint16_t> col(k + p);
  std::vector<uint32_t> pts(k);
  uint32_t x = 12345;
  for (uint32_t i = 0; i < k; ++i) {
    x = x * 1664525u + 1013904223u;
    col[i] = (uint16_t)(x >> 16);
    pts[i] = i;
  }
  std::vector<uint16_t> coef(pl.u);
  pl.top_coefficients(pts, col.data(), coef.data());
  const std::vector<uint16_t> par = apply(pl.enc, coef.data(), pl.u);
  for (uint32_t r = 0; r < p; ++r) col[k + r] = par[r];
  print_row("data", col.data(), k);
  print_row("parity", par.data(), p);

  // a mixed pattern: data 3, 77, 499 and parity 1, 11 lost
  std::vector<uint8_t> present(k + p, 1);
  for (uint32_t q : {3u, 77u, 499u, k + 1u, k + 11u}) present[q] = 0;
  Fft16Pattern pt;
  if (!rse::fft16_pattern(pl, present.data(), false, pt)) return 2;
  std::vector<uint16_t> lostf(pt.lost.begin(), pt.lost.end());
  print_row("lost", lostf.data(), lostf.size());
  for (size_t r = 0; r < pt.lost.size(); ++r) print_row("pat", &pt.mat[r * pl.u], pl.u);
  std::vector<uint16_t> vals(k);
  for (uint32_t i = 0; i < k; ++i) vals[i] = col[pt.valid[i]];
  pl.top_coefficients(pt.valid, vals.data(), coef.data());
  const std::vector<uint16_t> back = apply(pt.mat, coef.data(), pl.u);
  print_row("rebuilt", back.data(), back.size());
  // the same outputs from the pattern's plain rows over the valid inputs
  std::vector<uint16_t> rows;
  rse::fft16_pattern_rows(pl, pt, rows);
  std::vector<uint16_t> back2(pt.lost.size(), 0);
  for (size_t r = 0; r < pt.lost.size(); ++r)
    for (uint32_t i = 0; i < k; ++i) back2[r] ^= Gf16Field::mul(rows[r * k + i], vals[i]);
  print_row("rebuilt_rows", back2.data(), back2.size());
  // multiplication as the kernels' bit matrix, on one value
  uint16_t bm[16];
  rse::fft16_bit_matrix(pl.enc[0], bm);
  uint16_t y = 0;
  for (int r = 0; r < 16; ++r) {
    unsigned bit = 0;
    for (int c = 0; c < 16; ++c)
      if ((bm[r] >> c) & 1u) bit ^= (coef[0] >> (c ^ 8)) & 1u;
    y |= (uint16_t)(bit << (r ^ 8));
  }
  std::printf("bitmul %u %u\n", (unsigned)y, (unsigned)Gf16Field::mul(pl.enc[0], coef[0]));
  return 0;
}
