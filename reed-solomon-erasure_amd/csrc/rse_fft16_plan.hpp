// rse_fft16_plan.hpp -- host tables of the pruned additive-FFT kernel for
// GF(2^16) codecs past 256 shards (rse_fft16.hip).  Host only: no HIP
// includes, so a plain C++ program can walk it (tests/native/fft16_plan.cpp).
//
// The algebra.  Parity row j of the reference's matrix is P(k + j), P the
// polynomial of degree < k with P(i) = d_i (rse_fft.hip), and over GF(2^16) the
// point of shard i is the element i (galois_16.rs:49-51).  Let n = 2^m be the
// smallest power of two >= k + p and u = n - k.  The points 0 .. n-1 are the
// F2-span of 1, 2, .. n/2, and ifft is the Lin-Chung-Han inverse transform on
// them (tests/test_fft_math.py, beta = 0): values -> novel-basis coefficients,
// X_j of degree exactly j, so "degree < k" means coefficients k .. n-1 vanish.
//
// Take any set S of k points whose values are known and the set U of the other
// u points.  With c = ifft(values on S, zero on U) and H[q] the coefficients
// k .. n-1 of ifft(e_q), the coefficients k .. n-1 of the true polynomial are
// 0 = c[k..] + sum over q in U of P(q) H[q], so
//     (P(q))_{q in U} = A_U^-1 c[k .. n-1],   A_U = (H[q])_{q in U} as columns;
// A_U is invertible because the interpolating polynomial is unique.  Encode
// is S = {0 .. k-1}; reconstruct takes S = the first k present shards, which
// are the reference's valid shards (core.rs:801-841), so the bytes are the
// reference's for inconsistent inputs too.
//
// Pruning.  Only the top u <= 32 coefficients are needed.  Levels >= 5 of the
// inverse transform only XOR lower halves into upper ones as far as the last
// 32 outputs are concerned, so coefficients n-32 .. n-1 are the XOR over the
// n/32 blocks of 32 consecutive points of each block's own 5-level transform
// (twiddles s^_i(32 blk ^ j), i < 5): 80 butterflies per block.  The top u of
// those 32 are c[k .. n-1].  ifft(e_q) touches only q's block.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "rse_field.hpp"

namespace rse {

constexpr uint32_t kFft16Block = 32;   // points per block, 5 levels
constexpr uint32_t kFft16Levels = 5;
// Twiddle t of a block: level i, group g = (element in block) >> (i + 1), at
// fft16_tw_index(i, g): 16 + 8 + 4 + 2 + 1 = 31 of 32 entries used.
constexpr uint32_t fft16_tw_index(uint32_t level, uint32_t group) {
  return (kFft16Block - (kFft16Block >> level)) + group;
}

// The shapes the kernel serves: k + p > 256 (GF(2^16) proper) and
// u = 2^m - k <= 32.
inline bool fft16_shape(uint32_t k, uint32_t p, uint32_t* n_out, uint32_t* u_out) {
  if (k == 0 || p == 0 || (uint64_t)k + p <= 256 || (uint64_t)k + p > 65536) return false;
  uint32_t n = 512;
  while (n < k + p) n <<= 1;
  if (n - k > kFft16Block) return false;
  if (n_out) *n_out = n;
  if (u_out) *u_out = n - k;
  return true;
}

// Multiplication by t as a 16 x 16 bit matrix over the kernels' planes (plane
// q is bit q ^ 8 of the element, rse_bitslice_core.hpp BitsF16): bit c of
// rows[r] set iff input plane c contributes to output plane r.
inline void fft16_bit_matrix(uint16_t t, uint16_t (&rows)[16]) {
  for (int r = 0; r < 16; ++r) rows[r] = 0;
  for (int c = 0; c < 16; ++c) {
    const uint16_t y = Gf16Field::mul(t, (uint16_t)(1u << (c ^ 8)));
    for (int r = 0; r < 16; ++r)
      if ((y >> (r ^ 8)) & 1u) rows[r] |= (uint16_t)(1u << c);
  }
}

struct Fft16Plan {
  uint32_t k = 0, p = 0, n = 0, u = 0, nblk = 0;
  std::vector<uint16_t> tw;    // [nblk][32]: s^_i(32 blk ^ j) at fft16_tw_index
  std::vector<uint16_t> h;     // [n][u]: H[q], coefficients k .. n-1 of ifft(e_q)
  std::vector<uint16_t> enc;   // [p][u]: the first p rows of A^-1, A = (H[k] .. H[n-1])
  std::vector<uint16_t> rows;  // [p][k]: enc . (H[0] .. H[k-1]) = the codec's parity rows

  // The 5-level inverse transform of block blk, in place on 32 elements.
  void block_ifft(uint32_t blk, uint16_t (&d)[kFft16Block]) const {
    for (uint32_t i = 0; i < kFft16Levels; ++i) {
      const uint32_t hh = 1u << i;
      for (uint32_t j = 0; j < kFft16Block; j += 2 * hh) {
        const uint16_t s = tw[(size_t)blk * kFft16Block + fft16_tw_index(i, j >> (i + 1))];
        for (uint32_t t = j; t < j + hh; ++t) {
          d[t + hh] ^= d[t];
          d[t] ^= Gf16Field::mul(s, d[t + hh]);
        }
      }
    }
  }
  // c[k .. n-1] of the values v[q] on the points listed in `pts` (zero
  // elsewhere): the pruned transform as the kernel runs it.
  void top_coefficients(const std::vector<uint32_t>& pts, const uint16_t* v, uint16_t* c) const {
    std::vector<uint16_t> full(n, 0);
    for (size_t i = 0; i < pts.size(); ++i) full[pts[i]] = v[i];
    uint16_t acc[kFft16Block] = {};
    for (uint32_t b = 0; b < nblk; ++b) {
      uint16_t d[kFft16Block];
      for (uint32_t j = 0; j < kFft16Block; ++j) d[j] = full[(size_t)b * kFft16Block + j];
      block_ifft(b, d);
      for (uint32_t j = 0; j < kFft16Block; ++j) acc[j] ^= d[j];
    }
    for (uint32_t j = 0; j < u; ++j) c[j] = acc[kFft16Block - u + j];
  }
};

inline bool fft16_invert(const std::vector<uint16_t>& a, uint32_t u, std::vector<uint16_t>& out) {
  Matrix<Gf16Field> m(u, u), inv;
  m.d = a;
  if (!m.invert(inv)) return false;
  out = inv.d;
  return true;
}

inline bool fft16_make_plan(uint32_t k, uint32_t p, Fft16Plan& pl) {
  uint32_t n = 0, u = 0;
  if (!fft16_shape(k, p, &n, &u)) return false;
  pl.k = k;
  pl.p = p;
  pl.n = n;
  pl.u = u;
  pl.nblk = n / kFft16Block;
  // s_i(x) = prod over a in span(1 .. 2^(i-1)) of (x + a) is F2-linear in x, so
  // s_i(32 blk ^ j) = XOR of s_i(2^b) over the set bits b of 32 blk ^ j
  uint32_t bits = 0;
  while ((1u << bits) < n) ++bits;
  std::vector<uint16_t> basis(kFft16Levels * bits), norm(kFft16Levels);
  for (uint32_t i = 0; i < kFft16Levels; ++i) {
    auto s_i = [&](uint16_t x) {
      uint16_t r = 1;
      for (uint32_t a = 0; a < (1u << i); ++a) r = Gf16Field::mul(r, (uint16_t)(x ^ a));
      return r;
    };
    norm[i] = Gf16Field::inv(s_i((uint16_t)(1u << i)));
    for (uint32_t b = 0; b < bits; ++b)
      basis[i * bits + b] = Gf16Field::mul(s_i((uint16_t)(1u << b)), norm[i]);
  }
  pl.tw.assign((size_t)pl.nblk * kFft16Block, 0);
  for (uint32_t blk = 0; blk < pl.nblk; ++blk)
    for (uint32_t i = 0; i < kFft16Levels; ++i)
      for (uint32_t g = 0; g < (kFft16Block >> (i + 1)); ++g) {
        const uint32_t x = blk * kFft16Block + (g << (i + 1));
        uint16_t s = 0;
        for (uint32_t b = 0; b < bits; ++b)
          if ((x >> b) & 1u) s ^= basis[i * bits + b];
        pl.tw[(size_t)blk * kFft16Block + fft16_tw_index(i, g)] = s;
      }
  pl.h.assign((size_t)n * u, 0);
  for (uint32_t q = 0; q < n; ++q) {
    uint16_t d[kFft16Block] = {};
    d[q % kFft16Block] = 1;
    pl.block_ifft(q / kFft16Block, d);
    for (uint32_t j = 0; j < u; ++j) pl.h[(size_t)q * u + j] = d[kFft16Block - u + j];
  }
  std::vector<uint16_t> a((size_t)u * u), ainv;
  for (uint32_t c = 0; c < u; ++c)
    for (uint32_t j = 0; j < u; ++j) a[(size_t)c * u + j] = pl.h[(size_t)(k + j) * u + c];
  if (!fft16_invert(a, u, ainv)) return false;
  pl.enc.assign(ainv.begin(), ainv.begin() + (size_t)p * u);
  pl.rows.assign((size_t)p * k, 0);
  for (uint32_t r = 0; r < p; ++r)
    for (uint32_t q = 0; q < k; ++q) {
      uint16_t v = 0;
      for (uint32_t c = 0; c < u; ++c)
        v ^= Gf16Field::mul(pl.enc[(size_t)r * u + c], pl.h[(size_t)q * u + c]);
      pl.rows[(size_t)r * k + q] = v;
    }
  return true;
}

// A reconstruct pattern: `valid` = S, the first k present shards in index order;
// `lost` the shards to rebuild (not present; parity only unless data_only);
// mat[lost][u] the rows of A_U^-1 for them.  False if fewer than k are present.
struct Fft16Pattern {
  std::vector<uint32_t> valid, lost;
  std::vector<uint16_t> mat;
};
inline bool fft16_pattern(const Fft16Plan& pl, const uint8_t* present, bool data_only,
                          Fft16Pattern& pt) {
  const uint32_t k = pl.k, u = pl.u, total = pl.k + pl.p;
  std::vector<uint32_t> other;  // U
  pt.valid.clear();
  pt.lost.clear();
  for (uint32_t q = 0; q < pl.n; ++q) {
    if (q < total && present[q] && pt.valid.size() < k) pt.valid.push_back(q);
    else other.push_back(q);
  }
  if (pt.valid.size() < k || other.size() != u) return false;
  std::vector<uint16_t> a((size_t)u * u), ainv;
  for (uint32_t c = 0; c < u; ++c)
    for (uint32_t j = 0; j < u; ++j) a[(size_t)c * u + j] = pl.h[(size_t)other[j] * u + c];
  if (!fft16_invert(a, u, ainv)) return false;
  pt.mat.clear();
  for (uint32_t j = 0; j < u; ++j) {
    const uint32_t q = other[j];
    if (q >= total || present[q] || (data_only && q >= k)) continue;
    pt.lost.push_back(q);
    pt.mat.insert(pt.mat.end(), ainv.begin() + (size_t)j * u, ainv.begin() + (size_t)(j + 1) * u);
  }
  return true;
}

// The coefficients of the pattern's outputs over its k valid inputs
// (rows[lost][k]): what the kernel computes, as a plain matrix for the bytes
// past the last whole column.
inline void fft16_pattern_rows(const Fft16Plan& pl, const Fft16Pattern& pt,
                               std::vector<uint16_t>& rows) {
  const uint32_t k = pl.k, u = pl.u;
  rows.assign(pt.lost.size() * (size_t)k, 0);
  for (size_t r = 0; r < pt.lost.size(); ++r)
    for (uint32_t i = 0; i < k; ++i) {
      uint16_t v = 0;
      for (uint32_t c = 0; c < u; ++c)
        v ^= Gf16Field::mul(pt.mat[r * u + c], pl.h[(size_t)pt.valid[i] * u + c]);
      rows[r * k + i] = v;
    }
}

}  // namespace rse
