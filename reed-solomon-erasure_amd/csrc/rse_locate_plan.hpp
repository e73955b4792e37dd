// rse_locate_plan.hpp -- host plan and column decoder of rse_locate_flat
// (error LOCATION: which shards of a stripe are wrong, not merely that some
// are).  Plain C++: no HIP needed; the two decoder functions are
// __host__ __device__ under hipcc, so the CPU tests run the code the kernel
// (rse_locate.hip) runs.
//
// The codec's matrix is V (V[0..k])^-1 with V[r][c] = r^c (core.rs:430-436):
// every byte column of a stripe is the evaluation of a polynomial of degree
// < k at the points 0 .. n-1 (n = k + p), a Reed-Solomon code of minimum
// distance p + 1.  Such a code is invariant under translating its points
// (f(x) and f(x + c) have the same degree), so the decoder works with
//   y_r = r ^ 0xFF,  r = 0 .. n-1,
// all nonzero because n <= 255: the locator never meets the point 0.
//
// Check matrix (the dual of a generalised Reed-Solomon code):
//   u_r = 1 / prod_{s != r} (r ^ s),   H[j][r] = u_r y_r^j,  j = 0 .. p-1,
// so H M = 0 for the codec's n x k matrix M.  With d = P data ^ parity (the
// p-vector the check kernels form per column) the power-sum syndromes of the
// column are S = T d, T[j][i] = H[j][k + i]: if shard r is off by e_r,
//   S_j = sum_r (u_r e_r) y_r^j.
// Berlekamp-Massey over S_0 .. S_{p-1} gives the shortest recurrence Lambda of
// length L; up to t = p / 2 errors are located exactly as the r with
// Lambda(1 / y_r) = 0.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "rse_field.hpp"

#if defined(__HIPCC__)
#define RSE_LOC_HD __host__ __device__ __forceinline__
#else
#define RSE_LOC_HD inline
#endif
#if defined(__clang__)
#define RSE_LOC_UNROLL _Pragma("unroll")
#else
#define RSE_LOC_UNROLL
#endif

namespace rse {

constexpr uint32_t kLocateMaxParity = 16;  // S fits four words
constexpr uint32_t kLocateMaxT = 8;        // Lambda, B: nine bytes in three words
constexpr uint32_t kLocateBad = 0xFFu;     // locate_column: the column is undecodable

// GF(2^8) codecs with 1 <= p <= 16 and k + p <= 255 (a spare field point for
// the shift above).
inline bool locate_in_scope(int field, size_t k, size_t p) {
  return field == 8 && k >= 1 && p >= 1 && p <= kLocateMaxParity && k + p <= 255;
}

// ---- packed byte vectors -----------------------------------------------------
// The decoder's small arrays live as bytes packed into NW words and are read
// and written through unrolled selects, never through a run-time index into
// an array: on the device they stay in a few VGPRs instead of scratch.  Every
// word is read unconditionally and the select is made on the VALUES: a
// conditional read is folded back into a read at a computed address.
template <int NW>
RSE_LOC_HD uint32_t pk_get(const uint32_t (&w)[NW], uint32_t i) {
  uint32_t v = w[0];
  RSE_LOC_UNROLL
  for (int q = 1; q < NW; ++q) {
    const uint32_t wq = w[q];
    v = (i >> 2) == (uint32_t)q ? wq : v;
  }
  return (v >> ((i & 3u) * 8u)) & 0xFFu;
}
template <int NW>
RSE_LOC_HD void pk_set(uint32_t (&w)[NW], uint32_t i, uint32_t b) {
  const uint32_t sh = (i & 3u) * 8u, m = 0xFFu << sh;
  RSE_LOC_UNROLL
  for (int q = 0; q < NW; ++q) {
    const uint32_t old = w[q];
    w[q] = (i >> 2) == (uint32_t)q ? ((old & ~m) | (b << sh)) : old;
  }
}
// byte I of w, I known at compile time
template <int I, int NW>
RSE_LOC_HD uint32_t pk_at(const uint32_t (&w)[NW]) {
  return (w[I >> 2] >> ((I & 3) * 8)) & 0xFFu;
}

// a * b through lg[256] / ex[512] (rse_field.hpp Gf8: generator 2 modulo 0x11D)
RSE_LOC_HD uint32_t loc_mul(const uint8_t* lg, const uint8_t* ex, uint32_t a, uint32_t b) {
  return (a != 0u && b != 0u) ? (uint32_t)ex[(uint32_t)lg[a] + (uint32_t)lg[b]] : 0u;
}

// S = T d: d and S are p bytes packed into four words, T is p x p with rows
// kLocateMaxParity bytes apart.
RSE_LOC_HD void locate_syndromes(const uint8_t* lg, const uint8_t* ex, const uint8_t* T,
                                 const uint32_t (&d)[4], uint32_t p, uint32_t (&S)[4]) {
  S[0] = S[1] = S[2] = S[3] = 0u;
  for (uint32_t i = 0; i < p; ++i) {
    const uint32_t di = pk_get(d, i);
    if (di == 0u) continue;
    const uint32_t ld = lg[di];
    for (uint32_t j = 0; j < p; ++j) {
      const uint32_t c = T[j * kLocateMaxParity + i];  // never zero: u_r and y_r are not
      const uint32_t v = ex[ld + (uint32_t)lg[c]];
      const uint32_t sh = (j & 3u) * 8u;
      RSE_LOC_UNROLL
      for (int q = 0; q < 4; ++q) S[q] ^= (j >> 2) == (uint32_t)q ? (v << sh) : 0u;
    }
  }
}

namespace locate_detail {
// c ^= coef * b over the nine bytes (degrees 0 .. 8) of both
template <int I>
RSE_LOC_HD void axpy9(const uint8_t* lg, const uint8_t* ex, uint32_t (&c)[3],
                      const uint32_t (&b)[3], uint32_t lcoef) {
  if constexpr (I < 9) {
    const uint32_t bi = pk_at<I>(b);
    const uint32_t v = bi ? (uint32_t)ex[(uint32_t)lg[bi] + lcoef] : 0u;
    c[I >> 2] ^= v << ((I & 3) * 8);
    axpy9<I + 1>(lg, ex, c, b, lcoef);
  }
}
// sum_{i = I .. 8, i <= L} C_i S_{n - i}
template <int I>
RSE_LOC_HD uint32_t discrepancy(const uint8_t* lg, const uint8_t* ex, const uint32_t (&C)[3],
                                const uint32_t (&S)[4], uint32_t n, uint32_t L) {
  if constexpr (I <= 8) {
    uint32_t v = 0u;
    if ((uint32_t)I <= L) v = loc_mul(lg, ex, pk_at<I>(C), pk_get(S, n - (uint32_t)I));
    return v ^ discrepancy<I + 1>(lg, ex, C, S, n, L);
  } else {
    return 0u;
  }
}
// Horner: C_L x^(L - I) + .. + C_I for x = exp(lx), from the top degree down
template <int I>
RSE_LOC_HD uint32_t horner(const uint8_t* lg, const uint8_t* ex, const uint32_t (&C)[3],
                           uint32_t L, uint32_t lx, uint32_t v) {
  if ((uint32_t)I <= L) {
    v = v ? (uint32_t)ex[(uint32_t)lg[v] + lx] : 0u;
    v ^= pk_at<I>(C);
  }
  if constexpr (I > 0) return horner<I - 1>(lg, ex, C, L, lx, v);
  return v;
}
}  // namespace locate_detail

// One byte column: from its syndromes S_0 .. S_{p-1} (packed), the number L of
// wrong shards (0: a codeword) with their indices in roots[0 .. L), ascending,
// or kLocateBad when no codeword lies within t = p / 2 of the column.
// n = k + p <= 255, p <= 16.
RSE_LOC_HD uint32_t locate_column(const uint8_t* lg, const uint8_t* ex, const uint32_t (&S)[4],
                                  uint32_t p, uint32_t n, uint32_t (&roots)[2]) {
  using namespace locate_detail;
  const uint32_t t = p >> 1;
  roots[0] = roots[1] = 0u;
  // Berlekamp-Massey (Massey's form).  C is the connection polynomial, B the
  // one before the last length change, kept already multiplied by x^m.  A
  // length change to more than t ends the column, so whenever x^m B is used
  // its degree is at most t <= 8 and nine bytes hold it; bytes shifted out of
  // a B that is never used again are never missed.
  uint32_t C[3] = {1u, 0u, 0u}, B[3] = {1u, 0u, 0u};
  uint32_t L = 0u, lb = 0u;  // lb = log of the discrepancy at the last length change
  for (uint32_t i = 0; i < p; ++i) {
    B[2] = (B[2] << 8) | (B[1] >> 24);
    B[1] = (B[1] << 8) | (B[0] >> 24);
    B[0] <<= 8;
    const uint32_t d = pk_get(S, i) ^ discrepancy<1>(lg, ex, C, S, i, L);
    if (d == 0u) continue;
    const uint32_t lcoef = (uint32_t)lg[d] + 255u - lb;  // log(d / b) + 0 or 255: ex is doubled
    const uint32_t lc = lcoef >= 255u ? lcoef - 255u : lcoef;
    if (2u * L <= i) {
      const uint32_t nl = i + 1u - L;
      if (nl > t) return kLocateBad;
      const uint32_t T0 = C[0], T1 = C[1], T2 = C[2];
      axpy9<0>(lg, ex, C, B, lc);
      B[0] = T0;
      B[1] = T1;
      B[2] = T2;
      lb = lg[d];
      L = nl;
    } else {
      axpy9<0>(lg, ex, C, B, lc);
    }
  }
  if (L == 0u) return 0u;
  // Lambda(x) = prod (1 - y_r x) over the wrong shards r: its roots among the
  // points 1 / y_r.  Fewer than L of them: the recurrence is not an error
  // pattern of weight L.
  uint32_t cnt = 0u;
  for (uint32_t r = 0; r < n; ++r) {
    const uint32_t ly = lg[r ^ 0xFFu];
    const uint32_t lx = ly ? 255u - ly : 0u;  // log(1 / y_r)
    if (horner<8>(lg, ex, C, L, lx, 0u) == 0u) {
      if (cnt < 8u) pk_set(roots, cnt, r);
      ++cnt;
    }
  }
  return cnt == L ? L : kLocateBad;
}

// ---- host plan ---------------------------------------------------------------
struct LocatePlan {
  uint32_t k = 0, p = 0, n = 0, t = 0;
  std::vector<uint8_t> P;  // p x k: the codec's parity rows, row-major
  std::vector<uint8_t> H;  // p x n check matrix, row-major
  std::vector<uint8_t> T;  // p x p, rows kLocateMaxParity bytes apart: T[j][i] = H[j][k + i]
};

// Byte layout of the plan on the device (rse_locate.hip reads it).
constexpr size_t kLocLogOff = 0;     // log[256]
constexpr size_t kLocExpOff = 256;   // exp[512]
constexpr size_t kLocTOff = 768;     // T, 16 x 16
constexpr size_t kLocRowsOff = 1024; // P, p x k
inline size_t locate_consts_bytes(const LocatePlan& pl) { return kLocRowsOff + pl.P.size(); }

// parity_rows: the codec's p x k parity rows when the caller has them (row
// stride k, uint16 elements as rse_codec keeps them); null: built here as
// core.rs:430-436 does.
inline LocatePlan make_locate_plan(size_t k, size_t p, const uint16_t* parity_rows = nullptr) {
  LocatePlan pl;
  pl.k = (uint32_t)k;
  pl.p = (uint32_t)p;
  pl.n = (uint32_t)(k + p);
  pl.t = (uint32_t)(p / 2);
  const size_t n = k + p;
  pl.P.assign(p * k, 0);
  if (parity_rows) {
    for (size_t q = 0; q < p * k; ++q) pl.P[q] = (uint8_t)parity_rows[q];
  } else {
    using M = Matrix<Gf8Field>;
    const M v = M::vandermonde(n, k);
    M top(k, k), inv;
    for (size_t r = 0; r < k; ++r)
      for (size_t c = 0; c < k; ++c) top.at(r, c) = v.at(r, c);
    top.invert(inv);  // distinct points: never singular
    const M m = v.multiply(inv);
    for (size_t r = 0; r < p; ++r)
      for (size_t c = 0; c < k; ++c) pl.P[r * k + c] = (uint8_t)m.at(k + r, c);
  }
  pl.H.assign(p * n, 0);
  pl.T.assign(kLocateMaxParity * kLocateMaxParity, 0);
  for (size_t r = 0; r < n; ++r) {
    uint8_t prod = 1;
    for (size_t s = 0; s < n; ++s)
      if (s != r) prod = Gf8::mul(prod, (uint8_t)(r ^ s));
    const uint8_t u = Gf8::inv(prod);
    const uint8_t y = (uint8_t)(r ^ 0xFFu);
    for (size_t j = 0; j < p; ++j) {
      const uint8_t h = Gf8::mul(u, Gf8::pow(y, j));
      pl.H[j * n + r] = h;
      if (r >= k) pl.T[j * kLocateMaxParity + (r - k)] = h;
    }
  }
  return pl;
}

// The plan as the device reads it: locate_consts_bytes(pl) bytes.
inline void locate_consts(const LocatePlan& pl, uint8_t* out) {
  for (size_t i = 0; i < 256; ++i) out[kLocLogOff + i] = Gf8::log_table()[i];
  for (size_t i = 0; i < 512; ++i) out[kLocExpOff + i] = Gf8::exp_table()[i];
  for (size_t i = 0; i < 256; ++i) out[kLocTOff + i] = pl.T[i];
  for (size_t i = 0; i < pl.P.size(); ++i) out[kLocRowsOff + i] = pl.P[i];
}

}  // namespace rse
