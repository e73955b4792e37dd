// rse_correct_plan.hpp -- the column decoder of rse_correct_flat: error VALUES
// on top of the locations of rse_locate_plan.hpp, with known-missing shards
// (erasures) taken into account.  Plain C++ like the header it extends; the
// decoder is __host__ __device__ under hipcc, so the CPU tests run the code the
// kernel (rse_correct.hip) runs.
//
// Notation of rse_locate_plan.hpp: X_r = y_r = r ^ 0xFF, w_r = u_r e_r for a
// shard r that is off by e_r, S_j = sum_r w_r X_r^j (j < p), S(x) = sum S_j x^j.
// With the erased set E (|E| = f <= p) and the error set B (|B| = nu):
//   Gamma(x) = prod_{r in E} (1 - X_r x)          erasure locator, per stripe
//   Xi       = S Gamma mod x^p                    Forney syndromes: Xi_f .. Xi_{p-1}
//                                                 obey the recurrence of the errors alone
//   Lambda   = Berlekamp-Massey over those p - f values, length <= (p - f) / 2
//   Psi      = Lambda Gamma,   Omega = S Psi mod x^p
//   w_r      = X_r Omega(1 / X_r) / Psi'(1 / X_r)  at every root 1 / X_r of Psi
//   e_r      = w_r (1 / u_r),  1 / u_r = prod_{s != r} (r ^ s)
// (Omega = sum_r w_r prod_{s != r} (1 - X_s x) over the roots, of degree
// < nu + f <= p, so nothing of it is lost modulo x^p; in characteristic 2 Psi'
// is the odd coefficients of Psi shifted down.)  Without erasures Gamma = 1 and
// this is the plain Forney formula.  The column is undecodable when the length
// cap is exceeded, when Lambda has not exactly L roots among the n points, or
// when one of them is an erased point.
#pragma once

#include "rse_locate_plan.hpp"

namespace rse {

// Byte layout of the plan on the device: rse_locate_plan.hpp's (log, exp, T,
// P: at most 16 x 239 bytes from kLocRowsOff), then 1 / u_r for r < n.
constexpr size_t kCorInvUOff = 5120;
constexpr size_t kCorConstsBytes = kCorInvUOff + 256;
static_assert(kLocRowsOff + 16 * 239 <= kCorInvUOff, "P must end before 1/u");

constexpr uint32_t kCorGammaWords = 5;  // Gamma, Psi: 17 bytes (degrees 0 .. 16)

// The erasures of one stripe: the same for every column, so on the device
// these live in LDS and a run-time index into them is a plain LDS read.
struct CorrectErasures {
  uint32_t f;             // erased shards; f > p: nothing is decodable
  const uint8_t* pos;     // the first min(f, 16) of them, any order
  const uint32_t* gamma;  // Gamma packed, kCorGammaWords words (correct_gamma)
  const uint32_t* mask;   // 8 words: bit r = shard r is erased
};

namespace correct_detail {
// c ^= exp(lcoef) * b over the bytes I .. min(N, lim) - 1 of both
template <int I, int N, int NW>
RSE_LOC_HD void axpy(const uint8_t* lg, const uint8_t* ex, uint32_t (&c)[NW],
                     const uint32_t (&b)[NW], uint32_t lcoef, uint32_t lim) {
  if constexpr (I < N) {
    if ((uint32_t)I < lim) {
      const uint32_t bi = pk_at<I>(b);
      const uint32_t v = bi ? (uint32_t)ex[(uint32_t)lg[bi] + lcoef] : 0u;
      c[I >> 2] ^= v << ((I & 3) * 8);
      axpy<I + 1, N, NW>(lg, ex, c, b, lcoef, lim);
    }
  }
}
// w <- w x: every byte one place up, the top one dropped
template <int NW>
RSE_LOC_HD void shl8(uint32_t (&w)[NW]) {
  RSE_LOC_UNROLL
  for (int q = NW - 1; q > 0; --q) w[q] = (w[q] << 8) | (w[q - 1] >> 24);
  w[0] <<= 8;
}
// w <- w (1 - X_r x) for the 17-byte polynomials; deg: the degree of w before
RSE_LOC_HD void mul_linear(const uint8_t* lg, const uint8_t* ex, uint32_t (&w)[kCorGammaWords],
                           uint32_t r, uint32_t deg) {
  uint32_t sh[kCorGammaWords];
  RSE_LOC_UNROLL
  for (uint32_t q = 0; q < kCorGammaWords; ++q) sh[q] = w[q];
  shl8(sh);
  axpy<1, 17>(lg, ex, w, sh, (uint32_t)lg[r ^ 0xFFu], deg + 2u);
}
}  // namespace correct_detail

// Gamma of the erased shards pos[0 .. f), f <= 16, packed into
// kCorGammaWords words.
RSE_LOC_HD void correct_gamma(const uint8_t* lg, const uint8_t* ex, const uint8_t* pos, uint32_t f,
                              uint32_t* gamma) {
  uint32_t g[kCorGammaWords] = {1u, 0u, 0u, 0u, 0u};
  for (uint32_t i = 0; i < f; ++i) correct_detail::mul_linear(lg, ex, g, pos[i], i);
  for (uint32_t q = 0; q < kCorGammaWords; ++q) gamma[q] = g[q];
}

// One byte column that is not a codeword, from its syndromes S_0 .. S_{p-1}
// (packed; the bytes from p on are zero, as locate_syndromes leaves them): the
// number m <= p of positions in which the one codeword within reach may differ
// from it -- the located errors, then every erased shard -- with the shard
// indices in pos[0 .. m) and the values to XOR in val[0 .. m) (zero where an
// erased shard's byte was right already), or kLocateBad when no codeword
// differs from the column in nu positions outside the erased set with
// 2 nu + f <= p.  invu: 1 / u_r, n bytes.  n = k + p <= 255, p <= 16.
RSE_LOC_HD uint32_t correct_column(const uint8_t* lg, const uint8_t* ex, const uint8_t* invu,
                                   const uint32_t (&S)[4], uint32_t p, uint32_t n,
                                   const CorrectErasures& er, uint32_t (&pos)[4],
                                   uint32_t (&val)[4]) {
  using namespace correct_detail;
  const uint32_t f = er.f;
  pos[0] = pos[1] = pos[2] = pos[3] = 0u;
  val[0] = val[1] = val[2] = val[3] = 0u;
  if (f > p) return kLocateBad;
  // Forney syndromes Xi_f .. Xi_{p-1}, moved down to 0 .. p-f-1
  uint32_t Q[4] = {S[0], S[1], S[2], S[3]};
  if (f != 0u) {
    Q[0] = Q[1] = Q[2] = Q[3] = 0u;
    for (uint32_t j = f; j < p; ++j) {
      uint32_t v = 0u;
      for (uint32_t i = 0; i <= f; ++i) {
        const uint32_t gi = (er.gamma[i >> 2] >> ((i & 3u) * 8u)) & 0xFFu;
        v ^= loc_mul(lg, ex, gi, pk_get(S, j - i));
      }
      pk_set(Q, j - f, v);
    }
  }
  uint32_t roots[2];
  const uint32_t L = locate_column(lg, ex, Q, p - f, n, roots);
  if (L == kLocateBad) return kLocateBad;
  // Psi = Gamma prod (1 - X_r x) over the located errors
  uint32_t Psi[kCorGammaWords] = {1u, 0u, 0u, 0u, 0u};
  if (f != 0u) {
    RSE_LOC_UNROLL
    for (uint32_t q = 0; q < kCorGammaWords; ++q) Psi[q] = er.gamma[q];
  }
  for (uint32_t i = 0; i < L; ++i) {
    const uint32_t r = pk_get(roots, i);
    if (f != 0u && ((er.mask[r >> 5] >> (r & 31u)) & 1u) != 0u) return kLocateBad;
    mul_linear(lg, ex, Psi, r, f + i);
  }
  const uint32_t m = L + f;
  // Omega = S Psi: the bytes below m are all that is read (deg Omega < m <= p)
  uint32_t Om[4] = {0u, 0u, 0u, 0u}, Sh[4] = {S[0], S[1], S[2], S[3]};
  for (uint32_t i = 0; i <= m; ++i) {
    const uint32_t c = pk_get(Psi, i);
    if (c != 0u) axpy<0, 16>(lg, ex, Om, Sh, (uint32_t)lg[c], m);
    shl8(Sh);
  }
  for (uint32_t q = 0; q < m; ++q) {
    const uint32_t r = q < L ? pk_get(roots, q) : (uint32_t)er.pos[q - L];
    const uint32_t ly = lg[r ^ 0xFFu];
    const uint32_t lx = ly ? 255u - ly : 0u;  // log(1 / X_r)
    uint32_t om = 0u;
    for (uint32_t i = m; i-- > 0u;)
      om = (om ? (uint32_t)ex[(uint32_t)lg[om] + lx] : 0u) ^ pk_get(Om, i);
    // Psi'(x) = sum over odd i of Psi_i x^(i-1): Horner in x^2, from the
    // largest odd i <= m down
    const uint32_t lx2 = 2u * lx >= 255u ? 2u * lx - 255u : 2u * lx;
    uint32_t dv = 0u;
    for (uint32_t i = (m - 1u) | 1u;; i -= 2u) {
      dv = (dv ? (uint32_t)ex[(uint32_t)lg[dv] + lx2] : 0u) ^ pk_get(Psi, i);
      if (i == 1u) break;
    }
    if (dv == 0u) return kLocateBad;  // a repeated root: never with distinct points
    uint32_t e = 0u;
    if (om != 0u) {
      uint32_t l = (uint32_t)lg[om] + 255u - (uint32_t)lg[dv];
      l = (l >= 255u ? l - 255u : l) + ly;  // X_r Omega / Psi', below 510: ex is doubled
      e = loc_mul(lg, ex, (uint32_t)ex[l], (uint32_t)invu[r]);
    }
    pk_set(pos, q, r);
    pk_set(val, q, e);
  }
  return m;
}

// 1 / u_r = prod_{s != r} (r ^ s) for r < n, n bytes
inline void correct_inv_u(size_t n, uint8_t* out) {
  for (size_t r = 0; r < n; ++r) {
    uint8_t prod = 1;
    for (size_t s = 0; s < n; ++s)
      if (s != r) prod = Gf8::mul(prod, (uint8_t)(r ^ s));
    out[r] = prod;
  }
}

// The plan as the device reads it: kCorConstsBytes bytes, rse_locate_flat's
// layout first, so one copy on the device serves both entries.
inline void correct_consts(const LocatePlan& pl, uint8_t* out) {
  for (size_t i = 0; i < kCorConstsBytes; ++i) out[i] = 0;
  locate_consts(pl, out);
  correct_inv_u(pl.n, out + kCorInvUOff);
}

}  // namespace rse
