// rse_fft_sched.hpp -- the compile-time math and the schedule of the
// additive-FFT kernels (rse_fft.hip), free of device code so that a plain
// C++17 compiler can include it: tests/native/fft_schedule.cpp walks the same
// templates on scalar bytes and tests/test_fft_schedule.py compares the walk
// with the oracle.
//
// A workgroup of W waves holds the K elements (shards) of a byte column, E per
// wave, and runs the encode transform (the inverse FFT at shift B0, levels
// 0 .. m-1, then the forward one at B1, levels m-1 .. 0; m = log2 K) in three
// phases with an exchange through LDS between them:
//   phase A: wave h holds elements E h .. E h + E-1 (MapAC) and runs the
//            inverse levels 0 .. LA-1 (LA = log2 E; twiddles per wave);
//   phase B: wave w holds GPW groups of G = K / E elements with the same low
//            LA bits (MapB) and runs the inverse levels LA .. m-1, then the
//            forward levels m-1 .. LA (only bits >= LA matter to them, so the
//            twiddles are the same for every wave);
//   phase C: wave h holds its own elements again and runs the forward levels
//            LA-1 .. 0.
//   K          16  32  64  128
//   E           8   8   8   16
//   W           2   4   8    8
//   G           2   4   8    8
//   GPW         4   2   1    2
// The butterflies themselves come from an Ops policy: Ops::bfly<I, J, C, INV>
// (a, b) is the butterfly of level I, block offset J, twiddle C (the kernels:
// XOR networks over 8 bit planes; the host walk: one byte).
#pragma once

#include "rse_kernels.hpp"  // hb_mul8

#ifdef __HIPCC__
#define RSE_FFT_FN __device__ __forceinline__
#else
#define RSE_FFT_FN inline
#endif

namespace rse {
namespace {

// ------------------------------------------------------ field, at compile time
constexpr uint32_t f8_inv(uint32_t a) {
  for (uint32_t x = 1; x < 256; ++x)
    if (hb_mul8(a, x) == 1u) return x;
  return 0;
}
// s_i(x): the subspace polynomial of span(1, 2, .. 2^(i-1)) at x
constexpr uint32_t fft_vanish(int i, uint32_t x) {
  uint32_t r = 1;
  for (uint32_t a = 0; a < (1u << i); ++a) r = hb_mul8(r, x ^ a);
  return r;
}
// s^_i(x) = s_i(x) / s_i(2^i): the butterfly twiddle of level i at shift x
constexpr uint32_t fft_skew(int i, uint32_t x) {
  return hb_mul8(fft_vanish(i, x), f8_inv(fft_vanish(i, 1u << i)));
}
// Row q of the 8 x 8 bit matrix of multiplication by c: bit j set when bit q
// of c . 2^j is (the planes of b that plane q of c . b XORs).
constexpr uint64_t fft_row(uint32_t c, int q) {
  uint64_t m = 0;
  for (int j = 0; j < 8; ++j)
    if ((hb_mul8(c, 1u << j) >> q) & 1u) m |= 1ull << j;
  return m;
}
constexpr int fft_log2(int k) { return k <= 1 ? 0 : 1 + fft_log2(k / 2); }

// ------------------------------------------------------------------ schedule
template <int K>
struct FftSched {
  static constexpr int E = K > 64 ? 16 : 8;  // elements per wave
  static constexpr int W = K / E;            // waves
  static constexpr int M = fft_log2(K);      // levels
  static constexpr int LA = fft_log2(E);     // levels 0 .. LA-1: phases A and C
  static constexpr int G = K / E;            // phase B: elements per group
  static constexpr int GPW = E / G;          // ... groups per wave
  // the LDS slot (= element) of register t of wave w, phases A / C and B
  static constexpr int ac_slot(int w, int t) { return E * w + t; }
  static constexpr int b_slot(int w, int r) { return (w * GPW + r / G) + E * (r % G); }
};

// Which element register r of a wave holds, and back, by phase.
//  A / C: wave H holds elements E H + r.
template <int E, int H>
struct MapAC {
  static constexpr int elem(int r) { return E * H + r; }
  static constexpr int reg(int e) { return e - E * H; }
};
//  B: the wave's groups of G = K / E elements with the same low log2 E bits,
//  register gi * G + t = element g + E t.  Only bits >= log2 E matter to the
//  levels of phase B, so the first wave's map serves every wave.
template <int K, int E>
struct MapB {
  static constexpr int G = K / E;
  static constexpr int elem(int r) { return (r / G) + E * (r % G); }
  static constexpr int reg(int e) { return (e & (E - 1)) * G + (e / E); }
};

// One level I of a transform at shift BETA over the registers R .. R1-1: every
// one whose element has bit I clear is butterflied with its partner.
template <class Ops, class M, uint32_t BETA, int I, bool INV, int R, int R1, class X>
RSE_FFT_FN void fft_level(X& x) {
  if constexpr (R < R1) {
    constexpr int e = M::elem(R);
    if constexpr (((e >> I) & 1) == 0) {
      constexpr int r2 = M::reg(e + (1 << I));
      constexpr int j = e & ~((2 << I) - 1);
      constexpr uint32_t c = fft_skew(I, BETA ^ (uint32_t)j);
      Ops::template bfly<I, j, c, INV>(x[R], x[r2]);
    }
    fft_level<Ops, M, BETA, I, INV, R + 1, R1>(x);
  }
}

// Phase A of wave H (E elements), in parts: the inverse transform at B0,
// levels I .. I1-1, over the registers R0 .. R1-1 (whole: levels 0 .. LA-1
// over 0 .. E-1; the 16-element kernel: fft_a_quarters below).
template <class Ops, int E, int H, uint32_t B0, int I, int I1, int R0, int R1, class X>
RSE_FFT_FN void fft_phase_a(X& x) {
  if constexpr (I < I1) {
    fft_level<Ops, MapAC<E, H>, B0, I, true, R0, R1>(x);
    fft_phase_a<Ops, E, H, B0, I + 1, I1, R0, R1>(x);
  }
}
// Phase C of wave H: the forward transform at B1, levels I .. 0.
template <class Ops, int E, int H, uint32_t B1, int I, class X>
RSE_FFT_FN void fft_phase_c(X& x) {
  if constexpr (I >= 0) {
    fft_level<Ops, MapAC<E, H>, B1, I, false, 0, E>(x);
    fft_phase_c<Ops, E, H, B1, I - 1>(x);
  }
}
// Phase B: the inverse transform's levels LA .. m-1 at B0, then the forward
// transform's levels m-1 .. LA at B1.
template <class Ops, int K, uint32_t B0, int I, class X>
RSE_FFT_FN void fft_phase_b_inv(X& x) {
  using S = FftSched<K>;
  if constexpr (I < S::M) {
    fft_level<Ops, MapB<K, S::E>, B0, I, true, 0, S::E>(x);
    fft_phase_b_inv<Ops, K, B0, I + 1>(x);
  }
}
template <class Ops, int K, uint32_t B1, int I, class X>
RSE_FFT_FN void fft_phase_b_fwd(X& x) {
  using S = FftSched<K>;
  if constexpr (I >= S::LA) {
    fft_level<Ops, MapB<K, S::E>, B1, I, false, 0, S::E>(x);
    fft_phase_b_fwd<Ops, K, B1, I - 1>(x);
  }
}
template <class Ops, int K, uint32_t B0, uint32_t B1, class X>
RSE_FFT_FN void fft_phase_b(X& x) {
  fft_phase_b_inv<Ops, K, B0, FftSched<K>::LA>(x);
  fft_phase_b_fwd<Ops, K, B1, FftSched<K>::M - 1>(x);
}

// The wave-dependent phases, dispatched on the (uniform) wave index.
template <class Ops, int K, uint32_t B0, int I, int I1, int R0, int R1, int H = 0, class X>
RSE_FFT_FN void fft_a(int w, X& x) {
  if constexpr (H < FftSched<K>::W) {
    if (w == H) fft_phase_a<Ops, FftSched<K>::E, H, B0, I, I1, R0, R1>(x);
    else fft_a<Ops, K, B0, I, I1, R0, R1, H + 1>(w, x);
  }
}
template <class Ops, int K, uint32_t B1, int H = 0, class X>
RSE_FFT_FN void fft_c(int w, X& x) {
  if constexpr (H < FftSched<K>::W) {
    if (w == H) fft_phase_c<Ops, FftSched<K>::E, H, B1, FftSched<K>::LA - 1>(x);
    else fft_c<Ops, K, B1, H + 1>(w, x);
  }
}

// The 16-element kernel dispatches on the wave index once, around its whole
// column loop (f(FftConst<H>) for H = w: eight copies of the loop, none with a
// branch on the wave inside), because the register allocator spilled around
// per-phase branches with 128 registers of elements live across them.
template <int V>
struct FftConst {
  static constexpr int value = V;
};
template <int K, int H = 0, class F>
RSE_FFT_FN void fft_for_wave(int w, F&& f) {
  if constexpr (H < FftSched<K>::W) {
    if (w == H) f(FftConst<H>{});
    else fft_for_wave<K, H + 1>(w, f);
  }
}
// Its phase A by quarters: arrive(q) brings elements 4q .. 4q + 3 into the
// registers (the kernel: slices the quarter loaded last and issues the next
// quarter's loads, so that 4 elements' inputs are in flight at a time, not
// 16), and step q runs every level on the blocks of registers that quarter
// completes.
template <class Ops, int H, uint32_t B0, int Q, class X>
RSE_FFT_FN void fft_phase_a_step(X& x) {
  fft_phase_a<Ops, 16, H, B0, 0, 2, 4 * Q, 4 * Q + 4>(x);
  if constexpr (Q % 2 == 1) fft_phase_a<Ops, 16, H, B0, 2, 3, 4 * Q - 4, 4 * Q + 4>(x);
  if constexpr (Q == 3) fft_phase_a<Ops, 16, H, B0, 3, 4, 0, 16>(x);
}
template <class Ops, int K, int H, uint32_t B0, class X, class F>
RSE_FFT_FN void fft_phase_a_quarters(X& x, F&& arrive) {
  static_assert(FftSched<K>::E == 16 && FftSched<K>::LA == 4, "16 elements per wave");
  arrive(FftConst<0>{});
  fft_phase_a_step<Ops, H, B0, 0>(x);
  arrive(FftConst<1>{});
  fft_phase_a_step<Ops, H, B0, 1>(x);
  arrive(FftConst<2>{});
  fft_phase_a_step<Ops, H, B0, 2>(x);
  arrive(FftConst<3>{});
  fft_phase_a_step<Ops, H, B0, 3>(x);
}

}  // namespace
}  // namespace rse
