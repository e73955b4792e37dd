// rse_fft.hip -- GF(2^8) codecs with k = p = 2^m data and parity shards
// (the reference bench's 16+16, 32+32 and 64+64, benches/bandwidth.rs:88-190)
// coded with an additive FFT instead of k x p coefficient networks.
//
// Why it gives the reference's bytes.  ReedSolomon::new builds the systematic
// matrix M = V . V_top^-1 with V[r][c] = nth(r)^c and nth(r) = r
// (matrix.rs:263-276, core.rs:430-436, galois_8.rs:37-39).  So with P the
// unique polynomial of degree < k with P(i) = data_i for i < k, parity row j is
// P(k + j): M's rows are the evaluations of the interpolating polynomial.  For
// k = 2^m the points {0 .. k-1} are the F2-span U of {1, 2, .. 2^(m-1)} and
// {k .. 2k-1} = k ^ U is a coset of it.  The additive FFT of Lin, Chung and Han
// (novel polynomial basis X_j = prod over set bits i of j of s^_i, with
// s_i(x) = prod over a in span(1..2^(i-1)) of (x - a) and s^_i = s_i / s_i(2^i))
// evaluates a polynomial of degree < 2^m given in that basis on any coset
// beta ^ U in m 2^(m-1) butterflies
//     a ^= s^_i(beta ^ j) . b;   b ^= a
// (level i, block offset j), and its inverse interpolates.  Encode is the
// inverse transform on U (the data values -> P in the novel basis) followed
// by the forward transform on k ^ U (-> the parity values).  Rebuilding every
// data shard from the parity shards is the same map: Q(x) = P(x ^ k) has
// degree < k too and swaps the two cosets (i <-> k ^ i = k + i for i < k), so
// the k x k parity block is its own inverse and one kernel serves encode,
// verify and the rebuild (tests/test_fft_math.py checks the involution on the
// oracle's matrices).  The polynomial is unique, so the bytes are the
// reference's exactly (tests/test_fft_math.py checks the transform against the
// oracle's encode and reconstruct; tests/test_gpu_fft.py the kernels).
//
// Cost.  (k/2) log2 k butterflies per transform, each one constant multiply
// (an 8 x 8 bit matrix: a v_bitop3 XOR network over the bit-sliced planes)
// plus 8 XORs: 64+64 takes 384 multiplies per byte column against 4096 for
// the coefficient networks of the wide modules (rse_bitslice_core.hpp), and
// the zero twiddles of the transform on U (the first block of every level) are
// free.
//
// Kernel.  A workgroup of k/8 waves codes one 2 KiB column of every shard at a
// time (lane l: bytes 16 l and 1024 + 16 l, one 8-plane group, as
// wide_body_half; 1 KiB shards: two stripes per column).  Element e (a shard)
// lives in the registers of one wave as 8 planes:
//   phase A: wave h holds elements 8h .. 8h+7 (its own loads) and runs the
//            inverse transform's levels 0-2 (twiddles per wave);
//   phase B: through LDS, wave w holds the groups of elements with the same
//            low three bits (8 / (k/8) groups of k/8) and runs the levels >= 3
//            of the inverse transform, then of the forward one (twiddles equal
//            for every wave: they depend only on the bits >= 3);
//   phase C: back through LDS, wave h holds elements 8h .. 8h+7 again and runs
//            the forward transform's levels 2-0, then un-slices and stores (or
//            compares) its 8 outputs.
// Every wave writes its phase-B results into the LDS slots it read them from,
// and its phase-A results into the slots it read in phase C, so a column
// needs two workgroup barriers.  The next column's loads are issued before
// phase A.  LDS: k x 2 KiB (64+64: 128 KiB, one workgroup per CU).
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <vector>

#include "rse_bitslice_core.hpp"
#include "rse_field.hpp"
#include "rse_fft.hpp"
#include "rse_fft_sched.hpp"
#include "rse_options.hpp"

namespace rse {
namespace {

template <uint32_t C, int... Q>
__device__ __forceinline__ void fft_mul_add(uint32_t (&a)[8], const uint32_t (&b)[8],
                                            int_seq<int, Q...>) {
  ((a[Q] = xacc<fft_row(C, Q)>(a[Q], b)), ...);
}
// forward butterfly: a ^= C b; b ^= a.  Inverse: b ^= a; a ^= C b.
template <uint32_t C, bool INV>
__device__ __forceinline__ void fft_bfly(uint32_t (&a)[8], uint32_t (&b)[8]) {
  if constexpr (INV) {
#pragma unroll
    for (int q = 0; q < 8; ++q) b[q] ^= a[q];
    fft_mul_add<C>(a, b, make_int_seq<8>{});
  } else {
    fft_mul_add<C>(a, b, make_int_seq<8>{});
#pragma unroll
    for (int q = 0; q < 8; ++q) b[q] ^= a[q];
  }
}

// The butterflies of the kernels for rse_fft_sched.hpp: an element is 8 planes.
struct PlaneOps {
  template <int I, int J, uint32_t C, bool INV>
  static __device__ __forceinline__ void bfly(uint32_t (&a)[8], uint32_t (&b)[8]) {
    fft_bfly<C, INV>(a, b);
  }
};

// A workgroup's columns: column c's byte offset for this lane, the stripe it
// belongs to, and whether that stripe exists (SUB: the last column of an odd
// stripe count loads its last stripe twice and stores it once).
template <uint32_t SUB>
struct FftCols {
  static constexpr uint32_t S = SUB ? SUB / 2u : 1024u;  // a lane's two vectors, S apart
  static constexpr uint32_t SPC = 2048u / (SUB ? SUB : 2048u), LPS = 64u / SPC;  // stripes / column, lanes / stripe
  uint64_t cols, total, stripe_stride;
  uint32_t n_stripes, lane, lane_off;
  template <class A>
  __device__ __forceinline__ FftCols(const A& a)
      : cols(a.cols_per_stripe),
        total(SUB ? ((uint64_t)a.n_stripes + SPC - 1) / SPC : a.cols_per_stripe * a.n_stripes),
        stripe_stride(a.stripe_stride),
        n_stripes(a.n_stripes),
        lane(threadIdx.x & 63u),
        lane_off((SUB ? (threadIdx.x & 63u) % LPS : (threadIdx.x & 63u)) * 16u) {}
  __device__ __forceinline__ uint64_t stripe(uint64_t c) const {
    return SUB ? c * SPC + lane / LPS : c / cols;
  }
  __device__ __forceinline__ bool ok(uint64_t c) const { return SUB == 0 || stripe(c) < n_stripes; }
  __device__ __forceinline__ uint64_t off(uint64_t c) const {
    if constexpr (SUB) {
      uint64_t s = stripe(c);
      if (s >= n_stripes) s = n_stripes - 1;  // loaded, never stored
      return s * stripe_stride + lane_off;
    }
    const uint64_t s = c / cols;
    return s * stripe_stride + (c - s * cols) * 2048u + lane_off;
  }
};

// A wave's outputs T0 .. T1-1 of its E of column c (elements e0 ..): un-sliced,
// then stored and / or compared by mode.  True when a compared vector differs.
template <int E, uint32_t SUB, int T0 = 0, int T1 = E, class A>
__device__ __forceinline__ bool fft_emit(const A& a, const FftCols<SUB>& fc, uint32_t (&x)[E][8],
                                         int e0, uint64_t off, bool ok, uint32_t mode) {
  bool d = false;
#pragma unroll
  for (int t = T0; t < T1; ++t) {
    u32x4 v[2];
    unslice8(x[t], v);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const uint64_t o16 = off + j * FftCols<SUB>::S;
      if (mode != kCheck && ok) stv<true>(a.out[e0 + t] + o16, v[j]);
      if (mode != kStore) {
        const u32x4 q = ldv<true>(a.cmp[e0 + t] + o16);
        d |= ok & ((q.x != v[j].x) | (q.y != v[j].y) | (q.z != v[j].z) | (q.w != v[j].w));
      }
    }
  }
  return d;
}

// LDS: element e's 8 planes, as two quads of planes per lane.
template <int K>
using FftPlanes = uint4[K][2][64];

__device__ __forceinline__ void fft_put(uint4 (&slot)[2][64], const uint32_t (&x)[8], uint32_t lane) {
  slot[0][lane] = make_uint4(x[0], x[1], x[2], x[3]);
  slot[1][lane] = make_uint4(x[4], x[5], x[6], x[7]);
}
__device__ __forceinline__ void fft_get(const uint4 (&slot)[2][64], uint32_t (&x)[8], uint32_t lane) {
  const uint4 a = slot[0][lane], b = slot[1][lane];
  x[0] = a.x;
  x[1] = a.y;
  x[2] = a.z;
  x[3] = a.w;
  x[4] = b.x;
  x[5] = b.y;
  x[6] = b.z;
  x[7] = b.w;
}

// The kernel of K = k = p <= 64: B0 / B1 the cosets of the inputs / outputs
// (0 / K: the parity rows, which are also their inverse), SUB 1024 for 1 KiB
// shards (two stripes per 2 KiB column), else 0 (whole 2 KiB columns).
template <int K, uint32_t B0, uint32_t B1, uint32_t SUB>
__global__ __launch_bounds__(K * 8) void fft_kernel(const FftArgs<K> a) {
  static_assert(K == 16 || K == 32 || K == 64, "k = p = 16, 32 or 64");
  using SC = FftSched<K>;
  static_assert(SC::E == 8 && SC::W * 64 == K * 8, "8 elements per wave");
  __shared__ FftPlanes<K> st;
  constexpr uint32_t S = FftCols<SUB>::S;
  const int w = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const FftCols<SUB> fc(a);
  const uint32_t lane = fc.lane;
  const uint64_t total = fc.total;
  const uint32_t mode = a.mode;
  const uint8_t* const* in = a.in + 8 * w;
  u32x4 buf[8][2];
  if (blockIdx.x < total) {
    const uint64_t off0 = fc.off(blockIdx.x);
#pragma unroll
    for (int t = 0; t < 8; ++t) load2<S>(buf[t], in[t] + off0);
  }
  bool diff = false;
  for (uint64_t c = blockIdx.x; c < total; c += gridDim.x) {
    const uint64_t off = fc.off(c);
    const uint64_t next = c + gridDim.x;
    uint32_t x[8][8];
#pragma unroll
    for (int t = 0; t < 8; ++t) slice8(buf[t], x[t]);
    if (next < total) {  // the next column's inputs in flight through the transform
      const uint64_t noff = fc.off(next);
#pragma unroll
      for (int t = 0; t < 8; ++t) load2<S>(buf[t], in[t] + noff);
    }
    // phase A, then its results into the slots this wave read in phase C
    fft_a<PlaneOps, K, B0, 0, SC::LA, 0, 8>(w, x);
#pragma unroll
    for (int t = 0; t < 8; ++t) fft_put(st[SC::ac_slot(w, t)], x[t], lane);
    __syncthreads();
    // phase B on this wave's groups (the same slots written back)
#pragma unroll
    for (int r = 0; r < 8; ++r) fft_get(st[SC::b_slot(w, r)], x[r], lane);
    fft_phase_b<PlaneOps, K, B0, B1>(x);
#pragma unroll
    for (int r = 0; r < 8; ++r) fft_put(st[SC::b_slot(w, r)], x[r], lane);
    __syncthreads();
    // phase C on this wave's own elements, then its 8 outputs
#pragma unroll
    for (int t = 0; t < 8; ++t) fft_get(st[SC::ac_slot(w, t)], x[t], lane);
    fft_c<PlaneOps, K, B1>(w, x);
    const bool d = fft_emit<8, SUB>(a, fc, x, 8 * w, off, fc.ok(c), mode);
    if (a.per_stripe) {
      if (d) flag_mismatch(a.mismatch + fc.stripe(c));
    } else {
      diff |= d;
    }
  }
  if (mode != kStore && diff) flag_mismatch(a.mismatch);
}

// The kernel of K = k = p = 128: 8 waves of 16 elements (x[16][8]: 128 VGPRs,
// two waves per SIMD).  128 elements x 2 KiB do not fit a CU's 160 KiB of LDS,
// so each of the two exchanges goes one quad of planes at a time through
// 128 elements x 4 planes x 64 lanes x 4 B = 128 KiB: a wave puts planes 0-3
// of its registers, takes planes 0-3 of the other phase's elements into the
// registers just freed, and then the same for planes 4-7.  A wave puts its
// phase-B results into the slots it took them from and its phase-A results
// into the slots it takes in phase C, so only the puts of planes 4-7 have to
// wait for the other waves' takes of planes 0-3: six barriers per column.
// The next column's 16 inputs would be another 128 VGPRs, so the inputs arrive
// by quarters (rse_fft_sched.hpp fft_phase_a_quarters): four elements in
// flight while phase A runs on the ones before, the next column's first four
// while the last twelve outputs are un-sliced and stored (in flight through
// the whole transform they cost 32 VGPRs the kernel does not have).  Wave H's whole column loop is its own copy of the
// code (fft_for_wave in the kernel): with the wave's branch inside the loop,
// around phases A and C as in fft_kernel, the register allocator spilled 400+
// bytes per lane around the branches.
using FftQuads = uint32_t[128][4][64];  // a quad of planes of element e: [plane][lane]

template <int K, uint32_t B0, uint32_t B1, uint32_t SUB, int H>
__device__ __forceinline__ void fft_quads_wave(const FftArgs<K>& a, FftQuads& st) {
  using SC = FftSched<K>;
  constexpr int E = SC::E, QN = E / 4;
  constexpr uint32_t S = FftCols<SUB>::S;
  const FftCols<SUB> fc(a);
  const uint32_t lane = fc.lane;
  const uint64_t total = fc.total;
  const uint32_t mode = a.mode;
  const uint8_t* const* in = a.in + E * H;
  u32x4 buf[QN][2];
  if (blockIdx.x < total) {
    const uint64_t off0 = fc.off(blockIdx.x);
#pragma unroll
    for (int t = 0; t < QN; ++t) load2<S>(buf[t], in[t] + off0);
  }
  // planes 4 Q .. 4 Q + 3 of the wave's registers to / from its slots
  auto put = [&](uint32_t (&x)[E][8], auto q, auto phase_b) {
    constexpr int Q = decltype(q)::value;
#pragma unroll
    for (int r = 0; r < E; ++r)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        st[decltype(phase_b)::value ? SC::b_slot(H, r) : SC::ac_slot(H, r)][j][lane] = x[r][4 * Q + j];
  };
  auto take = [&](uint32_t (&x)[E][8], auto q, auto phase_b) {
    constexpr int Q = decltype(q)::value;
#pragma unroll
    for (int r = 0; r < E; ++r)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        x[r][4 * Q + j] = st[decltype(phase_b)::value ? SC::b_slot(H, r) : SC::ac_slot(H, r)][j][lane];
  };
  using Q0 = FftConst<0>;
  using Q1 = FftConst<1>;
  using AC = FftConst<0>;
  using B = FftConst<1>;
  bool diff = false;
  for (uint64_t c = blockIdx.x; c < total; c += gridDim.x) {
    const uint64_t off = fc.off(c);
    const uint64_t next = c + gridDim.x;
    uint32_t x[E][8];
    // phase A, a quarter of the inputs in flight at a time
    fft_phase_a_quarters<PlaneOps, K, H, B0>(x, [&](auto q) {
      constexpr int Q = decltype(q)::value;
      // (the scheduler otherwise issues all sixteen loads at once: 96 more VGPRs)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < QN; ++t) slice8(buf[t], x[QN * Q + t]);
      if constexpr (Q < 3) {
#pragma unroll
        for (int t = 0; t < QN; ++t) load2<S>(buf[t], in[QN * (Q + 1) + t] + off);
      }
      __builtin_amdgcn_sched_barrier(0);
    });
    // to this wave's phase-B groups
    put(x, Q0{}, AC{});
    __syncthreads();
    take(x, Q0{}, B{});
    __syncthreads();
    put(x, Q1{}, AC{});
    __syncthreads();
    take(x, Q1{}, B{});
    fft_phase_b<PlaneOps, K, B0, B1>(x);
    // and back to its own elements
    put(x, Q0{}, B{});
    __syncthreads();
    take(x, Q0{}, AC{});
    __syncthreads();
    put(x, Q1{}, B{});
    __syncthreads();
    take(x, Q1{}, AC{});
    fft_phase_c<PlaneOps, E, H, B1, SC::LA - 1>(x);
    // the first outputs free the registers of the next column's first inputs
    __builtin_amdgcn_sched_barrier(0);
    bool d = fft_emit<E, SUB, 0, QN>(a, fc, x, E * H, off, fc.ok(c), mode);
    if (next < total) {
      const uint64_t noff = fc.off(next);
#pragma unroll
      for (int t = 0; t < QN; ++t) load2<S>(buf[t], in[t] + noff);
    }
    d |= fft_emit<E, SUB, QN, E>(a, fc, x, E * H, off, fc.ok(c), mode);
    if (a.per_stripe) {
      if (d) flag_mismatch(a.mismatch + fc.stripe(c));
    } else {
      diff |= d;
    }
  }
  if (mode != kStore && diff) flag_mismatch(a.mismatch);
}

template <int K, uint32_t B0, uint32_t B1, uint32_t SUB>
__global__ __launch_bounds__(512) void fft_kernel_quads(const FftArgs<K> a) {
  static_assert(K == 128, "k = p = 128");
  using SC = FftSched<K>;
  static_assert(SC::E == 16 && SC::W == 8 && SC::LA == 4, "8 waves of 16 elements");
  static_assert(sizeof(FftQuads) == sizeof(uint32_t) * K * 4 * 64 && sizeof(FftQuads) <= 160 * 1024, "LDS");
  __shared__ FftQuads st;
  const int w = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  fft_for_wave<K>(w, [&](auto h) { fft_quads_wave<K, B0, B1, SUB, decltype(h)::value>(a, st); });
}

// ------------------------------------------------------------------- host
// The rows the kernels replace: the K+K codec's parity rows (encode, verify;
// their own inverse, so also every data shard rebuilt from the parity shards
// in parity order: reconstruct with shards 0 .. K-1 missing, core.rs:801-923).
// Built on K's first use: a 16+16 caller does not pay for the 128 x 128
// inversion.
template <size_t K>
const std::vector<uint16_t>& fft_rows() {
  static const std::vector<uint16_t> r = [] {
    const Matrix<Gf8Field> v = Matrix<Gf8Field>::vandermonde(2 * K, K);
    Matrix<Gf8Field> top(K, K), inv;
    for (size_t i = 0; i < K; ++i)
      for (size_t j = 0; j < K; ++j) top.at(i, j) = v.at(i, j);
    top.invert(inv);
    const Matrix<Gf8Field> m = v.multiply(inv);  // core.rs:430-436
    return std::vector<uint16_t>(m.d.begin() + K * K, m.d.begin() + 2 * K * K);
  }();
  return r;
}

// The kernel of K (its workgroup: FftSched<K>::W waves) and its arguments.
template <int K>
const void* fft_fn(uint32_t sub) {
  if constexpr (K == 128)
    return sub ? reinterpret_cast<const void*>(&fft_kernel_quads<K, 0u, K, 1024u>)
               : reinterpret_cast<const void*>(&fft_kernel_quads<K, 0u, K, 0u>);
  else
    return sub ? reinterpret_cast<const void*>(&fft_kernel<K, 0u, K, 1024u>)
               : reinterpret_cast<const void*>(&fft_kernel<K, 0u, K, 0u>);
}
struct FftLaunch {
  uint64_t stripe_stride, cols;
  uint32_t* mismatch;
  uint32_t n_stripes, mode, per_stripe, sub;
  const uint8_t* const* in;
  uint8_t* const* out;
  const uint8_t* const* cmp;
  hipStream_t stream;
};
template <int K>
hipError_t fft_launch(const FftLaunch& l) {
  FftArgs<K> a;
  std::memset(&a, 0, sizeof a);
  a.stripe_stride = l.stripe_stride;
  a.cols_per_stripe = l.cols;
  a.mismatch = l.mismatch;
  a.n_stripes = l.n_stripes;
  a.mode = l.mode;
  a.per_stripe = l.per_stripe;
  for (int i = 0; i < K; ++i) {
    a.in[i] = l.in[i];
    a.out[i] = l.out ? l.out[i] : nullptr;
    a.cmp[i] = l.cmp ? l.cmp[i] : nullptr;
  }
  const void* fn = fft_fn<K>(l.sub);
  constexpr uint32_t threads = FftSched<K>::W * 64u;
  const uint64_t total = l.sub ? ((uint64_t)l.n_stripes + 1) / 2 : l.cols * l.n_stripes;
  // resident workgroups (LDS: k x 2 KiB each, 128+128: 128 KiB), a few rounds of them
  int dev = 0, n_cu = 0, per = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);
  if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, fn, threads, 0);
  if (e != hipSuccess) return e;
  const int64_t grid_opt = get_option(RSE_OPT_GRID_X);
  uint64_t gx = grid_opt > 0 ? (uint64_t)grid_opt : (uint64_t)std::max(per, 1) * (uint64_t)n_cu;
  if (gx > total) gx = total;
  if (gx > 0x7fffffffu) gx = 0x7fffffffu;
  void* args[] = {&a};
  return hipLaunchKernel(fn, dim3((uint32_t)gx), dim3(threads), args, 0, l.stream);
}

}  // namespace

bool fft_applies(int field, uint32_t k, uint32_t p, const uint16_t* rows) {
  const int64_t opt = get_option(RSE_OPT_FFT);
  if (field != 8 || k != p || !opt) return false;
  const std::vector<uint16_t>* par = nullptr;
  switch (k) {
    case 16: par = &fft_rows<16>(); break;
    case 32: par = &fft_rows<32>(); break;
    case 64: par = &fft_rows<64>(); break;
    case 128:
      if (opt < 2) return false;
      par = &fft_rows<128>();
      break;
    default: return false;
  }
  return std::memcmp(rows, par->data(), (size_t)k * k * sizeof(uint16_t)) == 0;
}

hipError_t launch_fft(int field, uint32_t k, uint32_t p, const uint16_t* rows,
                      const uint8_t* const* in, uint8_t* const* out, const uint8_t* const* cmp,
                      uint64_t len, uint64_t stripe_stride, uint32_t n_stripes, uint32_t mode,
                      uint32_t* mismatch, bool per_stripe, hipStream_t stream, uint64_t* done) {
  *done = 0;
  if (!fft_applies(field, k, p, rows) || n_stripes == 0) return hipSuccess;
  // 1 KiB shards: two stripes per 2 KiB column; otherwise whole 2 KiB columns
  const uint32_t sub = len == 1024u && get_option(RSE_OPT_SUB_CHUNKS) != 0 ? 1024u : 0u;
  const uint64_t cols = len / 2048u;
  if (!sub && cols == 0) return hipSuccess;
  const FftLaunch l{stripe_stride, cols, mismatch, n_stripes, mode, per_stripe ? 1u : 0u, sub,
                    in, out, cmp, stream};
  hipError_t e = hipSuccess;
  switch (k) {
    case 16: e = fft_launch<16>(l); break;
    case 32: e = fft_launch<32>(l); break;
    case 64: e = fft_launch<64>(l); break;
    case 128: e = fft_launch<128>(l); break;
    default: return hipSuccess;
  }
  if (e != hipSuccess) return e;
  note_kernel("fft gf8 %u+%u %s%s", k, p, mode == kStore ? "code" : "check", sub ? " sub1" : "");
  count_bitslice_launch();
  *done = sub ? len : cols * 2048u;
  return hipSuccess;
}

}  // namespace rse
