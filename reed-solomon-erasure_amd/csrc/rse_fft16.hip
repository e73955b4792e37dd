// rse_fft16.hip -- GF(2^16) codecs past 256 shards (k + p > 256: coefficients
// outside the GF(2^8) subfield) with u = 2^m - k <= 32, n = 2^m the smallest
// power of two >= k + p: encode, verify and reconstruct on one compiled
// kernel with data-only tables, opt-in with RSE_OPT_FFT16.  The algebra and
// the tables: rse_fft16_plan.hpp.
//
// Per 4 KiB column of every shard (64 lanes x 64 B, 16 planes of 32 elements:
// the GF(2^16) slicing of rse_bitslice_core.hpp) the kernel
//   1. runs the pruned inverse transform: for each of the n/32 blocks of 32
//      consecutive points, the block's 5-level inverse transform (80
//      butterflies, twiddles s^_i(32 blk ^ j)), XORed into 32 accumulated
//      elements.  A shard with a null pointer is zero (padding points, and
//      every point outside the k valid ones);
//   2. applies the call's rows to the top u accumulated elements
//      (encode / verify: the first p rows of A^-1; reconstruct: the rows of
//      A_U^-1 of the lost shards), un-slices and stores or compares.
// 1000+24: 32 x 80 + 24 x 24 = 3,136 constant multiplies per element column
// against 24,000 for the coefficient networks.
//
// Twiddles and rows are run-time data, uniform per wave, each a 16 x 16 bit
// matrix (16 halfwords, fft16_bit_matrix) read with scalar loads: a multiply
// is 256 and-xor steps, the 0 / -1 masks from scalar bit-field extracts.  So
// one kernel serves every such codec and every pattern.
//
// Workgroup: 8 waves of 4 elements (x[4][16] and the accumulators: 128 VGPRs).
//   phase 1: wave w holds elements 4w .. 4w+3 (its own loads), levels 0-1;
//   phase 2: through LDS, wave a + 4c holds a + 4t + 16c (t < 4), levels 2-3,
//            written back to the slots it read;
//   phase 3: wave a + 4b holds a + 4(2b + (t & 1)) + 16(t >> 1), level 4, and
//            accumulates in this layout.
// Three barriers per block (the third: phase 3's reads before the next
// block's writes); the next block's four loads are issued before the block's
// butterflies.  After the last block the accumulators go to LDS and wave w
// codes rows w, w + 8, .. from them: no workspace and no second kernel, the
// kernel reads every valid shard and writes every row once.  LDS: 32 elements
// x 4 KiB = 128 KiB, one workgroup per CU, two waves per SIMD (231 VGPRs, no
// scratch).  Measurements and the limiter: DESIGN.md section 4.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "rse_bitslice_core.hpp"
#include "rse_fft16.hpp"
#include "rse_options.hpp"

namespace rse {
namespace {

// Uniform tables (twiddles, rows, shard pointers) are read through the
// constant address space: nothing writes them while the kernel runs, and the
// loads become scalar loads whatever the kernel stores in between.
template <class T>
using cptr = __attribute__((address_space(4))) const T*;

struct Fft16Args {
  const uint64_t* in;    // n shard pointers of stripe 0 (0: a zero shard)
  const uint64_t* out;   // n_rows output pointers (store modes)
  const uint64_t* cmp;   // n_rows compare pointers (check modes)
  const uint32_t* tw;    // [nblk][32 twiddles][8 dwords]
  const uint32_t* mat;   // [n_rows][u][8 dwords]
  uint32_t* mismatch;
  uint64_t stripe_stride, cols_per_stripe, total;
  uint32_t nblk, u, n_rows, mode, per_stripe;
};

using Fft16Lds = uint4[kFft16Block][4][64];  // element, quad of planes, lane
static_assert(sizeof(Fft16Lds) == 128 * 1024, "LDS");

__device__ __forceinline__ void put16(uint4 (&slot)[4][64], const uint32_t (&x)[16], uint32_t lane) {
#pragma unroll
  for (int q = 0; q < 4; ++q)
    slot[q][lane] = make_uint4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
}
__device__ __forceinline__ void get16(const uint4 (&slot)[4][64], uint32_t (&x)[16], uint32_t lane) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint4 v = slot[q][lane];
    x[4 * q] = v.x;
    x[4 * q + 1] = v.y;
    x[4 * q + 2] = v.z;
    x[4 * q + 3] = v.w;
  }
}

// y ^ (b & m), m a wave-uniform 0 / -1 mask: one v_bitop3_b32 (truth table
// (S0 & S1) ^ S2).  Written out as bfi is (rse_bitslice_core.hpp): from the C
// form the compiler emits a v_and and a v_xor per step.
__device__ __forceinline__ uint32_t and_xor(uint32_t m, uint32_t b, uint32_t y) {
  uint32_t r;
  asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x6a" : "=v"(r) : "s"(m), "v"(b), "v"(y));
  return r;
}

// y ^= T . b: m = T's bit matrix, halfword r the row of output plane r.
__device__ __forceinline__ void mul_acc16(uint32_t (&y)[16], const uint32_t (&b)[16],
                                          cptr<uint32_t> m) {
#pragma unroll
  for (int h = 0; h < 8; ++h) {
    const uint32_t w = m[h];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      y[2 * h] = and_xor((uint32_t)((int32_t)(w << (31 - c)) >> 31), b[c], y[2 * h]);
      y[2 * h + 1] = and_xor((uint32_t)((int32_t)(w << (15 - c)) >> 31), b[c], y[2 * h + 1]);
    }
  }
}

// Inverse butterfly: hi ^= lo; lo ^= T . hi.
__device__ __forceinline__ void bfly16(uint32_t (&lo)[16], uint32_t (&hi)[16], cptr<uint32_t> t) {
#pragma unroll
  for (int q = 0; q < 16; ++q) hi[q] ^= lo[q];
  mul_acc16(lo, hi, t);
}
// Two butterflies with one twiddle, each mask made once and used at once for
// both (as two bfly16 calls the compiler keeps the first one's 256 masks for
// the second: some 500 scalar registers spilled to lanes and read back).
__device__ __forceinline__ void bfly16x2(uint32_t (&lo0)[16], uint32_t (&hi0)[16],
                                         uint32_t (&lo1)[16], uint32_t (&hi1)[16],
                                         cptr<uint32_t> t) {
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    hi0[q] ^= lo0[q];
    hi1[q] ^= lo1[q];
  }
#pragma unroll
  for (int h = 0; h < 8; ++h) {
    const uint32_t w = t[h];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const uint32_t m0 = (uint32_t)((int32_t)(w << (31 - c)) >> 31);
      const uint32_t m1 = (uint32_t)((int32_t)(w << (15 - c)) >> 31);
      lo0[2 * h] = and_xor(m0, hi0[c], lo0[2 * h]);
      lo1[2 * h] = and_xor(m0, hi1[c], lo1[2 * h]);
      lo0[2 * h + 1] = and_xor(m1, hi0[c], lo0[2 * h + 1]);
      lo1[2 * h + 1] = and_xor(m1, hi1[c], lo1[2 * h + 1]);
    }
  }
}

__global__ __launch_bounds__(512) void fft16_kernel(const Fft16Args a) {
  __shared__ Fft16Lds st;
  const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63u;
  const cptr<uint64_t> in = (cptr<uint64_t>)a.in;
  const cptr<uint64_t> outp = (cptr<uint64_t>)a.out;
  const cptr<uint64_t> cmpp = (cptr<uint64_t>)a.cmp;
  const cptr<uint32_t> tw = (cptr<uint32_t>)a.tw;
  const cptr<uint32_t> mat = (cptr<uint32_t>)a.mat;
  const uint32_t mode = a.mode;
  const uint32_t wa = w & 3u, wh = w >> 2;  // phases 2 and 3: a, and c / b
  bool diff = false;
  for (uint64_t col = blockIdx.x; col < a.total; col += gridDim.x) {
    const uint64_t s = col / a.cols_per_stripe;
    const uint64_t off = s * a.stripe_stride + (col - s * a.cols_per_stripe) * 4096u + lane * 16u;
    uint32_t acc[4][16];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[t][q] = 0;
    // this wave's four inputs of block 0 in flight
    u32x4 buf[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (const uint64_t p = in[4u * w + t])
        load4<true, 1024u>(buf[t], reinterpret_cast<const uint8_t*>(p) + off);
    for (uint32_t blk = 0; blk < a.nblk; ++blk) {
      const cptr<uint32_t> tb = tw + (size_t)blk * (kFft16Block * 8u);
      uint32_t x[4][16];
      // phase 1: elements 4w + t
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (in[blk * kFft16Block + 4u * w + t]) {
          slice<BitsF16>(buf[t], x[t]);
        } else {
#pragma unroll
          for (int q = 0; q < 16; ++q) x[t][q] = 0;
        }
      }
      // the next block's inputs in flight through this block's butterflies
      if (blk + 1u < a.nblk) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (const uint64_t p = in[(blk + 1u) * kFft16Block + 4u * w + t])
            load4<true, 1024u>(buf[t], reinterpret_cast<const uint8_t*>(p) + off);
      }
      bfly16(x[0], x[1], tb + 8u * fft16_tw_index(0, 2u * w));
      bfly16(x[2], x[3], tb + 8u * fft16_tw_index(0, 2u * w + 1u));
      bfly16x2(x[0], x[2], x[1], x[3], tb + 8u * fft16_tw_index(1, w));
#pragma unroll
      for (int t = 0; t < 4; ++t) put16(st[4u * w + t], x[t], lane);
      __syncthreads();
      // phase 2: elements a + 4t + 16c
#pragma unroll
      for (int t = 0; t < 4; ++t) get16(st[wa + 4u * t + 16u * wh], x[t], lane);
      bfly16(x[0], x[1], tb + 8u * fft16_tw_index(2, 2u * wh));
      bfly16(x[2], x[3], tb + 8u * fft16_tw_index(2, 2u * wh + 1u));
      bfly16x2(x[0], x[2], x[1], x[3], tb + 8u * fft16_tw_index(3, wh));
#pragma unroll
      for (int t = 0; t < 4; ++t) put16(st[wa + 4u * t + 16u * wh], x[t], lane);
      __syncthreads();
      // phase 3: elements a + 4(2b + (t & 1)) + 16(t >> 1)
#pragma unroll
      for (int t = 0; t < 4; ++t)
        get16(st[wa + 4u * (2u * wh + (t & 1)) + 16u * (t >> 1)], x[t], lane);
      bfly16x2(x[0], x[2], x[1], x[3], tb + 8u * fft16_tw_index(4, 0));
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[t][q] ^= x[t][q];
      __syncthreads();
    }
    // the accumulated elements to LDS, then this wave's rows
#pragma unroll
    for (int t = 0; t < 4; ++t)
      put16(st[wa + 4u * (2u * wh + (t & 1)) + 16u * (t >> 1)], acc[t], lane);
    __syncthreads();
    bool d = false;
    for (uint32_t r = w; r < a.n_rows; r += 8u) {
      uint32_t y[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) y[q] = 0;
      for (uint32_t c = 0; c < a.u; ++c) {
        uint32_t b[16];
        get16(st[kFft16Block - a.u + c], b, lane);
        mul_acc16(y, b, mat + ((size_t)r * a.u + c) * 8u);
      }
      u32x4 v[4];
      unslice<BitsF16>(y, v);
      if (mode != kCheck) {
        uint8_t* o = reinterpret_cast<uint8_t*>(outp[r]) + off;
#pragma unroll
        for (int j = 0; j < 4; ++j) stv<true>(o + j * 1024u, v[j]);
      }
      if (mode != kStore) {
        const uint8_t* o = reinterpret_cast<const uint8_t*>(cmpp[r]) + off;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const u32x4 q = ldv<true>(o + j * 1024u);
          d |= (q.x != v[j].x) | (q.y != v[j].y) | (q.z != v[j].z) | (q.w != v[j].w);
        }
      }
    }
    if (a.per_stripe) {
      if (d) flag_mismatch(a.mismatch + s);
    } else {
      diff |= d;
    }
    __syncthreads();  // the rows' reads before the next column's writes
  }
  if (mode != kStore && diff) flag_mismatch(a.mismatch);
}

// ------------------------------------------------------------------- host
// A codec shape's plan and, per device, its twiddles as bit matrices.
struct Fft16Entry {
  Fft16Plan plan;
  bool ok = false;
  std::vector<uint32_t> enc_bits;  // plan.enc as bit matrices, 8 dwords each
  static constexpr int kDevs = 64;
  std::atomic<uint32_t*> tw_dev[kDevs] = {};
};

void pack_bit_matrix(uint16_t t, uint32_t* dst) {
  uint16_t rows[16];
  fft16_bit_matrix(t, rows);
  for (int h = 0; h < 8; ++h) dst[h] = (uint32_t)rows[2 * h] | ((uint32_t)rows[2 * h + 1] << 16);
}

Fft16Entry* fft16_entry(uint32_t k, uint32_t p) {
  static std::mutex mu;
  static std::map<std::pair<uint32_t, uint32_t>, std::unique_ptr<Fft16Entry>> plans;
  std::lock_guard<std::mutex> g(mu);
  auto& e = plans[{k, p}];
  if (!e) {
    e.reset(new Fft16Entry);
    e->ok = fft16_make_plan(k, p, e->plan);
    e->enc_bits.resize(e->plan.enc.size() * 8u);
    for (size_t i = 0; i < e->plan.enc.size(); ++i) pack_bit_matrix(e->plan.enc[i], &e->enc_bits[i * 8u]);
  }
  return e->ok ? e.get() : nullptr;
}

// Made once per device with a synchronous copy; two threads racing keep one.
hipError_t fft16_twiddles(Fft16Entry* e, const uint32_t** out) {
  int dev = 0;
  hipError_t he = hipGetDevice(&dev);
  if (he != hipSuccess) return he;
  if (dev < 0 || dev >= Fft16Entry::kDevs) return hipErrorInvalidDevice;
  if (uint32_t* q = e->tw_dev[dev].load(std::memory_order_acquire)) {
    *out = q;
    return hipSuccess;
  }
  std::vector<uint32_t> h(e->plan.tw.size() * 8u);
  for (size_t i = 0; i < e->plan.tw.size(); ++i) pack_bit_matrix(e->plan.tw[i], &h[i * 8u]);
  uint32_t* q = nullptr;
  he = hipMalloc(reinterpret_cast<void**>(&q), h.size() * sizeof(uint32_t));
  if (he == hipSuccess) he = hipMemcpy(q, h.data(), h.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (he != hipSuccess) {
    if (q) (void)hipFree(q);
    return he;
  }
  uint32_t* expect = nullptr;
  if (!e->tw_dev[dev].compare_exchange_strong(expect, q, std::memory_order_acq_rel)) {
    (void)hipFree(q);
    q = expect;
  }
  *out = q;
  return hipSuccess;
}

}  // namespace

const Fft16Plan* fft16_plan(int field, uint32_t k, uint32_t p) {
  if (field != 16 || !get_option(RSE_OPT_FFT16) || !fft16_shape(k, p, nullptr, nullptr))
    return nullptr;
  Fft16Entry* e = fft16_entry(k, p);
  return e ? &e->plan : nullptr;
}

bool fft16_applies(int field, uint32_t k, uint32_t p, const uint16_t* rows) {
  const Fft16Plan* pl = fft16_plan(field, k, p);
  return pl && std::memcmp(rows, pl->rows.data(), pl->rows.size() * sizeof(uint16_t)) == 0;
}

hipError_t launch_fft16(const Fft16Plan& pl, const uint8_t* const* in, uint32_t n_rows,
                        const uint16_t* mat, uint8_t* const* out, const uint8_t* const* cmp,
                        uint64_t len, uint64_t stripe_stride, uint32_t n_stripes, uint32_t mode,
                        uint32_t* mismatch, bool per_stripe, const char* what, hipStream_t stream,
                        uint64_t* done) {
  *done = 0;
  const uint64_t cols = len / 4096u;
  Fft16Entry* e = fft16_entry(pl.k, pl.p);
  if (!e || cols == 0 || n_stripes == 0 || n_rows == 0 || n_rows > kFft16Block) return hipSuccess;
  const uint32_t* tw = nullptr;
  hipError_t he = fft16_twiddles(e, &tw);
  if (he != hipSuccess) return he;
  // the call's tables in one block: n input pointers, n_rows output and
  // compare pointers, the rows as bit matrices
  const size_t n = pl.n, words = n + 2u * n_rows + (size_t)n_rows * pl.u * 4u;
  static thread_local std::vector<uint64_t> h;
  h.assign(words, 0);
  for (size_t i = 0; i < n; ++i) h[i] = reinterpret_cast<uint64_t>(in[i]);
  for (uint32_t r = 0; r < n_rows; ++r) {
    h[n + r] = out ? reinterpret_cast<uint64_t>(out[r]) : 0;
    h[n + n_rows + r] = cmp ? reinterpret_cast<uint64_t>(cmp[r]) : 0;
  }
  uint32_t* hm = reinterpret_cast<uint32_t*>(h.data() + n + 2u * n_rows);
  if (mat == pl.enc.data() && n_rows == pl.p)  // the codec's own rows: packed with the plan
    std::memcpy(hm, e->enc_bits.data(), e->enc_bits.size() * sizeof(uint32_t));
  else
    for (size_t i = 0; i < (size_t)n_rows * pl.u; ++i) pack_bit_matrix(mat[i], hm + i * 8u);
  uint64_t* d = nullptr;
  he = hipMallocAsync(reinterpret_cast<void**>(&d), words * sizeof(uint64_t), stream);
  if (he != hipSuccess) return he;
  he = hipMemcpyAsync(d, h.data(), words * sizeof(uint64_t), hipMemcpyHostToDevice, stream);
  if (he == hipSuccess) {
    Fft16Args a;
    std::memset(&a, 0, sizeof a);
    a.in = d;
    a.out = d + n;
    a.cmp = d + n + n_rows;
    a.tw = tw;
    a.mat = reinterpret_cast<const uint32_t*>(d + n + 2u * n_rows);
    a.mismatch = mismatch;
    a.stripe_stride = stripe_stride;
    a.cols_per_stripe = cols;
    a.total = cols * n_stripes;
    a.nblk = pl.nblk;
    a.u = pl.u;
    a.n_rows = n_rows;
    a.mode = mode;
    a.per_stripe = per_stripe ? 1u : 0u;
    // one workgroup per CU (128 KiB of LDS), each looping over its columns
    int dev = 0, n_cu = 0;
    he = hipGetDevice(&dev);
    if (he == hipSuccess) he = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);
    if (he == hipSuccess) {
      const int64_t grid_opt = get_option(RSE_OPT_GRID_X);
      uint64_t gx = grid_opt > 0 ? (uint64_t)grid_opt : (uint64_t)std::max(n_cu, 1);
      if (gx > a.total) gx = a.total;
      if (gx > 0x7fffffffu) gx = 0x7fffffffu;
      void* args[] = {&a};
      he = hipLaunchKernel(reinterpret_cast<const void*>(&fft16_kernel), dim3((uint32_t)gx),
                           dim3(512), args, 0, stream);
    }
  }
  const hipError_t fe = hipFreeAsync(d, stream);
  if (he != hipSuccess) return he;
  if (fe != hipSuccess) return fe;
  note_kernel("fft gf16 %u+%u %s", pl.k, pl.p, what);
  count_bitslice_launch();
  *done = cols * 4096u;
  return hipSuccess;
}

}  // namespace rse
