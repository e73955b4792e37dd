// rse_locate.hip -- CDNA4 (gfx950) kernels of rse_locate_flat: which shards of
// a stripe are wrong.
//
// One fused pass reads every shard byte once and writes only flags.  Per byte
// column the stripe is a Reed-Solomon codeword or not (rse_locate_plan.hpp):
//
//  fast path  the arithmetic of the table check (rse_kernels.hip gf8_span in
//             kCheck mode): 16 B per lane, the (input, output) v_perm tables
//             built once per workgroup into LDS and read as wave-uniform
//             broadcasts, gf8_mac4 into p accumulators, XOR with the stored
//             parity: d = P data ^ parity.  A wave whose d is zero in every
//             lane is done: a clean stripe costs k * p multiplies per column,
//             as verify does.
//  slow path  only in waves where __ballot shows a nonzero d: per bad byte
//             column S = T d and the shared column decoder (Berlekamp-Massey,
//             root search) over log/exp tables in LDS; bad shards are ORed
//             into the workgroup's mask in LDS, which goes to the stripe's
//             accumulator in HBM with one atomicOr per touched word when the
//             workgroup leaves the stripe.
//
// A second, tiny kernel turns the accumulators into present / status.
#include "rse_device.hpp"
#include "rse_locate.hpp"
#include "rse_locate_plan.hpp"

namespace rse {
namespace {

constexpr int kLocBlock = 256;
constexpr int kLocKC = 4;  // inputs loaded before any arithmetic (as gf8_span's KC)

// (input, output) tables a workgroup holds: 2048 x 20 B = 40 KiB, four
// workgroups per CU.  NO = 16 past k = 128 rebuilds them per chunk of inputs.
template <int NO>
constexpr uint32_t loc_tabs() {
  return NO == 4 ? 1024u : 2048u;
}

struct LocLds {
  const uint4* tq;
  const uint32_t* tt2;
  const uint8_t* lg;  // log[256]
  const uint8_t* ex;  // exp[512]
  const uint8_t* T;   // 16 x 16
  uint32_t* acc;      // 8 mask words + the fail word
};

template <int NW>
__device__ __forceinline__ void loc_load(const uint8_t* p, bool valid, uint32_t (&x)[NW]) {
  if constexpr (NW == 4) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (valid) v = ld16<true>(p);
    x[0] = v.x;
    x[1] = v.y;
    x[2] = v.z;
    x[3] = v.w;
  } else {
    x[0] = valid ? (uint32_t)*(gptr<const uint8_t>)(p) : 0u;
  }
}

template <int NO>
__device__ __forceinline__ void loc_build_tabs(uint4* tq, uint32_t* tt2, const uint8_t* rows,
                                               uint32_t k, uint32_t p, uint32_t c0, uint32_t kc) {
  for (uint32_t t = threadIdx.x; t < p * kc; t += kLocBlock) {
    const uint32_t r = t / kc, i = t % kc;
    write_tab(tq, tt2, t, make_gf8_tab(rows[r * k + c0 + i]));
  }
}

// The rare path: the lane's bad byte columns through the column decoder.
// The accumulators are picked apart with unrolled selects inside a rolled loop
// over the columns, so they stay in VGPRs (inlined: a call would put them in
// scratch) and the decoder's code exists once per kernel.
template <int NO, int NW>
__device__ __forceinline__ void loc_slow(const LocLds& l, const uint32_t (&acc)[NO][NW], uint32_t p,
                                      uint32_t n) {
#pragma unroll 1
  for (uint32_t c = 0; c < (NW == 1 ? 1u : 4u * NW); ++c) {
    uint32_t d[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int r = 0; r < NO; ++r) {
      uint32_t v = acc[r][0];
#pragma unroll
      for (int w = 1; w < NW; ++w) {
        const uint32_t aw = acc[r][w];  // read, then select (rse_locate_plan.hpp pk_get)
        v = (c >> 2) == (uint32_t)w ? aw : v;
      }
      d[r >> 2] |= ((v >> ((c & 3u) * 8u)) & 0xFFu) << ((r & 3) * 8);
    }
    if ((d[0] | d[1] | d[2] | d[3]) == 0u) continue;
    uint32_t S[4], roots[2];
    locate_syndromes(l.lg, l.ex, l.T, d, p, S);
    const uint32_t L = locate_column(l.lg, l.ex, S, p, n, roots);
    if (L == kLocateBad) {
      atomicOr(&l.acc[8], 1u);
    } else {
      for (uint32_t i = 0; i < L; ++i) {
        const uint32_t r = pk_get(roots, i);
        atomicOr(&l.acc[r >> 5], 1u << (r & 31u));
      }
    }
  }
}

// One unit of a workgroup's sweep: lane t takes NW words of every shard at
// byte offset `off` of the stripe at sbase (NW = 4: a 16-byte vector; NW = 1:
// one byte, for the ragged tail and unaligned stripes).  Called by every
// thread of the workgroup (MULTI rebuilds the tables between barriers).
template <int NO, int NW, bool MULTI>
__device__ __forceinline__ void loc_unit(const LocateArgs& a, uint4* tq, uint32_t* tt2,
                                         const LocLds& l, const uint8_t* sbase, uint64_t off,
                                         bool valid) {
  constexpr uint32_t KCH = loc_tabs<NO>() / NO;
  const uint32_t k = a.k, p = a.p;
  uint32_t acc[NO][NW];
#pragma unroll
  for (int r = 0; r < NO; ++r)
#pragma unroll
    for (int w = 0; w < NW; ++w) acc[r][w] = 0u;
  for (uint32_t c0 = 0; c0 < k; c0 += KCH) {
    const uint32_t kc = k - c0 < KCH ? k - c0 : KCH;
    if (MULTI) {
      __syncthreads();
      loc_build_tabs<NO>(tq, tt2, a.consts + kLocRowsOff, k, p, c0, kc);
      __syncthreads();
    }
    const uint32_t lb = opaque_zero();
    const uint8_t* in = sbase + (uint64_t)c0 * a.shard_bytes + off;
    for (uint32_t i0 = 0; i0 < kc; i0 += kLocKC) {
      uint32_t x[kLocKC][NW];
#pragma unroll
      for (int j = 0; j < kLocKC; ++j)
        if (i0 + j < kc) loc_load<NW>(in + (uint64_t)(i0 + j) * a.shard_bytes, valid, x[j]);
#pragma unroll
      for (int j = 0; j < kLocKC; ++j) {
        if (!(i0 + j < kc)) continue;
        Sel sel[NW];
#pragma unroll
        for (int w = 0; w < NW; ++w) sel[w] = make_sel(x[j][w]);
#pragma unroll
        for (int r = 0; r < NO; ++r) {
          if (!((uint32_t)r < p)) continue;
          const Gf8Tab t = read_tab(tq, tt2, lb + r * kc + i0 + j);
#pragma unroll
          for (int w = 0; w < NW; ++w) acc[r][w] = gf8_mac4(acc[r][w], t, sel[w]);
        }
        // as gf8_span: keep the XOR chains from being reassociated into a tree
#pragma unroll
        for (int r = 0; r < NO; ++r)
#pragma unroll
          for (int w = 0; w < NW; ++w) pin(acc[r][w]);
      }
    }
  }
  uint32_t any = 0u;
  const uint8_t* par = sbase + (uint64_t)k * a.shard_bytes + off;
#pragma unroll
  for (int r = 0; r < NO; ++r) {
    if (!((uint32_t)r < p)) continue;
    uint32_t x[NW];
    loc_load<NW>(par + (uint64_t)r * a.shard_bytes, valid, x);
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      acc[r][w] ^= x[w];
      any |= acc[r][w];
    }
  }
  if (__ballot(any != 0u) == 0ull) return;
  if (any != 0u) loc_slow<NO, NW>(l, acc, p, k + p);
}

template <int NO, bool MULTI>
__global__ __launch_bounds__(kLocBlock) void locate_kernel(const LocateArgs a) {
  __shared__ uint4 tq[loc_tabs<NO>()];
  __shared__ uint32_t tt2[loc_tabs<NO>()];
  __shared__ uint32_t s_tab[256];  // log, exp, T: the first 1 KiB of the plan
  __shared__ uint32_t s_acc[kLocAccWords];

  s_tab[threadIdx.x] = reinterpret_cast<const uint32_t*>(a.consts)[threadIdx.x];
  if (threadIdx.x < kLocAccWords) s_acc[threadIdx.x] = 0u;
  if (!MULTI) loc_build_tabs<NO>(tq, tt2, a.consts + kLocRowsOff, a.k, a.p, 0u, a.k);
  __syncthreads();

  const uint8_t* tabs = reinterpret_cast<const uint8_t*>(s_tab);
  const LocLds l{tq, tt2, tabs + kLocLogOff, tabs + kLocExpOff, tabs + kLocTOff, s_acc};
  const uint64_t n_vspans = (a.n_vec + kLocBlock - 1) / kLocBlock;
  const uint64_t tail0 = a.n_vec * 16u;  // first byte of the byte-wise part
  const uint64_t n_units = n_vspans + (a.shard_bytes - tail0 + kLocBlock - 1) / kLocBlock;
  const uint64_t stride = (uint64_t)(a.k + a.p) * a.shard_bytes;

  for (uint64_t stripe = blockIdx.y; stripe < a.n_stripes; stripe += gridDim.y) {
    const uint8_t* sbase = a.base + stripe * stride;
    for (uint64_t u = blockIdx.x; u < n_units; u += gridDim.x) {
      if (u < n_vspans) {
        const uint64_t v = u * kLocBlock + threadIdx.x;
        loc_unit<NO, 4, MULTI>(a, tq, tt2, l, sbase, v * 16u, v < a.n_vec);
      } else {
        const uint64_t b = tail0 + (u - n_vspans) * kLocBlock + threadIdx.x;
        loc_unit<NO, 1, MULTI>(a, tq, tt2, l, sbase, b, b < a.shard_bytes);
      }
    }
    // the workgroup's findings on this stripe, one atomic per touched word
    __syncthreads();
    if (threadIdx.x < 9) {
      const uint32_t m = s_acc[threadIdx.x];
      if (m != 0u) {
        atomicOr(&a.acc[stripe * kLocAccWords + threadIdx.x], m);
        s_acc[threadIdx.x] = 0u;
      }
    }
    __syncthreads();
  }
}

// One thread per (stripe, shard): present = 0 exactly at the located shards;
// all 1 for a clean stripe, a stripe with an undecodable column, and one whose
// columns implicate more than p shards.
__global__ __launch_bounds__(256) void locate_finalize_kernel(const uint32_t* __restrict__ acc,
                                                              uint64_t n_stripes, uint32_t n,
                                                              uint32_t p,
                                                              uint8_t* __restrict__ present,
                                                              uint8_t* __restrict__ status) {
  const uint64_t total = n_stripes * n;
  for (uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x; idx < total;
       idx += (uint64_t)gridDim.x * 256u) {
    const uint64_t s = idx / n;
    const uint32_t r = (uint32_t)(idx % n);
    const uint32_t* w = acc + s * kLocAccWords;
    uint32_t cnt = 0u;
#pragma unroll
    for (int q = 0; q < 8; ++q) cnt += (uint32_t)__popc(w[q]);
    const bool bad = w[8] != 0u || cnt > p;
    const bool mine = ((w[r >> 5] >> (r & 31u)) & 1u) != 0u;
    present[idx] = (!bad && mine) ? 0u : 1u;
    if (r == 0u) status[s] = bad ? 2u : (cnt ? 1u : 0u);
  }
}

template <int NO>
void launch_locate_no(const LocateArgs& a, dim3 grid, hipStream_t stream) {
  constexpr uint32_t KCH = loc_tabs<NO>() / NO;
  if constexpr (KCH < 254u) {  // k <= 254: only NO = 16 can need more than one chunk
    if (a.k > KCH) {
      hipLaunchKernelGGL((locate_kernel<NO, true>), grid, dim3(kLocBlock), 0, stream, a);
      return;
    }
  }
  hipLaunchKernelGGL((locate_kernel<NO, false>), grid, dim3(kLocBlock), 0, stream, a);
}

}  // namespace

hipError_t launch_locate(const LocateArgs& args, uint8_t* present, uint8_t* status,
                         hipStream_t stream) {
  LocateArgs a = args;
  const uint32_t n = a.k + a.p;
  if (!locate_in_scope(8, a.k, a.p) || a.shard_bytes == 0 || a.n_stripes == 0)
    return hipErrorInvalidValue;
  // 16-byte vectors when every shard starts on a 16-byte boundary
  const bool al = (reinterpret_cast<uintptr_t>(a.base) % 16u) == 0 && a.shard_bytes % 16u == 0;
  a.n_vec = al ? a.shard_bytes / 16u : 0;
  hipError_t e = hipMemsetAsync(a.acc, 0, a.n_stripes * kLocAccWords * sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  const uint64_t units = (a.n_vec + kLocBlock - 1) / kLocBlock +
                         (a.shard_bytes - a.n_vec * 16u + kLocBlock - 1) / kLocBlock;
  const uint32_t gy = (uint32_t)(a.n_stripes < 65535u ? a.n_stripes : 65535u);
  // A few workgroups per CU over the whole grid, and at most four units per
  // workgroup while that keeps the grid small: the stripes that take the slow
  // path are then spread over many CUs instead of trailing the clean ones on
  // eight workgroups each.
  uint64_t gx = 4096u / gy;
  if (gx < units / 4u) gx = units / 4u;
  if (gx > 65536u / gy + 1u) gx = 65536u / gy + 1u;
  if (gx < 1) gx = 1;
  if (gx > units) gx = units;
  const dim3 grid((uint32_t)gx, gy);
  if (a.p <= 4)
    launch_locate_no<4>(a, grid, stream);
  else if (a.p <= 8)
    launch_locate_no<8>(a, grid, stream);
  else
    launch_locate_no<16>(a, grid, stream);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  const uint64_t total = a.n_stripes * n;
  const uint64_t fb = (total + 255u) / 256u;
  hipLaunchKernelGGL(locate_finalize_kernel, dim3((uint32_t)(fb < 65536u ? fb : 65536u)),
                     dim3(256), 0, stream, a.acc, a.n_stripes, n, a.p, present, status);
  return hipGetLastError();
}

}  // namespace rse
