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
#include "rse_locate_core.hpp"

namespace rse {
namespace {

using namespace locate_core;

struct LocLds {
  const uint8_t* lg;  // log[256]
  const uint8_t* ex;  // exp[512]
  const uint8_t* T;   // 16 x 16
  uint32_t* acc;      // 8 mask words + the fail word
};

// The rare path: the lane's bad byte columns through the column decoder.
// The accumulators are picked apart with unrolled selects inside a rolled loop
// over the columns, so they stay in VGPRs (inlined: a call would put them in
// scratch) and the decoder's code exists once per kernel.
template <int NO, int NW>
__device__ __forceinline__ void loc_slow(const LocLds& l, const uint32_t (&acc)[NO][NW], uint32_t p,
                                      uint32_t n) {
#pragma unroll 1
  for (uint32_t c = 0; c < (NW == 1 ? 1u : 4u * NW); ++c) {
    uint32_t d[4];
    loc_column_d<NO, NW>(acc, c, d);
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
  const LocLds l{tabs + kLocLogOff, tabs + kLocExpOff, tabs + kLocTOff, s_acc};
  const uint32_t p = a.p, n = a.k + a.p;
  const auto slow = [&](const auto& acc, const LocFlat&, uint64_t) { loc_slow(l, acc, p, n); };
  const uint64_t stride = (uint64_t)(a.k + a.p) * a.shard_bytes;

  for (uint64_t stripe = blockIdx.y; stripe < a.n_stripes; stripe += gridDim.y) {
    loc_sweep<NO, MULTI>(a, tq, tt2, LocFlat{a.base + stripe * stride, a.shard_bytes, a.n_vec},
                         slow);
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

}  // namespace

hipError_t launch_locate(const LocateArgs& args, uint8_t* present, uint8_t* status,
                         hipStream_t stream) {
  LocateArgs a = args;
  return loc_launch(
      a, loc_flat_aligned(a), stream,
      [&](auto no, auto multi, dim3 grid) {
        hipLaunchKernelGGL((locate_kernel<decltype(no)::value, decltype(multi)::value>), grid,
                           dim3(kLocBlock), 0, stream, a);
      },
      [&](dim3 blocks) {
        hipLaunchKernelGGL(locate_finalize_kernel, blocks, dim3(256), 0, stream, a.acc,
                           a.n_stripes, a.k + a.p, a.p, present, status);
      });
}

}  // namespace rse
