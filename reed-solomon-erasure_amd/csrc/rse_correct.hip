// rse_correct.hip -- CDNA4 (gfx950) kernels of rse_correct_flat: wrong bytes
// are repaired where they lie, known-missing shards (erasures) included.
//
// One fused pass over every stripe.  The fast path is rse_locate_flat's
// (rse_locate_core.hpp): d = P data ^ parity per byte column, and a wave whose
// d is zero in every lane is done -- with erasures too: d = 0 says that the
// column, whatever the erased shards hold, already is a codeword.
//
//  stripe entry  with a present array, the workgroup reads the stripe's row:
//                erased shards into a mask, a list and their count f in LDS.
//                f > p: the stripe is skipped unread.  Otherwise one thread
//                builds the erasure locator Gamma into LDS.
//  slow path     per bad byte column of a lane S = T d and the shared column
//                decoder (rse_correct_plan.hpp): positions and values.  Every
//                nonzero value is one byte load, XOR and byte store.  No
//                atomics on data: a column of a stripe belongs to one lane of
//                one workgroup, which has read it before it writes.
//  accounting    changed-shard mask and the two counters in LDS, added to the
//                stripe's accumulator in HBM when the workgroup leaves it.
//
// A second, tiny kernel turns the accumulators into status / changed / counts.
#include "rse_correct.hpp"
#include "rse_correct_plan.hpp"
#include "rse_locate_core.hpp"

namespace rse {
namespace {

using namespace locate_core;
using u64 = unsigned long long;

struct CorLds {
  const uint8_t* lg;    // log[256]
  const uint8_t* ex;    // exp[512]
  const uint8_t* T;     // 16 x 16
  const uint8_t* invu;  // 1 / u_r
  CorrectErasures er;   // of the stripe the workgroup is in
  uint32_t* mask;       // 8 words: shards with a stored byte
  u64* cnt;             // bytes stored, columns left undecodable
};

// The rare path: the lane's bad byte columns through the column decoder, the
// error values XORed into the stripe.  Rolled over the columns with the
// accumulators picked apart by selects, as rse_locate.hip's loc_slow.
template <int NO, int NW>
__device__ __forceinline__ void cor_slow(const CorLds& l, const uint32_t (&acc)[NO][NW],
                                         uint32_t p, uint32_t n, uint8_t* col0,
                                         uint64_t shard_bytes) {
  uint32_t stored = 0u, bad = 0u;  // of the lane's columns: one atomic each at the end
#pragma unroll 1
  for (uint32_t c = 0; c < (NW == 1 ? 1u : 4u * NW); ++c) {
    uint32_t d[4];
    loc_column_d<NO, NW>(acc, c, d);
    if ((d[0] | d[1] | d[2] | d[3]) == 0u) continue;
    uint32_t S[4], pos[4], val[4];
    locate_syndromes(l.lg, l.ex, l.T, d, p, S);
    const uint32_t m = correct_column(l.lg, l.ex, l.invu, S, p, n, l.er, pos, val);
    if (m == kLocateBad) {
      ++bad;
      continue;
    }
    for (uint32_t i = 0; i < m; ++i) {
      const uint32_t e = pk_get(val, i);
      if (e == 0u) continue;
      const uint32_t r = pk_get(pos, i);
      gptr<uint8_t> q = (gptr<uint8_t>)(col0 + (uint64_t)r * shard_bytes + c);
      *q = (uint8_t)(*q ^ e);
      // a whole bad shard sets the same bit in every column: look before the atomic
      if (((l.mask[r >> 5] >> (r & 31u)) & 1u) == 0u) atomicOr(&l.mask[r >> 5], 1u << (r & 31u));
      ++stored;
    }
  }
  if (stored != 0u) atomicAdd(&l.cnt[0], (u64)stored);
  if (bad != 0u) atomicAdd(&l.cnt[1], (u64)bad);
}

template <int NO, bool MULTI>
__global__ __launch_bounds__(kLocBlock) void correct_kernel(const CorrectArgs ca) {
  __shared__ uint4 tq[loc_tabs<NO>()];
  __shared__ uint32_t tt2[loc_tabs<NO>()];
  __shared__ uint32_t s_tab[256 + 64];  // log, exp, T: the first 1 KiB of the plan; 1 / u
  __shared__ u64 s_cnt[2];
  __shared__ uint32_t s_mask[8];
  __shared__ uint32_t s_emask[8];
  __shared__ uint32_t s_gamma[kCorGammaWords];
  __shared__ uint32_t s_f;
  __shared__ uint8_t s_epos[16];

  const LocateArgs& a = ca.loc;
  const uint32_t p = a.p, n = a.k + a.p, tid = threadIdx.x;
  s_tab[tid] = reinterpret_cast<const uint32_t*>(a.consts)[tid];
  if (tid < 64) s_tab[256 + tid] = reinterpret_cast<const uint32_t*>(a.consts + kCorInvUOff)[tid];
  if (tid < 2) s_cnt[tid] = 0;
  if (tid < 8) s_mask[tid] = s_emask[tid] = 0u;
  if (tid < kCorGammaWords) s_gamma[tid] = tid == 0 ? 1u : 0u;
  if (tid < 16) s_epos[tid] = 0;
  if (tid == 0) s_f = 0u;
  if (!MULTI) loc_build_tabs<NO>(tq, tt2, a.consts + kLocRowsOff, a.k, a.p, 0u, a.k);
  __syncthreads();

  const uint8_t* tabs = reinterpret_cast<const uint8_t*>(s_tab);
  const uint64_t stride = (uint64_t)n * a.shard_bytes;

  for (uint64_t stripe = blockIdx.y; stripe < a.n_stripes; stripe += gridDim.y) {
    uint32_t f = 0u;
    if (ca.present != nullptr) {
      // the stripe's erasures: nobody is in the slow path of the one before
      // (the barrier that ended it), so the LDS copy can be rewritten
      if (tid < 8) s_emask[tid] = 0u;
      if (tid == 0) s_f = 0u;
      __syncthreads();
      if (tid < n && ca.present[stripe * n + tid] == 0) {
        atomicOr(&s_emask[tid >> 5], 1u << (tid & 31u));
        const uint32_t i = atomicAdd(&s_f, 1u);
        if (i < 16u) s_epos[i] = (uint8_t)tid;
      }
      __syncthreads();
      f = s_f;
      if (f <= p && tid == 0)
        correct_gamma(tabs + kLocLogOff, tabs + kLocExpOff, s_epos, f, s_gamma);
      __syncthreads();
      if (f > p) {  // the same for every thread: nothing of the stripe is read or written
        if (blockIdx.x == 0 && tid == 0) a.acc[stripe * kLocAccWords + kCorAccSkipped] = 1u;
        continue;
      }
    }
    const CorLds l{tabs + kLocLogOff, tabs + kLocExpOff, tabs + kLocTOff, tabs + 1024,
                   CorrectErasures{f, s_epos, s_gamma, s_emask}, s_mask, s_cnt};
    const auto slow = [&](const auto& acc, const uint8_t* sbase, uint64_t off) {
      cor_slow(l, acc, p, n, const_cast<uint8_t*>(sbase) + off, a.shard_bytes);
    };
    loc_sweep<NO, MULTI>(a, tq, tt2, a.base + stripe * stride, slow);
    // the workgroup's account of this stripe, one atomic per touched word
    __syncthreads();
    if (tid < 8) {
      const uint32_t m = s_mask[tid];
      if (m != 0u) {
        atomicOr(&a.acc[stripe * kLocAccWords + tid], m);
        s_mask[tid] = 0u;
      }
    } else if (tid < 10) {
      const u64 v = s_cnt[tid - 8];
      if (v != 0) {
        atomicAdd(reinterpret_cast<u64*>(&a.acc[stripe * kLocAccWords + kCorAccStored]) + (tid - 8),
                  v);
        s_cnt[tid - 8] = 0;
      }
    }
    __syncthreads();
  }
}

// One thread per (stripe, shard): changed flags; the thread of shard 0 also
// writes the stripe's status and counts (saturated).
__global__ __launch_bounds__(256) void correct_finalize_kernel(const uint32_t* __restrict__ acc,
                                                               uint64_t n_stripes, uint32_t n,
                                                               uint8_t* __restrict__ status,
                                                               uint8_t* __restrict__ changed,
                                                               uint32_t* __restrict__ counts) {
  const uint64_t total = n_stripes * n;
  for (uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x; idx < total;
       idx += (uint64_t)gridDim.x * 256u) {
    const uint64_t s = idx / n;
    const uint32_t r = (uint32_t)(idx % n);
    const uint32_t* w = acc + s * kLocAccWords;
    if (changed != nullptr) changed[idx] = (uint8_t)((w[r >> 5] >> (r & 31u)) & 1u);
    if (r == 0u) {
      const u64 stored = reinterpret_cast<const u64*>(w + kCorAccStored)[0];
      const u64 bad = reinterpret_cast<const u64*>(w + kCorAccStored)[1];
      status[s] = (bad != 0 || w[kCorAccSkipped] != 0u) ? 2u : (stored != 0 ? 1u : 0u);
      if (counts != nullptr) {
        counts[2 * s] = stored > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)stored;
        counts[2 * s + 1] = bad > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)bad;
      }
    }
  }
}

}  // namespace

hipError_t launch_correct(const CorrectArgs& args, uint8_t* status, uint8_t* changed,
                          uint32_t* counts, hipStream_t stream) {
  static_assert(kCorAccBad == kCorAccStored + 2 && kCorAccSkipped < kLocAccWords, "accumulator");
  CorrectArgs a = args;
  return loc_launch(
      a.loc, stream,
      [&](auto no, auto multi, dim3 grid) {
        hipLaunchKernelGGL((correct_kernel<decltype(no)::value, decltype(multi)::value>), grid,
                           dim3(kLocBlock), 0, stream, a);
      },
      [&](dim3 blocks) {
        hipLaunchKernelGGL(correct_finalize_kernel, blocks, dim3(256), 0, stream, a.loc.acc,
                           a.loc.n_stripes, a.loc.k + a.loc.p, status, changed, counts);
      });
}

}  // namespace rse
