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
//
// rse_scrub_flat's pre-filter route runs the same stripe body over a device
// list of stripes (correct_list_kernel); scrub_compact_kernel makes that list,
// and the caller's list of stripes that did not end CLEAN.
//
// rse_scrub_shards runs both sweep kernels over separately allocated shards:
// the kernels are instantiated a second time for CorrectShardsArgs, whose
// layout (rse_locate_core.hpp LocPtrs) reads a shard's address from a table.
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
// col0(r): the first of the lane's columns in shard r (a layout's cursor).
template <int NO, int NW, class Cursor>
__device__ __forceinline__ void cor_slow(const CorLds& l, const uint32_t (&acc)[NO][NW],
                                         uint32_t p, uint32_t n, const Cursor& col0) {
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
      gptr<uint8_t> q = (gptr<uint8_t>)(const_cast<uint8_t*>(col0(r)) + c);
      *q = (uint8_t)(*q ^ e);
      // a whole bad shard sets the same bit in every column: look before the atomic
      if (((l.mask[r >> 5] >> (r & 31u)) & 1u) == 0u) atomicOr(&l.mask[r >> 5], 1u << (r & 31u));
      ++stored;
    }
  }
  if (stored != 0u) atomicAdd(&l.cnt[0], (u64)stored);
  if (bad != 0u) atomicAdd(&l.cnt[1], (u64)bad);
}

// What a workgroup of the sweep kernels holds in LDS (COR_SHARED declares it
// in a kernel): the (input, output) tables, the plan's first 1 KiB (log, exp,
// T) and 1 / u, then the state of the stripe it is in -- its accounts, its
// erasures and their locator Gamma.  Nine arrays the compiler places, not one
// struct: as one struct correct_kernel<16, MULTI> allocated other registers.
struct CorShared {
  uint4* tq;
  uint32_t* tt2;
  uint32_t* tab;
  u64* cnt;
  uint32_t* mask;
  uint32_t* emask;
  uint32_t* gamma;
  uint32_t* f;
  uint8_t* epos;
};
#define COR_SHARED(NO, sh)                     \
  __shared__ uint4 tq[loc_tabs<NO>()];         \
  __shared__ uint32_t tt2[loc_tabs<NO>()];     \
  __shared__ uint32_t s_tab[256 + 64];         \
  __shared__ u64 s_cnt[2];                     \
  __shared__ uint32_t s_mask[8];               \
  __shared__ uint32_t s_emask[8];              \
  __shared__ uint32_t s_gamma[kCorGammaWords]; \
  __shared__ uint32_t s_f;                     \
  __shared__ uint8_t s_epos[16];               \
  const CorShared sh{tq, tt2, s_tab, s_cnt, s_mask, s_emask, s_gamma, &s_f, s_epos}

// The part of a listed stripe a workgroup of correct_list_kernel takes
// (rse_locate_core.hpp LocGridPart).
struct CorListPart {
  uint32_t f, s;
  __device__ __forceinline__ uint32_t first() const { return f; }
  __device__ __forceinline__ uint32_t step() const { return s; }
};

// Once per workgroup, before its first stripe: the tables, and the stripe
// state as a stripe without erasures and with nothing stored leaves it.
template <int NO, bool MULTI>
__device__ __forceinline__ void cor_enter(const CorShared& sh, const CorrectArgs& ca) {
  const LocateArgs& a = ca.loc;
  const uint32_t tid = threadIdx.x;
  sh.tab[tid] = reinterpret_cast<const uint32_t*>(a.consts)[tid];
  if (tid < 64) sh.tab[256 + tid] = reinterpret_cast<const uint32_t*>(a.consts + kCorInvUOff)[tid];
  if (tid < 2) sh.cnt[tid] = 0;
  if (tid < 8) sh.mask[tid] = sh.emask[tid] = 0u;
  if (tid < kCorGammaWords) sh.gamma[tid] = tid == 0 ? 1u : 0u;
  if (tid < 16) sh.epos[tid] = 0;
  if (tid == 0) *sh.f = 0u;
  if (!MULTI) loc_build_tabs<NO>(sh.tq, sh.tt2, a.consts + kLocRowsOff, a.k, a.p, 0u, a.k);
  __syncthreads();
}

// What a sweep kernel gets as its argument: CorrectArgs, the flat layout, or
// CorrectShardsArgs.  cor_args: the part both have; cor_layout: where stripe
// `stripe` lies.  The last block of separately allocated shards has its own
// length, and vectors only as far as it has whole ones.
__host__ __device__ __forceinline__ CorrectArgs& cor_args(CorrectArgs& ca) { return ca; }
__host__ __device__ __forceinline__ CorrectArgs& cor_args(CorrectShardsArgs& sa) { return sa.cor; }
__device__ __forceinline__ const CorrectArgs& cor_args(const CorrectArgs& ca) { return ca; }
__device__ __forceinline__ const CorrectArgs& cor_args(const CorrectShardsArgs& sa) {
  return sa.cor;
}
__device__ __forceinline__ LocFlat cor_layout(const CorrectArgs& ca, uint64_t stripe) {
  const LocateArgs& a = ca.loc;
  const uint64_t stride = (uint64_t)(a.k + a.p) * a.shard_bytes;
  return LocFlat{a.base + stripe * stride, a.shard_bytes, a.n_vec};
}
__device__ __forceinline__ LocPtrs cor_layout(const CorrectShardsArgs& sa, uint64_t stripe) {
  const LocateArgs& a = sa.cor.loc;
  const bool tail = sa.tail_bytes != 0 && stripe == a.n_stripes - 1;
  const uint64_t len = tail ? sa.tail_bytes : a.shard_bytes;
  return LocPtrs{sa.ptr, stripe * a.shard_bytes, len, sa.vec != 0u ? len / 16u : 0u};
}

// One stripe by one workgroup, which takes `part` of its units: the stripe's
// erasures, the sweep, the workgroup's account of it.  Called by every thread;
// the LDS state is left as cor_enter made it.
template <int NO, bool MULTI, class Lay, class Part>
__device__ __forceinline__ void cor_stripe(const CorShared& sh, const CorrectArgs& ca,
                                           const Lay& lay, uint64_t stripe, const Part& part) {
  const LocateArgs& a = ca.loc;
  const uint32_t p = a.p, n = a.k + a.p, tid = threadIdx.x;
  const uint8_t* tabs = reinterpret_cast<const uint8_t*>(sh.tab);
  uint32_t f = 0u;
  if (ca.present != nullptr) {
    // the stripe's erasures: nobody is in the slow path of the one before
    // (the barrier that ended it), so the LDS copy can be rewritten
    if (tid < 8) sh.emask[tid] = 0u;
    if (tid == 0) *sh.f = 0u;
    __syncthreads();
    if (tid < n && ca.present[stripe * n + tid] == 0) {
      atomicOr(&sh.emask[tid >> 5], 1u << (tid & 31u));
      const uint32_t i = atomicAdd(sh.f, 1u);
      if (i < 16u) sh.epos[i] = (uint8_t)tid;
    }
    __syncthreads();
    f = *sh.f;
    if (f <= p && tid == 0)
      correct_gamma(tabs + kLocLogOff, tabs + kLocExpOff, sh.epos, f, sh.gamma);
    __syncthreads();
    if (f > p) {  // the same for every thread: nothing of the stripe is read or written
      if (part.first() == 0 && tid == 0) a.acc[stripe * kLocAccWords + kCorAccSkipped] = 1u;
      return;
    }
  }
  const CorLds l{tabs + kLocLogOff, tabs + kLocExpOff, tabs + kLocTOff, tabs + 1024,
                 CorrectErasures{f, sh.epos, sh.gamma, sh.emask}, sh.mask, sh.cnt};
  const auto slow = [&](const auto& acc, const Lay& at, uint64_t off) {
    cor_slow(l, acc, p, n, at.from(0u, off));
  };
  loc_sweep<NO, MULTI>(a, sh.tq, sh.tt2, lay, slow, part);
  // the workgroup's account of this stripe, one atomic per touched word
  __syncthreads();
  if (tid < 8) {
    const uint32_t m = sh.mask[tid];
    if (m != 0u) {
      atomicOr(&a.acc[stripe * kLocAccWords + tid], m);
      sh.mask[tid] = 0u;
    }
  } else if (tid < 10) {
    const u64 v = sh.cnt[tid - 8];
    if (v != 0) {
      atomicAdd(reinterpret_cast<u64*>(&a.acc[stripe * kLocAccWords + kCorAccStored]) + (tid - 8),
                v);
      sh.cnt[tid - 8] = 0;
    }
  }
  __syncthreads();
}

// Every stripe: grid.x workgroups share a stripe, grid.y stripes are in flight.
template <int NO, bool MULTI, class Args = CorrectArgs>
__global__ __launch_bounds__(kLocBlock) void correct_kernel(const Args args) {
  COR_SHARED(NO, sh);
  const CorrectArgs& ca = cor_args(args);
  cor_enter<NO, MULTI>(sh, ca);
  for (uint64_t stripe = blockIdx.y; stripe < ca.loc.n_stripes; stripe += gridDim.y)
    cor_stripe<NO, MULTI>(sh, ca, cor_layout(args, stripe), stripe, LocGridPart{});
}

// The stripes list[0 .. *n_list) only (rse_scrub_flat's work list: both are
// written on the device, so the grid cannot follow the count).  The grid is
// sized by the device; a stripe is split into as many parts as that leaves
// workgroups for (at most one per unit), and the (stripe, part) pairs are
// walked with the grid's stride.  A workgroup without a pair returns before it
// builds any table: an empty list costs the launch.
template <int NO, bool MULTI, class Args = CorrectArgs>
__global__ __launch_bounds__(kLocBlock) void correct_list_kernel(
    const Args args, const uint32_t* __restrict__ list, const uint32_t* __restrict__ n_list) {
  COR_SHARED(NO, sh);
  const CorrectArgs& ca = cor_args(args);
  const uint64_t cnt = *n_list, units = loc_units(ca.loc);
  uint64_t parts = cnt != 0 ? gridDim.x / cnt : 0;
  parts = parts < 1 ? 1 : parts > units ? units : parts;
  const uint64_t work = cnt * parts;
  if (blockIdx.x >= work) return;
  cor_enter<NO, MULTI>(sh, ca);
  for (uint64_t w = blockIdx.x; w < work; w += gridDim.x) {
    const uint64_t stripe = list[w / parts];
    cor_stripe<NO, MULTI>(sh, ca, cor_layout(args, stripe), stripe,
                          CorListPart{(uint32_t)(w % parts), (uint32_t)parts});
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

// rse_scrub_flat's lists: the stripes that have a nonzero verdict word, an
// erased flag or a status that is not CLEAN (each array nullable), in ascending
// order into list[0 .. *count).  One workgroup walks the stripes in order,
// kCmpItems x 64 consecutive ones per wave and trip: a stripe's place is the
// entries of the trips before (base), of the waves before (through LDS, two
// buffers so that a trip needs one barrier) and of the ballots before, plus
// the hits below its lane.  list and count are nullable too.
constexpr int kCmpBlock = 1024, kCmpWaves = kCmpBlock / 64, kCmpItems = 4;

__global__ __launch_bounds__(kCmpBlock) void scrub_compact_kernel(
    const uint32_t* __restrict__ words, const uint8_t* __restrict__ present, uint32_t n,
    const uint8_t* __restrict__ status, uint64_t n_stripes, uint32_t* __restrict__ list,
    uint32_t* __restrict__ count) {
  __shared__ uint32_t s_wave[2][kCmpWaves];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t base = 0u;
  for (uint64_t s0 = 0, trip = 0; s0 < n_stripes; s0 += (uint64_t)kCmpBlock * kCmpItems, ++trip) {
    const uint64_t mine = s0 + (uint64_t)wave * (kCmpItems * 64u) + lane;
    u64 hit[kCmpItems];
    uint32_t total = 0u;
#pragma unroll
    for (int j = 0; j < kCmpItems; ++j) {
      const uint64_t s = mine + (uint64_t)j * 64u;
      bool h = false;
      if (s < n_stripes) {
        if (words != nullptr) h = words[s] != 0u;
        if (status != nullptr) h = h || status[s] != 0;
        if (present != nullptr)
          for (uint32_t r = 0; r < n && !h; ++r) h = present[s * n + r] == 0;
      }
      hit[j] = __ballot(h);
      total += (uint32_t)__popcll(hit[j]);
    }
    if (lane == 0) s_wave[trip & 1u][wave] = total;
    __syncthreads();
    uint32_t at = base;
#pragma unroll
    for (int w = 0; w < kCmpWaves; ++w) {
      const uint32_t v = s_wave[trip & 1u][w];
      base += v;
      if ((uint32_t)w < wave) at += v;
    }
#pragma unroll
    for (int j = 0; j < kCmpItems; ++j) {
      if (list != nullptr && ((hit[j] >> lane) & 1ull) != 0)
        list[at + (uint32_t)__popcll(hit[j] & ((1ull << lane) - 1ull))] =
            (uint32_t)(mine + (uint64_t)j * 64u);
      at += (uint32_t)__popcll(hit[j]);
    }
  }
  if (count != nullptr && threadIdx.x == 0) *count = base;
}

}  // namespace

hipError_t launch_scrub_compact(const uint32_t* words, const uint8_t* present, uint32_t n,
                                const uint8_t* status, uint64_t n_stripes, uint32_t* list,
                                uint32_t* count, hipStream_t stream) {
  if (n_stripes > 0xFFFFFFFFull) return hipErrorInvalidValue;  // the list's entries are 32-bit
  hipLaunchKernelGGL(scrub_compact_kernel, dim3(1), dim3(kCmpBlock), 0, stream, words, present, n,
                     status, n_stripes, list, count);
  return hipGetLastError();
}

namespace {

// The two passes of every entry above.  `a` is the sweep kernels' argument of
// either layout, `al` whether the layout admits 16-byte vectors; with a list
// the first pass is over the stripes list[0 .. *n_list), else over all.
template <class Args>
hipError_t cor_launch(Args& a, bool al, const uint32_t* list, const uint32_t* n_list,
                      uint8_t* status, uint8_t* changed, uint32_t* counts, hipStream_t stream) {
  static_assert(kCorAccBad == kCorAccStored + 2 && kCorAccSkipped < kLocAccWords, "accumulator");
  static_assert(sizeof(Args) + 2 * sizeof(void*) <= 4096, "the kernel-argument block");
  int dev = 0, cus = 0;
  if (list != nullptr) {
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess)
      e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
  }
  LocateArgs& loc = cor_args(a).loc;
  return loc_launch(
      loc, al, stream,
      [&](auto no, auto multi, dim3 grid) {
        constexpr int NO = decltype(no)::value;
        constexpr bool MULTI = decltype(multi)::value;
        if (list == nullptr) {
          hipLaunchKernelGGL((correct_kernel<NO, MULTI, Args>), grid, dim3(kLocBlock), 0, stream,
                             a);
          return;
        }
        // loc_grid's shape is by the stripe count: not used.  Four workgroups per CU:
        // sizing it by what the device holds at once (5 per CU at p <= 4, 3 above) was
        // tried: no faster at 10+4, slower at 100+16
        const dim3 lgrid((uint32_t)(cus > 0 ? cus : 1) * 4u);
        hipLaunchKernelGGL((correct_list_kernel<NO, MULTI, Args>), lgrid, dim3(kLocBlock), 0,
                           stream, a, list, n_list);
      },
      [&](dim3 blocks) {
        hipLaunchKernelGGL(correct_finalize_kernel, blocks, dim3(256), 0, stream, loc.acc,
                           loc.n_stripes, loc.k + loc.p, status, changed, counts);
      });
}

}  // namespace

hipError_t launch_correct_list(const CorrectArgs& args, const uint32_t* list,
                               const uint32_t* n_list, uint8_t* status, uint8_t* changed,
                               uint32_t* counts, hipStream_t stream) {
  if (list == nullptr) return hipErrorInvalidValue;
  CorrectArgs a = args;
  return cor_launch(a, loc_flat_aligned(a.loc), list, n_list, status, changed, counts, stream);
}

hipError_t launch_correct(const CorrectArgs& args, uint8_t* status, uint8_t* changed,
                          uint32_t* counts, hipStream_t stream) {
  CorrectArgs a = args;
  return cor_launch(a, loc_flat_aligned(a.loc), nullptr, nullptr, status, changed, counts, stream);
}

hipError_t launch_correct_shards(const CorrectShardsArgs& args, const uint32_t* list,
                                 const uint32_t* n_list, uint8_t* status, uint8_t* changed,
                                 uint32_t* counts, hipStream_t stream) {
  CorrectShardsArgs a = args;
  return cor_launch(a, a.vec != 0u, list, n_list, status, changed, counts, stream);
}

}  // namespace rse
