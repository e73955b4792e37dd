// rse_read.hip -- rse_read_flat, rse_read_shards: shards of the flat layout
// (at the end of this comment: of separately allocated shards) read into the
// caller's rows, the erased ones rebuilt on the way from the first k present
// shards of their stripe (reconstruct, core.rs:733-923, for the shards asked
// for and into a buffer of the caller's).  `stripes` is only read.
//
// Three launches on the caller's stream.
//  * read_list_kernel, one workgroup, is rse_update_flat's walk over the list
//    (list_pass, rse_list_pass.hpp) with k + p as the bound of a shard index:
//    the verdict and the run count into the workspace, the run heads compacted
//    in ascending order and closed by n_reads, `result` = {verdict, first
//    offender or 0}.
//  * read_plan_kernel, a workgroup per run in grid strides, returns at once on
//    a rejected list -- no address is ever formed from an entry that is not in
//    order -- and else calls read_plan_run (rse_read_plan.hpp) on the run's flag
//    row over LDS.  Every entry's class goes into `status` and into the
//    workspace, the lost ones are counted into result[1] (a word atomic: not
//    shard bytes), the valid set goes into the workspace, and every coefficient
//    of a rebuilt entry is stored as the ready multiply table (make_gf8_tab).
//  * read_kernel steps in grid strides over (run, group, span) items: at most
//    kReadRows entries of one stripe, 4 KiB of every shard they need, 16 bytes
//    per lane.  Where the group has a rebuilt entry the lane loads its bytes
//    of each shard of the valid set once and adds coef x bytes to every
//    rebuilt entry's sum (gf8_mac4); then a row is stored per entry, a copied
//    entry being a load and a store and a lost one skipped.  A group without a
//    rebuilt entry reads nothing but the copied shards.
//
// The tables.  The coefficients are a run's own, not the codec's as in
// rse_update.hip, so there is no table set a workgroup could build once.  The
// planner stores the 20-byte table of every (entry, input), and the kernel reads
// it where it is used through the constant address space: entry, input and run
// are the same in every lane, so these are scalar loads into SGPRs (as
// gf8_code_desc_kernel reads its descriptors), written by the launch before and
// never during this one.  No LDS image, so no barrier per item and no limit on
// the workgroups per compute unit but the registers.  The index is made
// through opaque_zero() and the sums are pinned, as gf8_span does it.
//
// A GF(2^16) codec of at most 256 shards has its matrix, and so every inverse
// and product of it, in the GF(2^8) subfield, where a constant multiplies each
// byte of an element by itself: the same kernels over 2 x shard_len bytes.
//
// rse_read_shards is the same three launches.  The list pass is shared as it
// is.  The planner (read_shards_plan_kernel) passes read_plan_run the pointer
// table from its arguments as the "has no buffer" predicate: a NULL shard is
// erased in every block.  The read kernel gets another address rule
// (ReadShards below): one pointer per shard from the kernel arguments, a block
// of columns in the place of a stripe, a shorter last block.  It takes a shard
// index from a run's valid set or from a copied entry and from nowhere else,
// and the planner puts a NULL shard in neither: no address is formed from one.
#include "rse_read.hpp"

#include "rse_list_pass.hpp"
#include "rse_read_plan.hpp"

namespace rse {
namespace {

// Reads at addresses that are the same in every lane, of memory no launch
// writes while this one runs: through the constant address space.
template <class T>
using cptr = const __attribute__((address_space(4))) T*;
__device__ __forceinline__ uint32_t cword(const uint32_t* p, uint64_t i) {
  return ((cptr<uint32_t>)p)[i];
}
__device__ __forceinline__ Gf8Tab ctab(const uint4* q, const uint32_t* t2, uint64_t i) {
  const u32x4 v = ((cptr<u32x4>)q)[i];
  Gf8Tab t;
  t.t0lo = v.x;
  t.t0hi = v.y;
  t.t1lo = v.z;
  t.t1hi = v.w;
  t.t2 = cword(t2, i);
  return t;
}

// The workspace's parts (rse_read.hpp read_ws).
struct Ws {
  uint32_t *words, *heads, *cls, *valid, *tabt2;
  uint4* tabq;
};
__device__ __forceinline__ Ws ws_of(const ReadArgs& a) {
  const ReadWs o = read_ws(a.n_reads, a.k);
  Ws w;
  w.words = reinterpret_cast<uint32_t*>(a.ws);
  w.heads = w.words + kReadWsHeads;
  w.cls = reinterpret_cast<uint32_t*>(a.ws + o.cls);
  w.valid = reinterpret_cast<uint32_t*>(a.ws + o.valid);
  w.tabq = reinterpret_cast<uint4*>(a.ws + o.tabq);
  w.tabt2 = reinterpret_cast<uint32_t*>(a.ws + o.tabt2);
  return w;
}

__global__ __launch_bounds__(kPlanBlock) void read_list_kernel(ReadArgs a) {
  const Ws w = ws_of(a);
  uint32_t first, runs;
  if (list_pass(a.reads, a.n_reads, a.n_stripes, a.k + a.p, w.heads, first, runs)) {
    const bool rejected = first != kNoOffender;
    w.words[kReadWsStatus] = rejected ? RSE_READ_REJECTED : RSE_READ_SERVED;
    w.words[kReadWsRuns] = runs;
    w.heads[runs] = a.n_reads;  // run r is the entries [heads[r], heads[r + 1])
    a.result[0] = rejected ? RSE_READ_REJECTED : RSE_READ_SERVED;
    a.result[1] = rejected ? first : 0u;  // accepted: the planner counts the lost entries
  }
}

// What read_plan_run hands out, stored where the read kernel looks for it.
struct PlanEmit {
  uint8_t* status;
  uint32_t* lost;
  uint32_t* cls_words;
  uint4* tabq;
  uint32_t* tabt2;
  uint64_t head;
  uint32_t k;
  __device__ __forceinline__ void cls(uint32_t j, uint8_t c) {
    status[head + j] = c;
    cls_words[head + j] = c;
    if (c == kReadLost) atomicAdd(lost, 1u);
  }
  __device__ __forceinline__ void coef(uint32_t j, uint32_t i, uint8_t c) {
    const Gf8Tab t = make_gf8_tab(c);
    const uint64_t at = (head + j) * k + i;
    tabq[at] = make_uint4(t.t0lo, t.t0hi, t.t1lo, t.t1hi);
    tabt2[at] = t.t2;
  }
};

struct BlockSync {
  __device__ __forceinline__ void operator()() const { __syncthreads(); }
};

constexpr int kReadPlanBlock = 256;

// The planner's body: every run's plan, with the layout's "has no buffer"
// predicate for read_plan_run.
template <class NoBuffer>
__device__ __forceinline__ void read_plan_runs(const ReadArgs& a, NoBuffer no_buffer) {
  __shared__ uint8_t lg[256], ex[512];
  __shared__ uint8_t s_fl[kReadMaxShards], s_where[kReadMaxShards], s_valid[kReadMaxShards];
  __shared__ uint8_t s_S[kReadMaxP], s_R[kReadMaxP];
  __shared__ uint8_t s_A[kReadWorkA], s_D[kReadWorkD];
  __shared__ uint32_t s_sc[4];
  const Ws w = ws_of(a);
  if (w.words[kReadWsStatus] != RSE_READ_SERVED) return;  // rejected: nothing is read or written

  // log and doubled exp of GF(2^8), generator 2 modulo 0x11D (rse_field.hpp Gf8)
  for (uint32_t l = threadIdx.x; l < 512u; l += kReadPlanBlock) {
    uint32_t r = 1u;
    for (uint32_t s = l % 255u; s != 0; --s) r = xtime(r);
    ex[l] = l < 510u ? (uint8_t)r : 0;
    if (l < 255u) lg[r] = (uint8_t)l;
  }
  if (threadIdx.x == 0) lg[0] = 0;
  __syncthreads();

  const ReadRunWork work{s_fl, s_where, s_valid, s_S, s_R, s_A, s_D, s_sc};
  const uint32_t runs = w.words[kReadWsRuns], T = a.k + a.p;
  for (uint32_t run = blockIdx.x; run < runs; run += gridDim.x) {
    const uint32_t head = w.heads[run], n = w.heads[run + 1] - head;
    const uint32_t stripe = a.reads[2 * (uint64_t)head];
    PlanEmit emit{a.status, a.result + 1, w.cls, w.tabq, w.tabt2, head, a.k};
    read_plan_run(lg, ex, a.coef, a.k, a.p,
                  a.present ? a.present + (uint64_t)stripe * T : nullptr,
                  a.reads + 2 * (uint64_t)head, n, work, emit, threadIdx.x, kReadPlanBlock,
                  BlockSync(), no_buffer);
    if (s_sc[3])  // a run of a stripe that is not recoverable rebuilds nothing
      for (uint32_t i = threadIdx.x; i < a.k; i += kReadPlanBlock)
        w.valid[(uint64_t)run * a.k + i] = s_valid[i];
  }
}

__global__ __launch_bounds__(kReadPlanBlock) void read_plan_kernel(ReadArgs a) {
  read_plan_runs(a, ReadAllBuffers());
}

// rse_read_shards: "stripe" is a block, and a shard whose pointer is NULL has
// no buffer.  The pointers are compared, never dereferenced.
__global__ __launch_bounds__(kReadPlanBlock) void read_shards_plan_kernel(ReadShardsArgs args) {
  read_plan_runs(args.rd, ReadNullShards{args.ptr});
}

// Where an item's bytes lie: the addressing policy of read_kernel, in the
// manner of rse_update.hip's UpdFlat.  A layout names the call's argument block,
// says how many bytes span s of a run has (0: the item is sat out), and makes a
// cursor per item for the lane's offset `off` into the run's stripe: the lane's
// address in shard i.
//
// The flat layout: base + stripe x (k + p) x bytes + shard x bytes.
struct ReadFlat {
  using Args = ReadArgs;
  static __host__ __device__ __forceinline__ const ReadArgs& rd(const Args& a) { return a; }
  static __device__ __forceinline__ uint64_t span_len(const Args& a, uint32_t, uint64_t span) {
    return update_span_len(a.shard_bytes, span);
  }
  struct At {
    const uint8_t* sbase;
    uint64_t bytes;
    __device__ __forceinline__ const uint8_t* shard(uint32_t i) const {
      return sbase + (uint64_t)i * bytes;
    }
  };
  static __device__ __forceinline__ At at(const Args& a, uint32_t stripe, uint64_t off) {
    return At{a.base + (uint64_t)stripe * (a.k + a.p) * a.shard_bytes + off, a.shard_bytes};
  }
};

// Separately allocated shards (rse_read_shards): ptr[shard] + block x block
// bytes, the pointers read from the kernel arguments.  The shard index is the
// same in every lane -- a word of the valid set, or a copied entry's shard --
// so a pointer is a scalar load.  A run in the shorter last block has the
// tail's bytes: fewer spans, a shorter last lane.  A row of `out` keeps the
// full block's stride.
struct ReadShards {
  using Args = ReadShardsArgs;
  static __host__ __device__ __forceinline__ const ReadArgs& rd(const Args& a) { return a.rd; }
  static __device__ __forceinline__ uint64_t span_len(const Args& a, uint32_t block,
                                                      uint64_t span) {
    return update_run_span_len(update_run_bytes(a.rd.shard_bytes, a.tail_bytes, a.n_full, block),
                               span);
  }
  struct At {
    const uint8_t* const* ptr;
    uint64_t o;
    __device__ __forceinline__ const uint8_t* shard(uint32_t i) const { return ptr[i] + o; }
  };
  static __device__ __forceinline__ At at(const Args& a, uint32_t block, uint64_t off) {
    return At{a.ptr, (uint64_t)block * a.rd.shard_bytes + off};
  }
};

constexpr int kReadKc = 4;  // shards of the valid set a lane has in flight

// NO: rows a lane accumulates, at least the entries of the call's largest
// group.  LAY: ReadFlat or ReadShards; below, "stripe" and "shard bytes" are a
// block and a full block's bytes for the latter.
template <int NO, bool VEC, class LAY>
__global__ __launch_bounds__(kUpdBlock) void read_kernel(typename LAY::Args args) {
  const ReadArgs& a = LAY::rd(args);
  const Ws w = ws_of(a);
  if (cword(w.words, kReadWsStatus) != RSE_READ_SERVED) return;  // rejected: nothing is read or written

  const uint32_t k = a.k;
  const uint64_t bytes = a.shard_bytes;
  const uint64_t n_spans = update_spans(bytes);
  // every run has the groups of the longest run there can be; the ones past a
  // run's own are sat out
  const uint64_t n_groups = read_groups(read_max_run(a.n_reads, a.k + a.p));
  const uint64_t n_items = (uint64_t)cword(w.words, kReadWsRuns) * n_groups * n_spans;

  for (uint64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
    const uint64_t span = item % n_spans, rg = item / n_spans;
    const uint64_t run = rg / n_groups;
    const uint32_t g = (uint32_t)(rg % n_groups);
    const uint32_t head = cword(w.heads, run), entries = cword(w.heads, run + 1) - head;
    if (read_group_first(g) >= entries) continue;
    const uint64_t first = (uint64_t)head + read_group_first(g);  // the group's first entry
    const uint32_t cnt = read_group_entries(entries, g);
    const uint32_t stripe = __builtin_amdgcn_readfirstlane(a.reads[2 * (uint64_t)head]);
    const uint32_t n = update_lane_len(LAY::span_len(args, stripe, span), threadIdx.x);
    if (n == 0) continue;  // no barrier below: the lanes past the shard's end sit the item out
    const uint64_t off = update_span_first(span) + (uint64_t)threadIdx.x * kUpdLaneBytes;
    const typename LAY::At at = LAY::at(args, stripe, off);

    uint32_t rebuilt = 0u;  // bit e: entry first + e is rebuilt
    for (uint32_t e = 0; e < cnt; ++e)
      if (cword(w.cls, first + e) == kReadRebuilt) rebuilt |= 1u << e;

    uint4 acc[NO];
#pragma unroll
    for (int e = 0; e < NO; ++e) acc[e] = make_uint4(0u, 0u, 0u, 0u);
    if (rebuilt != 0u) {
      const uint64_t vrow = run * k, trow = first * k;
      for (uint32_t i0 = 0; i0 < k; i0 += kReadKc) {
        uint4 x[kReadKc];
#pragma unroll
        for (int j = 0; j < kReadKc; ++j)
          if (i0 + j < k) x[j] = ld_lane<VEC>(at.shard(cword(w.valid, vrow + i0 + j)), n);
#pragma unroll
        for (int j = 0; j < kReadKc; ++j) {
          if (!(i0 + j < k)) continue;
          const Sel s0 = make_sel(x[j].x), s1 = make_sel(x[j].y), s2 = make_sel(x[j].z),
                    s3 = make_sel(x[j].w);
          // an opaque offset made anew for every input, and the sums pinned
          // after it: rse_kernels.hip gf8_span says why
          const uint32_t lb = opaque_zero();
#pragma unroll
          for (int e = 0; e < NO; ++e) {
            if (!((rebuilt >> e) & 1u)) continue;
            const Gf8Tab t = ctab(w.tabq, w.tabt2, trow + (uint64_t)e * k + (lb + i0 + j));
            acc[e].x = gf8_mac4(acc[e].x, t, s0);
            acc[e].y = gf8_mac4(acc[e].y, t, s1);
            acc[e].z = gf8_mac4(acc[e].z, t, s2);
            acc[e].w = gf8_mac4(acc[e].w, t, s3);
          }
#pragma unroll
          for (int e = 0; e < NO; ++e) pin(acc[e]);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < NO; ++e) {
      if (!((uint32_t)e < cnt)) continue;
      uint8_t* const row = a.out + (first + e) * bytes + off;
      if ((rebuilt >> e) & 1u) {
        st_lane<VEC>(row, acc[e], n);
      } else if (cword(w.cls, first + e) == kReadCopied) {
        const uint32_t shard = __builtin_amdgcn_readfirstlane(a.reads[2 * (first + e) + 1]);
        st_lane<VEC>(row, ld_lane<VEC>(at.shard(shard), n), n);
      }
    }
  }
}

template <int NO, class LAY>
void launch_one(const typename LAY::Args& args, uint32_t grid, hipStream_t stream) {
  if (LAY::rd(args).vec != 0u)
    hipLaunchKernelGGL((read_kernel<NO, true, LAY>), dim3(grid), dim3(kUpdBlock), 0, stream, args);
  else
    hipLaunchKernelGGL((read_kernel<NO, false, LAY>), dim3(grid), dim3(kUpdBlock), 0, stream, args);
}

constexpr uint32_t kReadPlanGrid = 1024;  // workgroups of the planner at most, in strides over the runs

// The list pass, the layout's planner (`plan`: the kernel, which takes the
// layout's argument block), the read kernel of the layout.
template <class LAY, class Plan>
hipError_t launch_passes(const typename LAY::Args& args, uint32_t grid, hipStream_t stream,
                         Plan plan) {
  const ReadArgs& a = LAY::rd(args);
  if (a.k == 0 || a.p == 0 || a.p > kReadMaxP || a.k + a.p > kReadMaxShards || a.shard_bytes == 0 ||
      a.n_stripes == 0 || a.n_reads == 0 || grid == 0 ||
      reinterpret_cast<uintptr_t>(a.ws) % 16u != 0)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(read_list_kernel, dim3(1), dim3(kPlanBlock), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(plan, dim3(a.n_reads < kReadPlanGrid ? a.n_reads : kReadPlanGrid),
                     dim3(kReadPlanBlock), 0, stream, args);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  const uint32_t rows = read_max_run(a.n_reads, a.k + a.p);  // of the largest group there can be
  if (rows <= 4)
    launch_one<4, LAY>(args, grid, stream);
  else if (rows <= 8)
    launch_one<8, LAY>(args, grid, stream);
  else
    launch_one<16, LAY>(args, grid, stream);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_read(const ReadArgs& a, uint32_t grid, hipStream_t stream) {
  return launch_passes<ReadFlat>(a, grid, stream, read_plan_kernel);
}

hipError_t launch_read_shards(const ReadShardsArgs& a, uint32_t grid, hipStream_t stream) {
  static_assert(sizeof(ReadShardsArgs) <= 4096, "the kernel-argument block");
  // the last block is shorter than the others, and the kernel finds it at n_full
  if (a.tail_bytes >= a.rd.shard_bytes ||
      a.n_full + (a.tail_bytes != 0 ? 1u : 0u) != a.rd.n_stripes)
    return hipErrorInvalidValue;
  return launch_passes<ReadShards>(a, grid, stream, read_shards_plan_kernel);
}

}  // namespace rse
