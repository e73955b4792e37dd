// rse_update.hip -- rse_update_flat: data shards rewritten in place and the
// parity patched by the delta, parity_j ^= M[k+j][i] * (old_i ^ new_i)
// (encode_single's accumulation, core.rs:545-562, applied to a difference).
//
// Two launches on the caller's stream.  update_plan_kernel, one workgroup,
// walks the list once (list_pass, rse_list_pass.hpp): the in-order predicate of
// every entry (rse_update_plan.hpp) with the lowest offender kept, the run heads
// compacted in ascending order into the workspace, the verdict into the
// workspace and into the caller's `result`.  update_kernel exits at once on a
// rejected list -- no address is ever formed from an entry that is not in order
// -- and else
// steps in grid strides over (run, span) items: one stripe's entries, 4 KiB of
// every shard they name, 16 bytes per lane.  The list is strictly ascending,
// so a run is its stripe's only writer: no atomics on shard bytes.
//
// Per item the lane loads its 16 bytes of every parity row of the group into
// the accumulators, then for every entry of the run loads old and new, stores
// new over old (same lane, same address), and adds M[k+r][shard] * (old ^ new)
// to every row with the table multiply of rse_kernels.hip (gf8_mac4); then the
// rows are stored.  The tables of a group's rows x k coefficients are built
// per workgroup into LDS from the codec's parity rows on the device.  More
// than kUpdRows parity rows are taken group by group, the groups outermost so
// that a workgroup builds each group's tables once: an item is always the same
// workgroup's and lane's, which re-reads old and new in every group's pass and
// stores the data shard in the last one, so every pass sees the old bytes.
//
// A GF(2^16) codec of at most 256 shards has its coefficients in the GF(2^8)
// subfield, where a constant multiplies each byte of an element by itself
// (rse_codec::kfield): the same kernel over 2 x shard_len bytes.
//
// rse_update_shards is the same two launches with another address rule for
// update_kernel (UpdShards below): one pointer per shard from the kernel
// arguments, a block of columns in the place of a stripe, a shorter last block.
#include "rse_update.hpp"

#include "rse_list_pass.hpp"
#include "rse_update_plan.hpp"

namespace rse {
namespace {

__global__ __launch_bounds__(kPlanBlock) void update_plan_kernel(UpdateArgs a) {
  uint32_t first, runs;
  if (list_pass(a.updates, a.n_updates, a.n_stripes, a.k, a.ws + kUpdWsList, first, runs)) {
    const bool rejected = first != kNoOffender;
    a.ws[kUpdWsStatus] = rejected ? RSE_UPDATE_REJECTED : RSE_UPDATE_APPLIED;
    a.ws[kUpdWsRuns] = runs;
    a.result[0] = rejected ? RSE_UPDATE_REJECTED : RSE_UPDATE_APPLIED;
    a.result[1] = rejected ? first : runs;  // accepted: a run per touched stripe
  }
}

// Where an item's bytes lie: the addressing policy of update_kernel.  A layout
// names the call's argument block, says how many bytes span s of a run has (0:
// the item is sat out), and makes a cursor per item for the lane's offset `off`
// into the run's stripe: the lane's address in data shard i, and in parity row
// r of the group whose first row is row0.
//
// The flat layout: base + stripe x (k + p) x bytes + shard x bytes.
struct UpdFlat {
  using Args = UpdateArgs;
  static __host__ __device__ __forceinline__ const UpdateArgs& upd(const Args& a) { return a; }
  static __device__ __forceinline__ uint64_t span_len(const Args& a, uint32_t, uint64_t span) {
    return update_span_len(a.shard_bytes, span);
  }
  struct At {
    uint8_t *sbase, *par;
    uint64_t bytes;
    __device__ __forceinline__ uint8_t* data(uint32_t i) const { return sbase + (uint64_t)i * bytes; }
    __device__ __forceinline__ uint8_t* row(uint32_t r) const { return par + (uint64_t)r * bytes; }
  };
  static __device__ __forceinline__ At at(const Args& a, uint32_t stripe, uint64_t off,
                                          uint32_t row0) {
    const uint64_t bytes = a.shard_bytes;
    uint8_t* const sbase = a.base + (uint64_t)stripe * (a.k + a.p) * bytes + off;
    return At{sbase, sbase + (uint64_t)(a.k + row0) * bytes, bytes};
  }
};

// Separately allocated shards (rse_update_shards): ptr[shard] + block x block
// bytes, the pointers read from the kernel arguments.  Shard and row indices are
// the same in every lane, so a pointer is a scalar load.  A run in the shorter
// last block has the tail's bytes: fewer spans, a shorter last lane.
struct UpdShards {
  using Args = UpdateShardsArgs;
  static __host__ __device__ __forceinline__ const UpdateArgs& upd(const Args& a) {
    return a.upd;
  }
  static __device__ __forceinline__ uint64_t span_len(const Args& a, uint32_t block,
                                                      uint64_t span) {
    return update_run_span_len(
        update_run_bytes(a.upd.shard_bytes, a.tail_bytes, a.n_full, block), span);
  }
  struct At {
    uint8_t* const* ptr;
    uint64_t o;
    uint32_t par0;
    __device__ __forceinline__ uint8_t* data(uint32_t i) const { return ptr[i] + o; }
    __device__ __forceinline__ uint8_t* row(uint32_t r) const { return ptr[par0 + r] + o; }
  };
  static __device__ __forceinline__ At at(const Args& a, uint32_t block, uint64_t off,
                                          uint32_t row0) {
    return At{a.ptr, (uint64_t)block * a.upd.shard_bytes + off, a.upd.k + row0};
  }
};

// TABS: tables the LDS image holds, at least group rows x k.  NO: parity rows
// a lane accumulates, at least the group's.  LAY: UpdFlat or UpdShards; below,
// "stripe" and "shard bytes" are a block and a full block's bytes for the
// latter.
template <int TABS, int NO, bool VEC, class LAY>
__global__ __launch_bounds__(kUpdBlock) void update_kernel(typename LAY::Args args) {
  __shared__ uint4 tq[TABS];
  __shared__ uint32_t tt2[TABS];
  const UpdateArgs& a = LAY::upd(args);
  if (a.ws[kUpdWsStatus] != RSE_UPDATE_APPLIED) return;  // rejected: nothing is read or written

  const uint32_t k = a.k, p = a.p, n_updates = a.n_updates;
  const uint64_t bytes = a.shard_bytes;
  const uint64_t n_spans = update_spans(bytes);
  const uint64_t n_items = (uint64_t)a.ws[kUpdWsRuns] * n_spans;
  const uint32_t n_groups = update_row_groups(p);

  for (uint32_t g = 0; g < n_groups; ++g) {
    const uint32_t row0 = update_group_first(g), rows = update_group_rows(p, g);
    const bool last = g + 1 == n_groups;
    if (g != 0) __syncthreads();  // the group before is done with its tables
    // table (r, i) of the group at index r * k + i
    for (uint32_t t = threadIdx.x; t < rows * k; t += kUpdBlock)
      write_tab(tq, tt2, t, make_gf8_tab(a.coef[(size_t)row0 * k + t]));
    __syncthreads();

    for (uint64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
      const uint64_t run = item / n_spans, span = item % n_spans;
      const uint32_t head = __builtin_amdgcn_readfirstlane(a.ws[kUpdWsList + run]);
      const uint32_t stripe = __builtin_amdgcn_readfirstlane(a.updates[2 * (uint64_t)head]);
      const uint32_t n = update_lane_len(LAY::span_len(args, stripe, span), threadIdx.x);
      if (n == 0) continue;  // no barrier below: the lanes past the shard's end sit the item out
      const uint64_t off = update_span_first(span) + (uint64_t)threadIdx.x * kUpdLaneBytes;
      const typename LAY::At at = LAY::at(args, stripe, off, row0);

      uint4 acc[NO];
#pragma unroll
      for (int r = 0; r < NO; ++r) {
        acc[r] = make_uint4(0u, 0u, 0u, 0u);
        if ((uint32_t)r < rows) acc[r] = ld_lane<VEC>(at.row(r), n);
      }
      for (uint32_t e = head; e < n_updates; ++e) {
        if (__builtin_amdgcn_readfirstlane(a.updates[2 * (uint64_t)e]) != stripe) break;
        const uint32_t shard = __builtin_amdgcn_readfirstlane(a.updates[2 * (uint64_t)e + 1]);
        uint8_t* const dst = at.data(shard);
        const uint4 old = ld_lane<VEC>(dst, n);
        const uint4 nw = ld_lane<VEC>(a.new_data + (uint64_t)e * bytes + off, n);
        if (last) st_lane<VEC>(dst, nw, n);
        const Sel s0 = make_sel(old.x ^ nw.x), s1 = make_sel(old.y ^ nw.y),
                  s2 = make_sel(old.z ^ nw.z), s3 = make_sel(old.w ^ nw.w);
        // an opaque LDS offset made anew for every entry, and the sums pinned
        // after it: rse_kernels.hip gf8_span says why
        const uint32_t lb = opaque_zero();
#pragma unroll
        for (int r = 0; r < NO; ++r) {
          if (!((uint32_t)r < rows)) continue;
          const Gf8Tab t = read_tab(tq, tt2, lb + r * k + shard);
          acc[r].x = gf8_mac4(acc[r].x, t, s0);
          acc[r].y = gf8_mac4(acc[r].y, t, s1);
          acc[r].z = gf8_mac4(acc[r].z, t, s2);
          acc[r].w = gf8_mac4(acc[r].w, t, s3);
        }
#pragma unroll
        for (int r = 0; r < NO; ++r) pin(acc[r]);
      }
#pragma unroll
      for (int r = 0; r < NO; ++r)
        if ((uint32_t)r < rows) st_lane<VEC>(at.row(r), acc[r], n);
    }
  }
}

template <int TABS, int NO, class LAY>
void launch_one(const typename LAY::Args& args, uint32_t grid, hipStream_t stream) {
  if (LAY::upd(args).vec != 0u)
    hipLaunchKernelGGL((update_kernel<TABS, NO, true, LAY>), dim3(grid), dim3(kUpdBlock), 0, stream,
                       args);
  else
    hipLaunchKernelGGL((update_kernel<TABS, NO, false, LAY>), dim3(grid), dim3(kUpdBlock), 0,
                       stream, args);
}

// LDS images: the small one keeps eight workgroups on a compute unit, the
// large one (a group of 16 rows of a codec with k up to 255) one or two.
constexpr int kTabsSmall = 1024, kTabsLarge = 4096;

// The plan kernel over the list, then the update kernel of the layout.
template <class LAY>
hipError_t launch_both(const typename LAY::Args& args, uint32_t grid, hipStream_t stream) {
  const UpdateArgs& a = LAY::upd(args);
  if (a.k == 0 || a.p == 0 || a.k + a.p > 256 || a.shard_bytes == 0 || a.n_stripes == 0 ||
      a.n_updates == 0 || grid == 0)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(update_plan_kernel, dim3(1), dim3(kPlanBlock), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const uint32_t rows = a.p < kUpdRows ? a.p : kUpdRows;  // of the largest group
  if (rows * a.k > (uint32_t)kTabsSmall)
    launch_one<kTabsLarge, 16, LAY>(args, grid, stream);
  else if (rows <= 4)
    launch_one<kTabsSmall, 4, LAY>(args, grid, stream);
  else if (rows <= 8)
    launch_one<kTabsSmall, 8, LAY>(args, grid, stream);
  else
    launch_one<kTabsSmall, 16, LAY>(args, grid, stream);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_update(const UpdateArgs& a, uint32_t grid, hipStream_t stream) {
  return launch_both<UpdFlat>(a, grid, stream);
}

hipError_t launch_update_shards(const UpdateShardsArgs& a, uint32_t grid, hipStream_t stream) {
  static_assert(sizeof(UpdateShardsArgs) <= 4096, "the kernel-argument block");
  // the last block is shorter than the others, and the kernel finds it at n_full
  if (a.tail_bytes >= a.upd.shard_bytes ||
      a.n_full + (a.tail_bytes != 0 ? 1u : 0u) != a.upd.n_stripes)
    return hipErrorInvalidValue;
  return launch_both<UpdShards>(a, grid, stream);
}

}  // namespace rse
