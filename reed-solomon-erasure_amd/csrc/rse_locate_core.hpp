// rse_locate_core.hpp -- the fast path the kernels of rse_locate_flat
// (rse_locate.hip) and rse_correct_flat (rse_correct.hip) share: one unit of a
// workgroup's sweep forms d = P data ^ parity per byte column with the
// arithmetic of the table check (rse_kernels.hip gf8_span in kCheck mode) and
// hands the lanes with a nonzero d to the caller's slow path.  Then the launch
// sequence the two share (loc_launch).  Included by those two translation units.
#pragma once

#include <type_traits>

#include "rse_device.hpp"
#include "rse_locate.hpp"
#include "rse_locate_plan.hpp"

namespace rse {
namespace locate_core {

constexpr int kLocBlock = 256;
constexpr int kLocKC = 4;  // inputs loaded before any arithmetic (as gf8_span's KC)

// (input, output) tables a workgroup holds: 2048 x 20 B = 40 KiB, four
// workgroups per CU.  NO = 16 past k = 128 rebuilds them per chunk of inputs.
template <int NO>
constexpr uint32_t loc_tabs() {
  return NO == 4 ? 1024u : 2048u;
}

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

// d of the lane's byte column c, packed, out of the accumulators: unrolled
// selects on values (rse_locate_plan.hpp pk_get), so that inside a rolled loop
// over the columns the accumulators stay in VGPRs.
template <int NO, int NW>
__device__ __forceinline__ void loc_column_d(const uint32_t (&acc)[NO][NW], uint32_t c,
                                             uint32_t (&d)[4]) {
  d[0] = d[1] = d[2] = d[3] = 0u;
#pragma unroll
  for (int r = 0; r < NO; ++r) {
    uint32_t v = acc[r][0];
#pragma unroll
    for (int w = 1; w < NW; ++w) {
      const uint32_t aw = acc[r][w];  // read, then select
      v = (c >> 2) == (uint32_t)w ? aw : v;
    }
    d[r >> 2] |= ((v >> ((c & 3u) * 8u)) & 0xFFu) << ((r & 3) * 8);
  }
}

// Where the shards of the stripe a workgroup sweeps lie, and how long they
// are: a layout has shard_bytes, n_vec (the 16-byte vectors of every shard the
// vector body takes) and from(r0, off), a cursor over the shards from r0 on at
// byte offset `off` -- cursor(i) is the address of that byte of shard r0 + i.
//
// Flat, rse_locate_flat's and rse_correct_flat's: the k + p shards of a stripe
// end to end from sbase.
struct LocFlat {
  const uint8_t* sbase;
  uint64_t shard_bytes, n_vec;
  struct Cursor {
    const uint8_t* p;
    uint64_t sb;
    __device__ __forceinline__ const uint8_t* operator()(uint32_t i) const {
      return p + (uint64_t)i * sb;
    }
  };
  __device__ __forceinline__ Cursor from(uint32_t r0, uint64_t off) const {
    return Cursor{sbase + (uint64_t)r0 * shard_bytes + off, shard_bytes};
  }
};

// One pointer per shard, rse_scrub_shards': the stripe is a block of
// shard_bytes of every shard, `boff` bytes into it.  The table is read at a
// wave-uniform index on the fast path (a scalar load) and at the lane's shard
// on the slow path.
struct LocPtrs {
  const uint8_t* const* ptr;
  uint64_t boff, shard_bytes, n_vec;
  struct Cursor {
    const uint8_t* const* q;
    uint64_t o;
    __device__ __forceinline__ const uint8_t* operator()(uint32_t i) const { return q[i] + o; }
  };
  __device__ __forceinline__ Cursor from(uint32_t r0, uint64_t off) const {
    return Cursor{ptr + r0, boff + off};
  }
};

// One unit of a workgroup's sweep: lane t takes NW words of every shard at
// byte offset `off` of the stripe `lay` (NW = 4: a 16-byte vector; NW = 1:
// one byte, for the ragged tail and unaligned stripes).  Called by every
// thread of the workgroup (MULTI rebuilds the tables between barriers).  A
// wave whose d is zero in every lane is done; in any other, the lanes with a
// nonzero d call slow(acc, lay, off) -- the rare path, inlined so that the
// accumulators are never passed through memory.
template <int NO, int NW, bool MULTI, class Lay, class Slow>
__device__ __forceinline__ void loc_unit(const LocateArgs& a, uint4* tq, uint32_t* tt2,
                                         const Lay& lay, uint64_t off, bool valid,
                                         const Slow& slow) {
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
    const auto in = lay.from(c0, off);
    for (uint32_t i0 = 0; i0 < kc; i0 += kLocKC) {
      uint32_t x[kLocKC][NW];
#pragma unroll
      for (int j = 0; j < kLocKC; ++j)
        if (i0 + j < kc) loc_load<NW>(in(i0 + j), valid, x[j]);
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
  const auto par = lay.from(k, off);
#pragma unroll
  for (int r = 0; r < NO; ++r) {
    if (!((uint32_t)r < p)) continue;
    uint32_t x[NW];
    loc_load<NW>(par((uint32_t)r), valid, x);
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      acc[r][w] ^= x[w];
      any |= acc[r][w];
    }
  }
  if (__ballot(any != 0u) == 0ull) return;
  if (any != 0u) slow(acc, lay, off);
}

// Units of 256 lanes in a stripe's sweep: the 16-byte vectors, then the
// byte-wise part.
__device__ __forceinline__ uint64_t loc_units(const LocateArgs& a) {
  return (a.n_vec + kLocBlock - 1) / kLocBlock +
         (a.shard_bytes - a.n_vec * 16u + kLocBlock - 1) / kLocBlock;
}

// Which of a stripe's units a workgroup takes: it is number first() of the
// step() workgroups that share the stripe.  Here for a grid of (workgroups per
// stripe) x (stripes in flight), loc_grid's.
struct LocGridPart {
  __device__ __forceinline__ uint32_t first() const { return blockIdx.x; }
  __device__ __forceinline__ uint32_t step() const { return gridDim.x; }
};

// The sweep of one stripe by one workgroup: its units of 256 lanes, 16-byte
// vectors first, then the byte-wise part.
template <int NO, bool MULTI, class Lay, class Slow, class Part = LocGridPart>
__device__ __forceinline__ void loc_sweep(const LocateArgs& a, uint4* tq, uint32_t* tt2,
                                          const Lay& lay, const Slow& slow,
                                          const Part& part = Part{}) {
  const uint64_t n_vspans = (lay.n_vec + kLocBlock - 1) / kLocBlock;
  const uint64_t tail0 = lay.n_vec * 16u;  // first byte of the byte-wise part
  const uint64_t n_units = n_vspans + (lay.shard_bytes - tail0 + kLocBlock - 1) / kLocBlock;
  for (uint64_t u = part.first(); u < n_units; u += part.step()) {
    if (u < n_vspans) {
      const uint64_t v = u * kLocBlock + threadIdx.x;
      loc_unit<NO, 4, MULTI>(a, tq, tt2, lay, v * 16u, v < lay.n_vec, slow);
    } else {
      const uint64_t b = tail0 + (u - n_vspans) * kLocBlock + threadIdx.x;
      loc_unit<NO, 1, MULTI>(a, tq, tt2, lay, b, b < lay.shard_bytes, slow);
    }
  }
}

// Does every shard of the flat layout start on a 16-byte boundary?
inline bool loc_flat_aligned(const LocateArgs& a) {
  return (reinterpret_cast<uintptr_t>(a.base) % 16u) == 0 && a.shard_bytes % 16u == 0;
}

// Vector width and grid of both passes.  16-byte vectors when every shard
// starts on a 16-byte boundary (al).  A few workgroups per CU over the whole grid,
// and at most four units per workgroup while that keeps the grid small: the
// stripes that take the slow path are then spread over many CUs instead of
// trailing the clean ones on eight workgroups each.
inline dim3 loc_grid(LocateArgs& a, bool al) {
  a.n_vec = al ? a.shard_bytes / 16u : 0;
  const uint64_t units = (a.n_vec + kLocBlock - 1) / kLocBlock +
                         (a.shard_bytes - a.n_vec * 16u + kLocBlock - 1) / kLocBlock;
  const uint32_t gy = (uint32_t)(a.n_stripes < 65535u ? a.n_stripes : 65535u);
  uint64_t gx = 4096u / gy;
  if (gx < units / 4u) gx = units / 4u;
  if (gx > 65536u / gy + 1u) gx = 65536u / gy + 1u;
  if (gx < 1) gx = 1;
  if (gx > units) gx = units;
  return dim3((uint32_t)gx, gy);
}

// The launch sequence of both entries: the accumulators zeroed, the sweep
// kernel, the finalize kernel.  sweep(NO, MULTI, grid) launches the caller's
// sweep kernel for these two integral constants; finalize(blocks) launches its
// finalize kernel, one thread per (stripe, shard) up to 65536 blocks.  Sets
// a.n_vec (loc_grid, by `al`), which the sweep kernel reads.
template <class Sweep, class Finalize>
hipError_t loc_launch(LocateArgs& a, bool al, hipStream_t stream, const Sweep& sweep,
                      const Finalize& finalize) {
  if (!locate_in_scope(8, a.k, a.p) || a.shard_bytes == 0 || a.n_stripes == 0)
    return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(a.acc, 0, a.n_stripes * kLocAccWords * sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  const dim3 grid = loc_grid(a, al);
  const auto with_no = [&](auto no) {
    constexpr int NO = decltype(no)::value;
    constexpr uint32_t KCH = loc_tabs<NO>() / NO;
    if constexpr (KCH < 254u) {  // k <= 254: only NO = 16 can need more than one chunk
      if (a.k > KCH) {
        sweep(no, std::true_type{}, grid);
        return;
      }
    }
    sweep(no, std::false_type{}, grid);
  };
  if (a.p <= 4)
    with_no(std::integral_constant<int, 4>{});
  else if (a.p <= 8)
    with_no(std::integral_constant<int, 8>{});
  else
    with_no(std::integral_constant<int, 16>{});
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  const uint64_t fb = (a.n_stripes * (a.k + a.p) + 255u) / 256u;
  finalize(dim3((uint32_t)(fb < 65536u ? fb : 65536u)));
  return hipGetLastError();
}

}  // namespace locate_core
}  // namespace rse
