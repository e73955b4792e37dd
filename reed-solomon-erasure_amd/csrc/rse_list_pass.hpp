// rse_list_pass.hpp -- device code the list entries share (rse_update.hip,
// rse_read.hip): the one-workgroup walk over a sorted device list of
// {stripe, shard} entries, and a lane's 16 bytes of a span on the vector and on
// the byte route.
#pragma once

#include "rse_device.hpp"
#include "rse_update_plan.hpp"

namespace rse {
namespace {

constexpr int kPlanBlock = 1024, kPlanWaves = kPlanBlock / 64;
constexpr uint32_t kNoOffender = 0xFFFFFFFFu;  // n <= 2^32 - 1: no entry has this index

// One workgroup of kPlanBlock threads walks the list once: the in-order
// predicate of every entry (rse_update_plan.hpp; `bound` is what a shard index
// stays below) with the lowest offender kept, and the run heads compacted in
// ascending order into heads[0 .. runs).  True in thread 0 alone, which gets the
// first offender (kNoOffender: the list is in order) and the number of runs.
__device__ __forceinline__ bool list_pass(const uint32_t* list, uint32_t n, uint32_t n_stripes,
                                          uint32_t bound, uint32_t* heads, uint32_t& first,
                                          uint32_t& runs) {
  __shared__ uint32_t s_wave[2][kPlanWaves];
  __shared__ uint32_t s_bad;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) s_bad = kNoOffender;
  uint32_t bad = kNoOffender, base = 0u;
  // a head's place in the list: the heads of the trips before (base), of the
  // waves before (through LDS, two buffers so that a trip needs one barrier)
  // and of the lanes below
  for (uint64_t u0 = 0, trip = 0; u0 < n; u0 += kPlanBlock, ++trip) {
    const uint64_t u = u0 + threadIdx.x;
    bool head = false;
    if (u < n) {
      if (bad == kNoOffender && !update_in_order(list, u, n_stripes, bound)) bad = (uint32_t)u;
      head = update_run_head(list, u);
    }
    const unsigned long long heads_here = __ballot(head);
    if (lane == 0) s_wave[trip & 1u][wave] = (uint32_t)__popcll(heads_here);
    __syncthreads();
    uint32_t at = base;
#pragma unroll
    for (int w = 0; w < kPlanWaves; ++w) {
      const uint32_t v = s_wave[trip & 1u][w];
      base += v;
      if ((uint32_t)w < wave) at += v;
    }
    if (head) heads[at + (uint32_t)__popcll(heads_here & ((1ull << lane) - 1ull))] = (uint32_t)u;
  }
  if (bad != kNoOffender) atomicMin(&s_bad, bad);
  __syncthreads();
  first = s_bad;
  runs = base;
  return threadIdx.x == 0;
}

// A lane's n <= 16 bytes at p: one 16-byte access on the vector path (n is 16
// there), byte by byte otherwise, the bytes past n read as zero and not stored.
template <bool VEC>
__device__ __forceinline__ uint4 ld_lane(const uint8_t* p, uint32_t n) {
  if constexpr (VEC) {
    return ld16(p);
  } else {
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t b = 0; b < kUpdLaneBytes; ++b)
      if (b < n) w[b / 4] |= (uint32_t)((gptr<const uint8_t>)p)[b] << (8u * (b % 4));
    return make_uint4(w[0], w[1], w[2], w[3]);
  }
}
template <bool VEC>
__device__ __forceinline__ void st_lane(uint8_t* p, uint4 v, uint32_t n) {
  if constexpr (VEC) {
    st16(p, v);
  } else {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (uint32_t b = 0; b < kUpdLaneBytes; ++b)
      if (b < n) ((gptr<uint8_t>)p)[b] = (uint8_t)(w[b / 4] >> (8u * (b % 4)));
  }
}

}  // namespace
}  // namespace rse
