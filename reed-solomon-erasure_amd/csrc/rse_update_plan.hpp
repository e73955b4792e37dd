// rse_update_plan.hpp -- the arithmetic of one rse_update_flat call: when an
// entry of the update list is in order, where a stripe's run of entries
// starts, how the parity rows are cut into groups, whether the kernel may take
// its 16-byte path, how a shard's bytes are cut into the spans one work item
// covers, and how many workgroups are launched.  No memory access but the
// list's own words.  Plain C++, __host__ __device__ under hipcc: the pre-pass
// (rse_update.hip) calls the predicates the CPU test walks
// (tests/native/update_plan.cpp).  At the end: what rse_update_shards adds
// (tests/native/update_shards_plan.cpp).
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RSE_UPD_HD __host__ __device__ __forceinline__
#else
#define RSE_UPD_HD inline
#endif

namespace rse {

// Which codecs rse_update_flat takes: every GF(2^8) codec, and the GF(2^16)
// codecs of at most 256 shards (coefficients in the GF(2^8) subfield).
inline bool update_in_scope(int field, size_t k, size_t p) {
  return k >= 1 && p >= 1 && k + p <= 256 && (field == 8 || field == 16);
}

// The list: entry u is the words {stripe, data shard} at upd[2u], upd[2u + 1].
// In order: both in range, and after its predecessor lexicographically on the
// raw values -- strictly ascending, so no duplicates, one stripe's entries
// adjacent.
RSE_UPD_HD bool update_in_order(const uint32_t* upd, uint64_t u, uint32_t n_stripes, uint32_t k) {
  const uint32_t stripe = upd[2 * u], shard = upd[2 * u + 1];
  if (stripe >= n_stripes || shard >= k) return false;
  if (u == 0) return true;
  const uint32_t ps = upd[2 * u - 2], ph = upd[2 * u - 1];
  return ps < stripe || (ps == stripe && ph < shard);
}

// Entry u starts a stripe's run of entries.
RSE_UPD_HD bool update_run_head(const uint32_t* upd, uint64_t u) {
  return u == 0 || upd[2 * u] != upd[2 * u - 2];
}

// The p parity rows in groups of kUpdRows: a work item keeps one group's
// sums in registers.
constexpr uint32_t kUpdRows = 16;
RSE_UPD_HD uint32_t update_row_groups(uint32_t p) { return (p + kUpdRows - 1) / kUpdRows; }
RSE_UPD_HD uint32_t update_group_first(uint32_t g) { return g * kUpdRows; }
RSE_UPD_HD uint32_t update_group_rows(uint32_t p, uint32_t g) {
  const uint32_t first = g * kUpdRows;
  return p - first < kUpdRows ? p - first : kUpdRows;
}

// The 16-byte path: every shard of `stripes` and of `new_data` starts on a
// 16-byte boundary and ends on one.
inline bool update_vec(const void* stripes, const void* new_data, uint64_t shard_bytes) {
  return reinterpret_cast<uintptr_t>(stripes) % 16u == 0 &&
         reinterpret_cast<uintptr_t>(new_data) % 16u == 0 && shard_bytes % 16u == 0;
}

// A work item covers span s of its run's shards: bytes
// [s x kUpdSpanBytes, ...) of every shard, 16 per lane of a kUpdBlock workgroup;
// only the last span may be shorter.
constexpr uint32_t kUpdBlock = 256;
constexpr uint32_t kUpdLaneBytes = 16;
constexpr uint64_t kUpdSpanBytes = (uint64_t)kUpdBlock * kUpdLaneBytes;
RSE_UPD_HD uint64_t update_spans(uint64_t shard_bytes) {
  return (shard_bytes + kUpdSpanBytes - 1) / kUpdSpanBytes;
}
RSE_UPD_HD uint64_t update_span_first(uint64_t s) { return s * kUpdSpanBytes; }
RSE_UPD_HD uint64_t update_span_len(uint64_t shard_bytes, uint64_t s) {
  const uint64_t first = s * kUpdSpanBytes;
  return shard_bytes - first < kUpdSpanBytes ? shard_bytes - first : kUpdSpanBytes;
}
// Bytes of lane t within a span of `span_len` bytes: 16, fewer at the end, or 0.
RSE_UPD_HD uint32_t update_lane_len(uint64_t span_len, uint32_t t) {
  const uint64_t first = (uint64_t)t * kUpdLaneBytes;
  if (first >= span_len) return 0;
  return span_len - first < kUpdLaneBytes ? (uint32_t)(span_len - first) : kUpdLaneBytes;
}

// Workgroups of the update kernel, which steps over its (run, span) items in
// grid strides: grid_opt > 0 (RSE_OPT_GRID_X) sets the count outright; else as
// many as the device holds at once (kUpdPerCu per compute unit), and no more
// than the items there can be -- at most one run per entry.
constexpr uint32_t kUpdPerCu = 8;
inline uint32_t update_grid(uint32_t cus, int64_t grid_opt, uint64_t n_updates,
                            uint64_t shard_bytes) {
  if (grid_opt > 0) return grid_opt > 0x7fffffff ? 0x7fffffffu : (uint32_t)grid_opt;
  const uint64_t fill = (uint64_t)(cus > 0 ? cus : 1) * kUpdPerCu;
  const uint64_t spans = update_spans(shard_bytes);
  // n_updates, spans >= 1; the product saturates
  const uint64_t items = n_updates > UINT64_MAX / spans ? UINT64_MAX : n_updates * spans;
  return (uint32_t)(items < fill ? items : fill);
}

// ---- rse_update_shards: a block of every separately allocated shard in the
// place of a stripe (the cut itself is rse_scrub_shards_plan.hpp's).

// The 16-byte path: every one of the n shard pointers and `new_data` start on
// a 16-byte boundary, and a block's bytes and a shard's bytes are multiples of
// 16 -- so every block starts on a boundary and the shorter last block ends on
// one.
inline bool update_shards_vec(const void* const* ptrs, size_t n, const void* new_data,
                              uint64_t block_bytes, uint64_t len_bytes) {
  bool al = reinterpret_cast<uintptr_t>(new_data) % 16u == 0 && block_bytes % 16u == 0 &&
            len_bytes % 16u == 0;
  for (size_t i = 0; i < n; ++i) al = al && reinterpret_cast<uintptr_t>(ptrs[i]) % 16u == 0;
  return al;
}

// Bytes of every shard a run in `block` covers: tail_bytes in the shorter last
// block (block n_full, where tail_bytes != 0), block_bytes in every other.
RSE_UPD_HD uint64_t update_run_bytes(uint64_t block_bytes, uint64_t tail_bytes, uint32_t n_full,
                                     uint32_t block) {
  return tail_bytes != 0 && block == n_full ? tail_bytes : block_bytes;
}

// Items are counted in spans of a full block; span s of a run of run_bytes
// has update_span_len's bytes, or none where the run ends before it (the
// shorter last block): that item is sat out.
RSE_UPD_HD uint64_t update_run_span_len(uint64_t run_bytes, uint64_t s) {
  return update_span_first(s) >= run_bytes ? 0 : update_span_len(run_bytes, s);
}

}  // namespace rse
