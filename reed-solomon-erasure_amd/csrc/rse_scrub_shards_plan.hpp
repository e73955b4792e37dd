// rse_scrub_shards_plan.hpp -- the arithmetic of one rse_scrub_shards call:
// how the shards are cut into blocks, whether the repair sweep may take its
// 16-byte path and whether the block length admits the pre-filter route.  Host
// code without HIP, so that it is tested without a device
// (tests/native/scrub_shards_plan.cpp).
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace rse {

// Shard lengths the bit-sliced kernels code (some of): at least one 4 KiB
// chunk, or exactly 1 or 2 KiB where sub-chunks are on (RSE_OPT_SUB_CHUNKS).
inline bool chunk_kernels_len(uint64_t bytes, bool sub_chunks) {
  return bytes >= 4096 || ((bytes == 1024 || bytes == 2048) && sub_chunks);
}

struct ScrubShardsPlan {
  uint64_t block_len;    // B in elements: min(block_len, len), or len for block_len 0
  uint64_t n_blocks;     // ceil(len / B)
  uint64_t n_full;       // blocks of B elements: n_blocks, or n_blocks - 1
  uint64_t block_bytes;  // B x element size
  uint64_t tail_bytes;   // of the shorter last block; 0 when every block is full
  bool vec;              // every pointer and block_bytes are multiples of 16
  bool len_prefilters;   // block_bytes is a length the check's chunk kernels take, and % 16 == 0
};

// len >= 1 elements per shard, esize bytes per element, n pointers.
inline ScrubShardsPlan scrub_shards_plan(uint64_t len, uint64_t block_len, uint64_t esize,
                                         const void* const* ptrs, size_t n, bool sub_chunks) {
  ScrubShardsPlan pl{};
  pl.block_len = block_len == 0 || block_len > len ? len : block_len;
  pl.n_full = len / pl.block_len;
  const uint64_t tail = len % pl.block_len;
  pl.n_blocks = pl.n_full + (tail != 0 ? 1 : 0);
  pl.block_bytes = pl.block_len * esize;
  pl.tail_bytes = tail * esize;
  bool al = pl.block_bytes % 16u == 0;
  for (size_t i = 0; i < n; ++i) al = al && (reinterpret_cast<uintptr_t>(ptrs[i]) % 16u) == 0;
  pl.vec = al;
  pl.len_prefilters = pl.block_bytes % 16u == 0 && chunk_kernels_len(pl.block_bytes, sub_chunks);
  return pl;
}

// Block b of the plan: its first element and its length in elements.
inline uint64_t scrub_block_first(const ScrubShardsPlan& pl, uint64_t b) { return b * pl.block_len; }
inline uint64_t scrub_block_len(const ScrubShardsPlan& pl, uint64_t len, uint64_t b) {
  const uint64_t first = b * pl.block_len;
  return len - first < pl.block_len ? len - first : pl.block_len;
}

}  // namespace rse
