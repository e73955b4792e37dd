// rse_correct.hpp -- launch interface of the in-place repair kernels
// (rse_correct.hip) behind rse_correct_flat.
#pragma once

#include "rse_locate.hpp"

namespace rse {

// A stripe's accumulator, kLocAccWords words as rse_locate_flat's: bit r of
// the 8 mask words = a byte of shard r was stored; then two 64-bit counters,
// bytes stored and columns left undecodable; then the word that says the
// stripe was skipped (more than p shards erased).
constexpr uint32_t kCorAccStored = 8;   // words 8, 9
constexpr uint32_t kCorAccBad = 10;     // words 10, 11
constexpr uint32_t kCorAccSkipped = 12;

struct CorrectArgs {
  LocateArgs loc;          // the stripes (written in place), the plan, the accumulators
  const uint8_t* present;  // n_stripes x (k + p), 0 = erased; null: nothing is erased
};

// rse_scrub_shards' stripes: one pointer per shard, and a stripe is a block of
// cor.loc.shard_bytes of every shard -- block s of shard r starts at
// ptr[r] + s * cor.loc.shard_bytes.  cor.loc.base is not used, and
// cor.loc.n_stripes counts the blocks, the shorter last one included.  The
// table travels in the kernel arguments (2,040 B of the 4 KiB block): nothing
// to copy, nothing whose lifetime outlasts the call.
constexpr uint32_t kCorMaxShards = 255;
struct CorrectShardsArgs {
  CorrectArgs cor;
  uint64_t tail_bytes;  // of the last block where it is shorter than the others, else 0
  uint32_t vec;         // the 16-byte path: every pointer and the block bytes are multiples of 16
  const uint8_t* ptr[kCorMaxShards];
};

// The repairing pass over every stripe, then the pass that turns the
// accumulators into status (n_stripes), changed (n_stripes x (k + p), nullable)
// and counts (n_stripes x 2, nullable).
hipError_t launch_correct(const CorrectArgs& a, uint8_t* status, uint8_t* changed,
                          uint32_t* counts, hipStream_t stream);

// rse_scrub_flat's pre-filter route.  The same two passes, the first over the
// stripes list[0 .. *n_list) only (both device memory, read on the device; the
// list's stripes are distinct and below a.loc.n_stripes): every other stripe
// comes out CLEAN with nothing changed.
hipError_t launch_correct_list(const CorrectArgs& a, const uint32_t* list, const uint32_t* n_list,
                               uint8_t* status, uint8_t* changed, uint32_t* counts,
                               hipStream_t stream);

// Both of the above for separately allocated shards: the blocks
// list[0 .. *n_list), or every block when list is null.
hipError_t launch_correct_shards(const CorrectShardsArgs& a, const uint32_t* list,
                                 const uint32_t* n_list, uint8_t* status, uint8_t* changed,
                                 uint32_t* counts, hipStream_t stream);

// Ascending into list[0 .. *count): the stripes with a nonzero word in `words`
// (n_stripes), a zero flag in their row of `present` (n_stripes x n) or a
// nonzero `status` (n_stripes); each of the three, and list and count, may be
// null.  Entries from *count on are not written.  n_stripes < 2^32.
hipError_t launch_scrub_compact(const uint32_t* words, const uint8_t* present, uint32_t n,
                                const uint8_t* status, uint64_t n_stripes, uint32_t* list,
                                uint32_t* count, hipStream_t stream);

}  // namespace rse
