// rse_update.hpp -- launch interface of the small-write kernels
// (rse_update.hip) behind rse_update_flat and rse_update_shards.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rse_hip.h"

namespace rse {

// Words of the call's workspace before the run list: the verdict
// (RSE_UPDATE_APPLIED / RSE_UPDATE_REJECTED) and the number of runs.
constexpr uint32_t kUpdWsStatus = 0, kUpdWsRuns = 1, kUpdWsList = 2;

struct UpdateArgs {
  uint8_t* base;            // stripe 0, shard 0 (flat layout: k + p shards end to end)
  uint64_t shard_bytes;
  uint32_t n_stripes;
  uint32_t k, p;
  uint32_t n_updates;
  const uint32_t* updates;  // n_updates x {stripe, data shard}
  const uint8_t* new_data;  // n_updates x shard_bytes
  const uint8_t* coef;      // the parity rows on the device, p x k bytes
  uint32_t* ws;             // kUpdWsList + n_updates words, written by the plan kernel
  uint32_t* result;         // the caller's 2 words
  uint32_t vec;             // the 16-byte path (rse_update_plan.hpp update_vec)
};

// The plan kernel over the list, then the update kernel over `grid`
// workgroups (rse_update_plan.hpp update_grid), which does nothing for a
// rejected list.
hipError_t launch_update(const UpdateArgs& a, uint32_t grid, hipStream_t stream);

// rse_update_shards' layout: one pointer per shard, and a block of
// upd.shard_bytes of every shard in the place of a stripe -- block b of shard r
// starts at ptr[r] + b * upd.shard_bytes, row u of new_data at
// u * upd.shard_bytes.  upd.base is not used, and upd.n_stripes counts the
// blocks, the shorter last one included.  The table travels in the kernel
// arguments (2 KiB of the 4 KiB block): nothing to copy, nothing whose lifetime
// outlasts the call.
constexpr uint32_t kUpdMaxShards = 256;
struct UpdateShardsArgs {
  UpdateArgs upd;
  uint64_t tail_bytes;  // of the last block where it is shorter than the others, else 0
  uint32_t n_full;      // blocks of upd.shard_bytes: the index of the shorter last block
  uint8_t* ptr[kUpdMaxShards];
};

// The same two launches; the plan kernel reads a.upd alone.
hipError_t launch_update_shards(const UpdateShardsArgs& a, uint32_t grid, hipStream_t stream);

}  // namespace rse
