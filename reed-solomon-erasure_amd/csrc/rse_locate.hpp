// rse_locate.hpp -- launch interface of the error-locating kernels
// (rse_locate.hip) behind rse_locate_flat.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rse {

// Words of a stripe's accumulator: bit r of the 8 mask words = shard r is bad
// in some column, word 8 nonzero = some column is undecodable (16 words: one
// 64-byte line per stripe).
constexpr uint32_t kLocAccWords = 16;

struct LocateArgs {
  const uint8_t* base;    // stripe 0, shard 0 (flat layout: k + p shards end to end; not
                          // used where the shards come as pointers, CorrectShardsArgs)
  uint64_t shard_bytes;
  uint64_t n_vec;         // 16-byte vectors of every shard the vector body takes
  uint64_t n_stripes;
  uint32_t k, p;
  const uint8_t* consts;  // the plan on the device (rse_locate_plan.hpp locate_consts)
  uint32_t* acc;          // n_stripes x kLocAccWords, zeroed
};

// The locating pass over every stripe, then the pass that turns the
// accumulators into present (n_stripes x (k + p)) and status (n_stripes).
hipError_t launch_locate(const LocateArgs& a, uint8_t* present, uint8_t* status,
                         hipStream_t stream);

}  // namespace rse
