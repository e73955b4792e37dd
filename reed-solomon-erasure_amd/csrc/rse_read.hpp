// rse_read.hpp -- launch interface of the degraded-read kernels (rse_read.hip)
// behind rse_read_flat and rse_read_shards.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rse_hip.h"
#include "rse_read_plan.hpp"

namespace rse {

// The call's workspace, one allocation.  Words first: the verdict
// (RSE_READ_SERVED / RSE_READ_REJECTED), the number of runs, then
//   heads  n_reads + 1 words: the run heads in ascending order, n_reads after them
//   cls    n_reads words: every entry's class (RSE_READ_*), as `status` has it
//   valid  n_reads x k words: a run's valid set, for a run that rebuilds
// and then the multiply tables of every (entry, input) of the rebuilt entries,
// as the kernels read them (Gf8Tab, rse_device.hpp): its first four words in
//   tabq   n_reads x k x 16 bytes, on a 16-byte boundary
// and the fifth in
//   tabt2  n_reads x k words.
constexpr uint32_t kReadWsStatus = 0, kReadWsRuns = 1, kReadWsHeads = 2;
struct ReadWs {
  size_t cls, valid, tabq, tabt2;  // byte offsets
  size_t bytes;
};
__host__ __device__ inline ReadWs read_ws(uint64_t n_reads, uint32_t k) {
  ReadWs w;
  w.cls = (kReadWsHeads + n_reads + 1) * sizeof(uint32_t);
  w.valid = w.cls + n_reads * sizeof(uint32_t);
  w.tabq = (w.valid + n_reads * k * sizeof(uint32_t) + 15u) / 16u * 16u;
  w.tabt2 = w.tabq + n_reads * k * 16u;
  w.bytes = w.tabt2 + n_reads * k * sizeof(uint32_t);
  return w;
}

struct ReadArgs {
  const uint8_t* base;     // stripe 0, shard 0 (flat layout: k + p shards end to end); only read
  uint64_t shard_bytes;
  uint32_t n_stripes;
  uint32_t k, p;
  uint32_t n_reads;
  const uint8_t* present;  // n_stripes x (k + p) flags, or nullptr: all present
  const uint32_t* reads;   // n_reads x {stripe, shard}
  uint8_t* out;            // n_reads x shard_bytes
  uint8_t* status;         // n_reads
  uint32_t* result;        // the caller's 2 words
  const uint8_t* coef;     // the parity rows on the device, p x k bytes
  uint8_t* ws;             // read_ws(n_reads, k).bytes, 16-byte aligned
  uint32_t vec;            // the 16-byte path (rse_read_plan.hpp read_vec)
};

// The list pass, the run planner and the read kernel over `grid` workgroups
// (rse_read_plan.hpp read_grid); the last two do nothing for a rejected list.
hipError_t launch_read(const ReadArgs& a, uint32_t grid, hipStream_t stream);

// rse_read_shards' layout: one pointer per shard, and a block of
// rd.shard_bytes of every shard in the place of a stripe -- block b of shard r
// starts at ptr[r] + b * rd.shard_bytes, row u of `out` at u * rd.shard_bytes.
// rd.base is not used, and rd.n_stripes counts the blocks, the shorter last one
// included.  ptr[r] == nullptr: shard r has no buffer; the planner asks the
// table itself (rse_read_plan.hpp ReadNullShards), so nothing else marks it.
// The table travels in the kernel arguments (2 KiB of the 4 KiB block): nothing
// to copy, nothing whose lifetime outlasts the call.
struct ReadShardsArgs {
  ReadArgs rd;
  uint64_t tail_bytes;  // of the last block where it is shorter than the others, else 0
  uint32_t n_full;      // blocks of rd.shard_bytes: the index of the shorter last block
  const uint8_t* ptr[kReadMaxShards];
};

// The same three launches; the list pass reads a.rd alone.
hipError_t launch_read_shards(const ReadShardsArgs& a, uint32_t grid, hipStream_t stream);

}  // namespace rse
