// rse_bitslice_ticket.hpp -- a persistent encode / verify body for the compiled
// codecs' 16 KiB chunks whose workgroups claim chunks from a device counter
// instead of walking blockIdx.x + n * gridDim.x (rse_bitslice_core.hpp
// bitslice_body_deep).  Included by rse_bitslice.hip only: the run-time modules'
// source (and with it their cache key) does not change.
//
// Why: with a fixed grid-stride share, the last workgroups of a launch run
// while the resident count falls towards zero, and workgroups that drift
// apart spread the chunks in flight over the whole index space.  Here every
// resident workgroup takes the next unclaimed chunk until none is left.
// Measured (profiles/ticket/): the tail itself costs little, one
// global order of chunks is slower than the grid-stride one, and one
// contiguous run of chunks per XCD (NL = 8) with the cross-chunk prefetch
// below is 2 % faster on large launches.
//
// The arithmetic and the two inputs in flight per lane are bitslice_body_deep's
// (D = 2: a ring of three input slots).  Added to it:
//  - the chunk index comes from `ticket` (kTkWords counter words, zeroed by
//    the host on the launch's stream before the launch): a relaxed agent-scope
//    atomic increment, no fence -- no data passes between workgroups;
//  - the next chunk is claimed at the top of the current one and its first two
//    inputs are loaded during the current chunk's last two inputs, so loads
//    stay in flight through the output phase (the cross-chunk prefetch the deep
//    body lacks);
//  - no workgroup barrier after the prologue.  The four waves share a chunk
//    (lane t takes vectors t, t + 256, ...): lane 0 of wave 0 claims, and
//    publishes the index through a ring of kTkRing LDS slots, each (step + 1)
//    << 32 | index, written two inputs before the waves need it.  A wave spins
//    on the slot only when it is not there yet.  A slot is rewritten kTkRing
//    steps later; wave 0 first checks the other waves' progress words, so a
//    wave that far behind is waited for, not overrun.
//  - NL = 8 (variant 11): workgroup label blockIdx.x % 8 (its XCD under
//    round-robin dispatch) draws from its own eighth of the index space, so
//    each XCD walks a contiguous run; a label that runs dry steals from the
//    next eighths.  NL = 1 (variant 10): one counter over all chunks.
// Every label's first G_l chunks (G_l = its workgroups) are the workgroups'
// first chunks without an atomic; counter value r stands for position G_l + r.
#pragma once

namespace rse {
namespace {

constexpr uint32_t kTkRing = 4;            // published steps kept in LDS
constexpr uint32_t kTkNone = 0xFFFFFFFFu;  // published index: nothing left
constexpr int kTkWords = 8;                // counter words of one launch (NL <= 8)

struct TkShared {
  uint64_t slot[kTkRing];  // (step + 1) << 32 | chunk index
  uint32_t prog[4];        // wave w has read steps < prog[w]
};

// Lane 0 of wave 0's claiming state (the other lanes carry it unused).
template <int NL>
struct TkClaim {
  uint32_t* ticket;
  uint32_t total, grid;
  uint32_t cur, tried;  // label drawn from, labels found dry
  int32_t pending;      // counter value of the claim in flight (first: minus G_l + rank)
  __device__ uint32_t lo(uint32_t l) const { return (uint32_t)((uint64_t)total * l / NL); }
  __device__ uint32_t wgs(uint32_t l) const { return (grid + NL - 1u - l) / NL; }  // G_l
  __device__ void start() {
    cur = blockIdx.x % NL;
    tried = 0;
    pending = (int32_t)(blockIdx.x / NL) - (int32_t)wgs(cur);
  }
  // Relaxed, agent scope.  As the wrapping increment (global_atomic_inc, wrap
  // at 2^32 - 1: a plain + 1 here) rather than atomicAdd, which the compiler
  // rewrites into a wave-level reduction that reads the result back at once:
  // the claim must stay in flight until resolve().
  __device__ int32_t draw() const {
    return (int32_t)__builtin_amdgcn_atomic_inc32(ticket + cur, 0xFFFFFFFFu, __ATOMIC_RELAXED,
                                                  "agent");
  }
  __device__ void issue() {
    if (tried < NL) pending = draw();
  }
  // The chunk of the claim in flight; a dry label moves on to the next one
  // (a wait for the atomic's round trip: at most NL - 1 times per workgroup).
  __device__ uint32_t resolve() {
    while (tried < NL) {
      const uint32_t pos = (uint32_t)((int32_t)wgs(cur) + pending);
      if (pos < lo(cur + 1) - lo(cur)) return lo(cur) + pos;
      cur = (cur + 1u) % NL;
      ++tried;
      if (tried < NL) pending = draw();
    }
    return kTkNone;
  }
};

// Wave 0, lane 0: make step m's chunk index visible to the workgroup.
template <int NL>
__device__ __forceinline__ void tk_publish(TkShared& sh, TkClaim<NL>& cl, uint32_t m) {
  if (threadIdx.x == 0) {
    const uint32_t idx = cl.resolve();
    if (m >= kTkRing) {  // the slot's previous step (m - kTkRing) read by every wave
      for (int w = 1; w < kBsBlock / 64; ++w)
        while (__hip_atomic_load(&sh.prog[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) + kTkRing <=
               m)
          __builtin_amdgcn_s_sleep(1);
    }
    __hip_atomic_store(&sh.slot[m % kTkRing], ((uint64_t)(m + 1u) << 32) | idx, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_WORKGROUP);
  }
}

// Every wave: step m's chunk index (wave-uniform, in an SGPR).
__device__ __forceinline__ uint32_t tk_read(TkShared& sh, uint32_t m) {
  uint64_t v;
  while ((uint32_t)((v = __hip_atomic_load(&sh.slot[m % kTkRing], __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_WORKGROUP)) >>
                    32) != m + 1u)
    __builtin_amdgcn_s_sleep(1);
  if ((threadIdx.x & 63u) == 0)
    __hip_atomic_store(&sh.prog[threadIdx.x >> 6], m + 1u, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_WORKGROUP);
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}

// flag_mismatch (rse_device.hpp) as a global-address-space store.  Its flat
// store, pending at the loop's back edge, makes the compiler drain every load
// (s_waitcnt vmcnt(0)) at the next chunk's first inputs, which here are in
// flight across that edge.
__device__ __forceinline__ void tk_flag(uint32_t* p) { *(gptr<volatile uint32_t>)(p) = 1u; }

struct TkChunk {
  uint64_t cps;
  uint64_t stride;
  __device__ uint64_t off(uint32_t idx) const {
    const uint64_t stripe = idx / cps, chunk = idx - stripe * cps;
    return stripe * stride + chunk * kBsChunk + threadIdx.x * 16u;
  }
};

// Inputs I.. of the chunk at `off` (code_inputs_deep, D = 2, ring of 3 slots:
// input I in slot I % 3), with the workgroup's next chunk found and begun on
// the way:
//  I == k - 4  wave 0 publishes step m + 1 (claimed at the top of this chunk);
//  I == k - 2  every wave reads it (nidx, kTkNone: none);
//  I >= k - 2  the next chunk's inputs 0 and 1 are loaded into slots 0 and 1,
//              where its own pass expects them.  With k % 3 != 0 one or both
//              of those slots still hold this chunk's last inputs: the load
//              is then issued right after the slot has been sliced.
template <class C, int NL, int I>
__device__ __forceinline__ void code_inputs_ticket(uint32_t (&acc)[C::p * 16], u32x4 (&buf)[3][4],
                                                   const CodeArgs& a, uint64_t off,
                                                   const TkChunk& ck, TkShared& sh,
                                                   TkClaim<NL>& cl, uint32_t m, uint32_t& nidx,
                                                   uint64_t& noff) {
  constexpr int K = C::k, R = K % 3;
  static_assert(K >= 6, "the publish point is four inputs before the end");
  if constexpr (I < K) {
    if constexpr (I == K - 4) {
      if (__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) == 0) tk_publish<NL>(sh, cl, m + 1u);
    }
    if constexpr (I == K - 2) {
      nidx = tk_read(sh, m + 1u);
      noff = nidx != kTkNone ? ck.off(nidx) : off;  // none: loaded again, never used
    }
    // the next chunk's input J goes to slot J: free before this slice, or by it?
    constexpr int J = R == 0 ? I - (K - 2) : R == 1 ? (K - 1) - I : I - (K - 2);
    constexpr bool kNext = I >= K - 2;
    constexpr bool kAfter = kNext && I % 3 == J;  // slot J is the one being sliced
    if constexpr (I + 2 < K) load4<true>(buf[(I + 2) % 3], a.in[I + 2] + off);
    if constexpr (kNext && !kAfter) {
      load4<true>(buf[J], a.in[J] + noff);
    }
    __builtin_amdgcn_sched_barrier(0);
    uint32_t pl[16];
    slice<typename C::Field>(buf[I % 3], pl);
    if constexpr (kAfter) {
      __builtin_amdgcn_sched_barrier(0);
      load4<true>(buf[J], a.in[J] + noff);
      __builtin_amdgcn_sched_barrier(0);
    }
    mac_input<C, I, false>(acc, pl, make_int_seq<C::p * 16>{});
#pragma unroll
    for (int q = 0; q < C::p * 16; ++q) asm volatile("" : "+v"(acc[q]));
    code_inputs_ticket<C, NL, I + 1>(acc, buf, a, off, ck, sh, cl, m, nidx, noff);
  }
}

template <class C, int NL>
__device__ __forceinline__ void bitslice_body_ticket(const CodeArgs& a, uint64_t chunks_per_stripe,
                                                     uint32_t* ticket) {
  __shared__ TkShared sh;
  if (threadIdx.x < kTkRing) sh.slot[threadIdx.x] = 0;
  if (threadIdx.x < 4) sh.prog[threadIdx.x] = 0;
  __syncthreads();  // the only barrier: the slots hold no earlier workgroup's steps
  const TkChunk ck{chunks_per_stripe, a.stripe_stride};
  TkClaim<NL> cl{ticket, (uint32_t)(chunks_per_stripe * a.n_stripes), gridDim.x, 0, 0, 0};
  const bool claimer = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) == 0;
  const uint32_t mode = a.mode;
  bool diff = false;
  if (claimer) {
    if (threadIdx.x == 0) cl.start();
    tk_publish<NL>(sh, cl, 0);
  }
  uint32_t idx = tk_read(sh, 0);
  u32x4 buf[3][4];
  uint64_t off = 0;
  if (idx != kTkNone) {
    off = ck.off(idx);
    load4<true>(buf[0], a.in[0] + off);
    load4<true>(buf[1], a.in[1] + off);
  }
  for (uint32_t m = 0; idx != kTkNone; ++m) {
    if (threadIdx.x == 0) cl.issue();  // step m + 1's claim, read four inputs before the end
    uint32_t nidx = kTkNone;
    uint64_t noff = 0;
    uint32_t acc[C::p * 16];
    code_inputs_ticket<C, NL, 0>(acc, buf, a, off, ck, sh, cl, m, nidx, noff);
    store_outputs<C, true>(acc, a, off, mode, diff);
    if (a.per_stripe && diff) {
      tk_flag(a.mismatch + idx / chunks_per_stripe);
      diff = false;
    }
    idx = nidx;
    off = noff;
  }
  if (mode != kStore && diff) tk_flag(a.mismatch);
}

}  // namespace
}  // namespace rse
