// ticket_probe.hip -- occupancy timeline of encode's access shape (10 shards
// read, 4 written, 16 KiB chunks, 256 lanes, trivial XOR arithmetic) under two
// ways of handing chunks to workgroups:
//   stride   workgroup b takes chunks b, b + G, b + 2G, ... (the bit-sliced
//            kernels' grid-stride loop), at grid G
//   ticket   every workgroup takes the next unclaimed chunk from a device
//            counter (claimed one chunk ahead), at the resident grid
// Every workgroup records the 100 MHz wall clock at its first load and after
// its last store has completed, and every chunk the clock when it was begun
// and when its stores had been issued.  From those the host prints the
// resident workgroup count and the width of the window of chunks in flight
// against time, the length of the tail (from the last moment every launched
// or resident workgroup was still running to the end) and the rate.
// The probe's ticket loop publishes the next index through LDS behind one
// workgroup barrier per chunk; the library kernel (rse_bitslice_ticket.hpp)
// has none.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/ticket_probe.hip -o tools/ticket_probe
//   tools/ticket_probe [stripes=512]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x)                                                                 \
  do {                                                                        \
    hipError_t e = (x);                                                       \
    if (e != hipSuccess) {                                                    \
      fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e)); \
      exit(1);                                                                \
    }                                                                         \
  } while (0)

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
constexpr int NR = 10, NW = 4;
constexpr uint64_t kChunkVec = 1024;  // 16 KiB of one shard
// Dynamic LDS per workgroup, unused: it holds the probe (92 VGPRs) to the three
// workgroups per CU of the library kernel (163 VGPRs) on a 160 KiB CU.
constexpr size_t kLdsPad = 48 << 10;

template <bool TICKET>
__global__ __launch_bounds__(256, 3) void probe_k(u32x4* base, uint64_t nvec, uint32_t stripes,
                                                  uint32_t* counter, uint64_t* wg_t,
                                                  uint64_t* ck_t) {
  __shared__ uint32_t nxt[2];
  const uint64_t cps = nvec / kChunkVec;
  const uint32_t total = (uint32_t)(cps * stripes);
  uint32_t idx = blockIdx.x, step = 0, pend = 0;
  const uint64_t t0 = wall_clock64();
  while (idx < total) {
    if (TICKET && threadIdx.x == 0)
      pend = __builtin_amdgcn_atomic_inc32(counter, 0xFFFFFFFFu, __ATOMIC_RELAXED, "agent");
    const uint64_t ts = wall_clock64();
    const uint64_t stripe = idx / cps, chunk = idx - stripe * cps;
    u32x4* sb = base + stripe * (NR + NW) * nvec + chunk * kChunkVec + threadIdx.x;
    u32x4 acc[NW][4];
#pragma unroll
    for (int r = 0; r < NW; ++r)
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[r][u] = (u32x4){(unsigned)r, 1u, 2u, 3u};
#pragma unroll 2  // two inputs in flight, as the library kernel; more spills
    for (int i = 0; i < NR; ++i) {
      u32x4 x[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) x[u] = __builtin_nontemporal_load(sb + i * nvec + u * 256);
#pragma unroll
      for (int r = 0; r < NW; ++r)
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[r][u] ^= (x[u] << (unsigned)((r + i) & 7));
    }
#pragma unroll
    for (int r = 0; r < NW; ++r)
#pragma unroll
      for (int u = 0; u < 4; ++u)
        __builtin_nontemporal_store(acc[r][u], sb + (NR + r) * nvec + u * 256);
    uint32_t nidx;
    if (TICKET) {
      // slot step & 1 is rewritten two barriers after it was read
      if (threadIdx.x == 0) nxt[step & 1u] = gridDim.x + pend;
      __syncthreads();
      nidx = nxt[step & 1u];
    } else {
      nidx = idx + gridDim.x;
    }
    if (threadIdx.x == 0) {
      ck_t[2 * (uint64_t)idx] = ts;
      ck_t[2 * (uint64_t)idx + 1] = wall_clock64();
    }
    idx = nidx;
    ++step;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (threadIdx.x == 0) {
    wg_t[2 * blockIdx.x] = t0;
    wg_t[2 * blockIdx.x + 1] = wall_clock64();
  }
}

struct Run {
  const char* name;
  bool ticket;
  uint32_t grid;
};

int main(int argc, char** argv) {
  const uint32_t stripes = argc > 1 ? (uint32_t)atoi(argv[1]) : 512;
  const uint64_t nvec = (16ull << 20) / 16;
  const uint64_t cps = nvec / kChunkVec, total = cps * stripes;
  const size_t bytes = (size_t)stripes * (NR + NW) * nvec * 16;
  int dev = 0, cus = 0, per_cu_s = 0, per_cu_t = 0, khz = 0;
  CK(hipGetDevice(&dev));
  CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  CK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev));
  CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_s, probe_k<false>, 256, kLdsPad));
  CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_t, probe_k<true>, 256, kLdsPad));
  const uint32_t res_s = (uint32_t)(cus * per_cu_s), res_t = (uint32_t)(cus * per_cu_t);
  printf("%u stripes of 10+4 x 16 MiB: %lu chunks of 16 KiB, %.1f GiB; %d CUs, resident "
         "workgroups %u (stride) %u (ticket); wall clock %d kHz\n",
         stripes, (unsigned long)total, bytes / 1073741824.0, cus, res_s, res_t, khz);
  u32x4* buf;
  uint32_t* counter;
  uint64_t *wg_t, *ck_t;
  const uint32_t max_grid = 8192;
  CK(hipMalloc(&buf, bytes));
  CK(hipMemset(buf, 0x5A, bytes));
  CK(hipMalloc(&counter, 64));
  CK(hipMalloc(&wg_t, max_grid * 16));
  CK(hipMalloc(&ck_t, total * 16));
  const Run runs[] = {{"stride", false, 4096},  {"stride", false, res_s}, {"stride", false, 5 * res_s},
                      {"stride", false, 8192},  {"ticket", true, res_t},  {"ticket", true, 2 * res_t}};
  std::vector<uint64_t> wg(2 * max_grid), ck(2 * total);
  const double us = 1e3 / khz;  // per tick
  for (const Run& r : runs) {
    if (r.grid > max_grid) continue;
    float ms = 0;
    for (int rep = 0; rep < 2; ++rep) {  // the second run is the one read
      CK(hipMemset(counter, 0, 64));
      CK(hipMemset(wg_t, 0, max_grid * 16));
      hipEvent_t a, b;
      CK(hipEventCreate(&a));
      CK(hipEventCreate(&b));
      CK(hipEventRecord(a));
      if (r.ticket)
        hipLaunchKernelGGL(probe_k<true>, dim3(r.grid), dim3(256), kLdsPad, 0, buf, nvec, stripes, counter,
                           wg_t, ck_t);
      else
        hipLaunchKernelGGL(probe_k<false>, dim3(r.grid), dim3(256), kLdsPad, 0, buf, nvec, stripes,
                           counter, wg_t, ck_t);
      CK(hipGetLastError());
      CK(hipEventRecord(b));
      CK(hipEventSynchronize(b));
      CK(hipEventElapsedTime(&ms, a, b));
      CK(hipEventDestroy(a));
      CK(hipEventDestroy(b));
    }
    CK(hipMemcpy(wg.data(), wg_t, (size_t)r.grid * 16, hipMemcpyDeviceToHost));
    CK(hipMemcpy(ck.data(), ck_t, total * 16, hipMemcpyDeviceToHost));
    uint64_t t_first = ~0ull, t_last = 0;
    for (uint32_t b = 0; b < r.grid; ++b) {
      t_first = std::min(t_first, wg[2 * b]);
      t_last = std::max(t_last, wg[2 * b + 1]);
    }
    // the tail: from the first workgroup's end after which no workgroup starts
    std::vector<uint64_t> ends, starts;
    for (uint32_t b = 0; b < r.grid; ++b) {
      starts.push_back(wg[2 * b]);
      ends.push_back(wg[2 * b + 1]);
    }
    std::sort(starts.begin(), starts.end());
    std::sort(ends.begin(), ends.end());
    const uint64_t last_start = starts.back();
    const uint64_t tail0 = *std::upper_bound(ends.begin(), ends.end(), last_start);
    const double span = (t_last - t_first) * us;
    printf("\n%s grid %u: %.3f ms by events, %.1f GB/s; %.1f us first start to last end; last "
           "workgroup starts at %.1f us; tail (first end after it, to the end) %.1f us = %.2f %%\n",
           r.name, r.grid, ms, bytes / ms / 1e6, span, (last_start - t_first) * us,
           (t_last - tail0) * us, 100.0 * (t_last - tail0) / (t_last - t_first));
    printf("    t_us  resident  chunks_in_flight  window(min..max index)  window_width\n");
    const int kSamples = 40;
    for (int s = 0; s <= kSamples + 8; ++s) {
      // 40 even samples, then 8 more over the last 2 % of the launch
      const double f = s <= kSamples ? (s + 0.5) / (kSamples + 1)
                                     : 0.98 + 0.02 * (s - kSamples - 0.5) / 8;
      const uint64_t t = t_first + (uint64_t)((t_last - t_first) * f);
      uint32_t resident = 0, in_flight = 0, lo = ~0u, hi = 0;
      for (uint32_t b = 0; b < r.grid; ++b) resident += wg[2 * b] <= t && t < wg[2 * b + 1];
      for (uint64_t c = 0; c < total; ++c)
        if (ck[2 * c] <= t && t < ck[2 * c + 1]) {
          ++in_flight;
          lo = std::min(lo, (uint32_t)c);
          hi = std::max(hi, (uint32_t)c);
        }
      printf("%8.1f  %8u  %16u  %10u..%-10u  %u\n", (t - t_first) * us, resident, in_flight,
             in_flight ? lo : 0, hi, in_flight ? hi - lo + 1 : 0);
    }
    fflush(stdout);
  }
  CK(hipFree(buf));
  CK(hipFree(counter));
  CK(hipFree(wg_t));
  CK(hipFree(ck_t));
  return 0;
}
