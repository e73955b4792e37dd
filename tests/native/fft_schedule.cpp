// Walks the schedule of the additive-FFT kernels (rse_fft_sched.hpp: the maps,
// phases and twiddle templates rse_fft.hip instantiates) on scalar bytes, for
// K = 16, 32, 64 and 128: per wave phase A, the exchange, phase B, the
// exchange back, phase C.  Prints every butterfly (direction, level, block
// offset, twiddle) and the parity of a few fixed data columns for
// tests/test_fft_schedule.py, which checks them against the oracle.
#define RSE_JIT 1
#define __host__
#define __device__
#include <cstdint>
#include <cstdio>
using std::uint16_t;
using std::uint32_t;
using std::uint64_t;
using std::uint8_t;
using std::int32_t;
#include "rse_fft_sched.hpp"

namespace {

bool g_log = false;

// One byte in place of the kernels' 8 bit planes.
struct ByteOps {
  template <int I, int J, uint32_t C, bool INV>
  static void bfly(uint8_t& a, uint8_t& b) {
    if (g_log) std::printf("bfly %s %d %d %u\n", INV ? "inv" : "fwd", I, J, C);
    if (INV) {
      b ^= a;
      a ^= (uint8_t)rse::hb_mul8(C, b);
    } else {
      a ^= (uint8_t)rse::hb_mul8(C, b);
      b ^= a;
    }
  }
};

template <int K>
void encode_column(const uint8_t (&data)[K], uint8_t (&par)[K]) {
  using namespace rse;
  using S = FftSched<K>;
  constexpr int E = S::E;
  constexpr uint32_t B0 = 0, B1 = K;
  uint8_t lds[K];
  uint8_t x[E] = {};
  for (int w = 0; w < S::W; ++w) {  // phase A on the wave's own elements
    if constexpr (E == 16) {  // as the 16-element kernel: by quarters
      fft_for_wave<K>(w, [&](auto h) {
        fft_phase_a_quarters<ByteOps, K, h.value, B0>(x, [&](auto q) {
          for (int t = 0; t < 4; ++t) x[4 * q.value + t] = data[S::ac_slot(w, 4 * q.value + t)];
        });
      });
    } else {
      for (int t = 0; t < E; ++t) x[t] = data[S::ac_slot(w, t)];
      fft_a<ByteOps, K, B0, 0, S::LA, 0, E>(w, x);
    }
    for (int t = 0; t < E; ++t) lds[S::ac_slot(w, t)] = x[t];
  }
  for (int w = 0; w < S::W; ++w) {  // phase B on the wave's groups, written back in place
    for (int r = 0; r < E; ++r) x[r] = lds[S::b_slot(w, r)];
    fft_phase_b<ByteOps, K, B0, B1>(x);
    for (int r = 0; r < E; ++r) lds[S::b_slot(w, r)] = x[r];
  }
  for (int w = 0; w < S::W; ++w) {  // phase C on the wave's own elements
    for (int t = 0; t < E; ++t) x[t] = lds[S::ac_slot(w, t)];
    if constexpr (E == 16)
      fft_for_wave<K>(w, [&](auto h) { fft_phase_c<ByteOps, E, h.value, B1, S::LA - 1>(x); });
    else
      fft_c<ByteOps, K, B1>(w, x);
    for (int t = 0; t < E; ++t) par[S::ac_slot(w, t)] = x[t];
  }
}

template <int K>
void run() {
  using S = rse::FftSched<K>;
  std::printf("K %d E %d W %d G %d GPW %d LA %d M %d\n", K, S::E, S::W, S::G, S::GPW, S::LA, S::M);
  uint32_t seed = 0x9E3779B9u * K + 1u;
  for (int col = 0; col < 4; ++col) {
    uint8_t data[K], par[K];
    for (int i = 0; i < K; ++i) {
      seed = seed * 1664525u + 1013904223u;
      // column 0: one nonzero element; the others pseudo-random
      data[i] = col == 0 ? (i == K - 3 ? 0xC5 : 0) : (uint8_t)(seed >> 24);
    }
    g_log = col == 0;
    encode_column<K>(data, par);
    std::printf("in");
    for (int i = 0; i < K; ++i) std::printf(" %u", data[i]);
    std::printf("\nout");
    for (int i = 0; i < K; ++i) std::printf(" %u", par[i]);
    std::printf("\n");
  }
}

}  // namespace

int main() {
  run<16>();
  run<32>();
  run<64>();
  run<128>();
  return 0;
}
