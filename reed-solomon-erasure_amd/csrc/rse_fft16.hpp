// rse_fft16.hpp -- the pruned additive-FFT kernel of GF(2^16) codecs past 256
// shards with u = 2^m - k <= 32 (rse_fft16.hip; tables: rse_fft16_plan.hpp):
// encode, verify and reconstruct with no run-time module, opt-in with
// RSE_OPT_FFT16.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rse_fft16_plan.hpp"

namespace rse {

// RSE_OPT_FFT16 is on and k+p is a shape of the kernel: the codec's plan, built
// on first use and kept for the life of the process; otherwise null.
const Fft16Plan* fft16_plan(int field, uint32_t k, uint32_t p);
// rows[p x k] are the codec's parity rows and fft16_plan(field, k, p).
bool fft16_applies(int field, uint32_t k, uint32_t p, const uint16_t* rows);

// Codes the whole 4 KiB columns of every shard of n_stripes stripes:
//   out[r] = sum_c mat[r][c] . coef[c],  coef = the top u coefficients of the
//   pruned inverse transform of in[0 .. n-1] (a null pointer is a zero shard),
// stored and / or compared with cmp[r] by mode (CodeMode).  what: "code",
// "check" or "rebuild" for rse_last_kernel.  *done = bytes per shard coded.
hipError_t launch_fft16(const Fft16Plan& pl, const uint8_t* const* in, uint32_t n_rows,
                        const uint16_t* mat, uint8_t* const* out, const uint8_t* const* cmp,
                        uint64_t len, uint64_t stripe_stride, uint32_t n_stripes, uint32_t mode,
                        uint32_t* mismatch, bool per_stripe, const char* what, hipStream_t stream,
                        uint64_t* done);

}  // namespace rse
