// mx4.h — the MXFP4 quantisation rule (include/bloomstage.h) as device arithmetic, shared by the weight quantiser
// (kernels.hip) and the KV cache (kv_mxfp4.hip): a block of 32 values shares the E8M0 exponent byte E, each value
// becomes an E2M1 code (bit 3 the sign, bits 2..0 the index into {0, .5, 1, 1.5, 2, 3, 4, 6}).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// E of a block whose largest magnitude is amax, and inv = 2^(127 - E) (0 for a block below 2^-100: E = 127, codes 0).
__device__ __forceinline__ uint32_t mx4_block_exp(float amax, float& inv) {
  const bool zero = !(amax >= 0x1p-100f);
  const uint32_t E = zero ? 127u : (__float_as_uint(amax) >> 23) - 2u;
  inv = zero ? 0.f : __uint_as_float((254u - E) << 23);
  return E;
}

// Nearest grid point of |w| * inv, the even code on a tie, saturating at 6.
__device__ __forceinline__ uint32_t mx4_code(float w, float inv) {
  const float r = fabsf(w) * inv;  // exact: inv is a power of two
  const uint32_t idx = (uint32_t)(r > 0.25f) + (uint32_t)(r >= 0.75f) + (uint32_t)(r > 1.25f) + (uint32_t)(r >= 1.75f) +
                       (uint32_t)(r > 2.5f) + (uint32_t)(r >= 3.5f) + (uint32_t)(r > 5.0f);
  return idx | ((__float_as_uint(w) >> 28) & 8u);
}
