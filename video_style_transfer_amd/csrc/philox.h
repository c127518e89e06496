// Counter-based noise: Philox4x32-10 (Salmon et al. 2011, the Random123 constants) and the normals
// made of its output.  Nothing here has state: the noise of an element is a function of (seed, step, stream, where
// the element sits in the whole clip), so it is the same from any thread, rank or launch, eager or replayed.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace vst {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;  // round multipliers
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;  // Weyl key increments

// x <- philox4x32_10(counter = x, key = (k0, k1)): ten rounds of two 32x32 -> 64 multiplies, the key bumped between.
__device__ __forceinline__ void philox4x32_10(uint32_t x[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)kPhiloxM0 * x[0];
    const uint64_t p1 = (uint64_t)kPhiloxM1 * x[2];
    const uint32_t y0 = (uint32_t)(p1 >> 32) ^ x[1] ^ k0;
    const uint32_t y2 = (uint32_t)(p0 >> 32) ^ x[3] ^ k1;
    x[0] = y0, x[1] = (uint32_t)p1, x[2] = y2, x[3] = (uint32_t)p0;
    k0 += kPhiloxW0, k1 += kPhiloxW1;
  }
}

// Where an element sits in the whole clip: clip b, global frame fg of F_total, pixel p of HW.
__device__ __forceinline__ uint64_t noise_position(int b, int F_total, int fg, int HW, int p) {
  return ((uint64_t)b * (uint64_t)F_total + (uint64_t)fg) * (uint64_t)HW + (uint64_t)p;
}

// The four words of channel group `group` (channels 4 group .. 4 group + 3; channel c takes lane c & 3):
// counter (lo32(pos), hi32(pos), step, stream_id << 16 | group), key (lo32(seed), hi32(seed)).
__device__ __forceinline__ void noise_bits4(uint64_t seed, uint64_t pos, uint32_t step, uint32_t stream_id,
                                            uint32_t group, uint32_t x[4]) {
  x[0] = (uint32_t)pos, x[1] = (uint32_t)(pos >> 32), x[2] = step, x[3] = (stream_id << 16) | group;
  philox4x32_10(x, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// Box-Muller on the four words: u_k = ((x_k >> 9) + 0.5) * 2^-23 is exact in fp32 and inside (0, 1);
// (n0, n1) = sqrt(-2 log u0) * (cospi, sinpi)(2 u1), (n2, n3) likewise from (u2, u3).  Every caller's normals come from
// this one function, with contraction off, so the fused step and the stand-alone fill store the same bits.
__device__ __forceinline__ void normals_of_bits4(const uint32_t x[4], float n[4]) {
#pragma clang fp contract(off)
  float u[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) u[k] = ((float)(x[k] >> 9) + 0.5f) * 0x1p-23f;
#pragma unroll
  for (int k = 0; k < 4; k += 2) {
    const float r = sqrtf(-2.0f * logf(u[k]));
    const float a = 2.0f * u[k + 1];
    n[k] = r * cospif(a);
    n[k + 1] = r * sinpif(a);
  }
}

__device__ __forceinline__ void noise_normal4(uint64_t seed, uint64_t pos, uint32_t step, uint32_t stream_id,
                                              uint32_t group, float n[4]) {
  uint32_t x[4];
  noise_bits4(seed, pos, step, stream_id, group, x);
  normals_of_bits4(x, n);
}

}  // namespace vst
