// Video-to-video entry into the denoise loop: start latents from an encoded source clip, the Euler
// step with a per-pixel keep mask, and the uint8 frame -> bf16 NHWC boundary of the VAE encode.  No reference
// counterpart (the reference loop starts from noise only); semantics follow the diffusers img2img / inpaint pipelines.
#include "vst_common.h"
#include <algorithm>

namespace vst {

// lat[i] = z0[i] + sigmas[*step] * eps[i]  (EulerDiscreteScheduler.add_noise at the start step; sigma read on the
// device, so a new strength needs no host copy and no recapture)
__global__ __launch_bounds__(256) void noise_latents_kernel(const float* __restrict__ z0,
                                                            const float* __restrict__ eps,
                                                            const float* __restrict__ sigmas,
                                                            const int* __restrict__ step, float* __restrict__ lat,
                                                            size_t n) {
  const float sg = sigmas[*step];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    lat[i] = z0[i] + sg * eps[i];
}

// The update of euler_cfg_kernel (elementwise.hip), written in the same form so both round alike: with m == 1 the
// masked step below stores exactly what the plain step stores.
__device__ __forceinline__ float euler_update(float lat, float ds, float e) { return lat + ds * e; }
__device__ __forceinline__ float cfg_combine(float u, float c, float guidance) { return u + guidance * (c - u); }

// One thread per pixel (b, f, p): the mask is read once, the pixel's noise row(s) once (CL4: one 8-byte load per CFG
// copy), then the Cl channel planes of lat / z0 / eps are walked (each plane access is coalesced in p).
//   lat' = lat + (sigma[s+1] - sigma[s]) * eps_hat;  lat = m * lat' + (1 - m) * (z0 + sigma[s+1] * eps)
// noise rows as in euler_cfg_kernel: ((k*B + b)*F + f)*HW + p, Cl channels, k = 0 uncond, k = 1 cond.
template <bool CL4>
__global__ __launch_bounds__(256) void euler_cfg_masked_kernel(const bf16_t* __restrict__ noise, int ncopy,
                                                               float guidance, float* __restrict__ lat, int B, int Cl,
                                                               int F, int HW, const float* __restrict__ sigmas,
                                                               const int* __restrict__ step,
                                                               const float* __restrict__ z0,
                                                               const float* __restrict__ eps,
                                                               const float* __restrict__ mask, int mask_clips) {
  const size_t npix = (size_t)B * F * HW;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= npix) return;
  const int p = (int)(t % HW);
  const size_t bf = t / HW;  // b * F + f
  const int f = (int)(bf % F);
  const int b = (int)(bf / F);
  const int s = *step;
  const float s1 = sigmas[s + 1];
  const float ds = s1 - sigmas[s];
  const float m = mask[((size_t)(mask_clips == 1 ? 0 : b) * F + f) * HW + p];
  const float keep = 1.0f - m;
  const size_t plane = (size_t)F * HW;
  size_t li = ((size_t)b * Cl * F + f) * HW + p;
  const bf16_t* nu = noise + t * Cl;            // uncond (or the only) row
  const bf16_t* nc = noise + (npix + t) * Cl;   // cond row (ncopy == 2)
  if (CL4) {
    const u32x2 u2 = *reinterpret_cast<const u32x2*>(nu);
    float e[4] = {__uint_as_float(u2.x << 16), __uint_as_float(u2.x & 0xffff0000u), __uint_as_float(u2.y << 16),
                  __uint_as_float(u2.y & 0xffff0000u)};
    if (ncopy == 2) {
      const u32x2 c2 = *reinterpret_cast<const u32x2*>(nc);
      const float c[4] = {__uint_as_float(c2.x << 16), __uint_as_float(c2.x & 0xffff0000u),
                          __uint_as_float(c2.y << 16), __uint_as_float(c2.y & 0xffff0000u)};
#pragma unroll
      for (int k = 0; k < 4; ++k) e[k] = cfg_combine(e[k], c[k], guidance);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k, li += plane) {
      const float ln = euler_update(lat[li], ds, e[k]);
      lat[li] = m * ln + keep * (z0[li] + s1 * eps[li]);
    }
  } else {
    for (int k = 0; k < Cl; ++k, li += plane) {
      float e = bf2f(nu[k]);
      if (ncopy == 2) e = cfg_combine(e, bf2f(nc[k]), guidance);
      const float ln = euler_update(lat[li], ds, e);
      lat[li] = m * ln + keep * (z0[li] + s1 * eps[li]);
    }
  }
}

// dst[(i*HW + p)*ldd + c] = bf16((src[(i*HW + p)*C + c] / 255 - 0.5) / 0.5) for c < C, 0 for C <= c < ldd
// (video_dataset.py:117-118 in fp32, an IEEE division, then the bf16 rounding of the encoder's input boundary)
__global__ __launch_bounds__(256) void u8_to_frames_kernel(const uint8_t* __restrict__ src, size_t npix, int C,
                                                           bf16_t* __restrict__ dst, int ldd) {
  const size_t total = npix * ldd;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % ldd);
    const size_t t = i / ldd;  // img * HW + p
    dst[i] = c < C ? f2bf(((float)src[t * C + c] / 255.0f - 0.5f) / 0.5f) : (bf16_t)0;
  }
}

}  // namespace vst

using namespace vst;

static inline int grid_for(size_t total) { return (int)std::min<size_t>((total + 255) / 256, 16384); }

extern "C" int vst_noise_latents(const float* z0, const float* eps, const float* sigmas, const int* step_idx,
                                 float* lat, size_t n, void* stream) {
  if (!z0 || !eps || !sigmas || !step_idx || !lat || n == 0) return VST_ERR_ARG;
  hipLaunchKernelGGL(noise_latents_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, z0, eps, sigmas,
                     step_idx, lat, n);
  return launch_status();
}

extern "C" int vst_euler_cfg_step_masked(const void* noise, int ncopy, float guidance, float* lat, int B, int Cl,
                                         int F, int HW, const float* sigmas, const int* step_idx, const float* z0,
                                         const float* eps, const float* mask, int mask_clips, void* stream) {
  if (!noise || !lat || !sigmas || !step_idx || !z0 || !eps || !mask) return VST_ERR_ARG;
  if ((ncopy != 1 && ncopy != 2) || B <= 0 || Cl <= 0 || F <= 0 || HW <= 0) return VST_ERR_ARG;
  if (mask_clips != 1 && mask_clips != B) return VST_ERR_ARG;
  const size_t npix = (size_t)B * F * HW;
  const dim3 grid((unsigned)((npix + 255) / 256));
  const hipStream_t s = (hipStream_t)stream;
  const bf16_t* nz = (const bf16_t*)noise;
  if (Cl == 4 && ((uintptr_t)noise & 7) == 0)
    hipLaunchKernelGGL(euler_cfg_masked_kernel<true>, grid, dim3(256), 0, s, nz, ncopy, guidance, lat, B, Cl, F, HW,
                       sigmas, step_idx, z0, eps, mask, mask_clips);
  else
    hipLaunchKernelGGL(euler_cfg_masked_kernel<false>, grid, dim3(256), 0, s, nz, ncopy, guidance, lat, B, Cl, F, HW,
                       sigmas, step_idx, z0, eps, mask, mask_clips);
  return launch_status();
}

extern "C" int vst_u8_to_frames(const void* src, int n, int C, int HW, void* dst, int ldd, void* stream) {
  if (!src || !dst || n <= 0 || C <= 0 || HW <= 0 || ldd < C) return VST_ERR_ARG;
  const size_t npix = (size_t)n * HW;
  hipLaunchKernelGGL(u8_to_frames_kernel, dim3(grid_for(npix * ldd)), dim3(256), 0, (hipStream_t)stream,
                     (const uint8_t*)src, npix, C, (bf16_t*)dst, ldd);
  return launch_status();
}
