// Video-to-video entry into the denoise loop: start latents from an encoded source clip and the uint8
// frame -> bf16 NHWC boundary of the VAE encode (the step with the per-pixel keep mask is sampler.hip's).  No reference
// counterpart (the reference loop starts from noise only); semantics follow the diffusers img2img / inpaint pipelines.
#include "vst_common.h"

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

extern "C" int vst_noise_latents(const float* z0, const float* eps, const float* sigmas, const int* step_idx,
                                 float* lat, size_t n, void* stream) {
  if (!z0 || !eps || !sigmas || !step_idx || !lat || n == 0) return VST_ERR_ARG;
  hipLaunchKernelGGL(noise_latents_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, z0, eps, sigmas,
                     step_idx, lat, n);
  return launch_status();
}

extern "C" int vst_u8_to_frames(const void* src, int n, int C, int HW, void* dst, int ldd, void* stream) {
  if (!src || !dst || n <= 0 || C <= 0 || HW <= 0 || ldd < C) return VST_ERR_ARG;
  const size_t npix = (size_t)n * HW;
  hipLaunchKernelGGL(u8_to_frames_kernel, dim3(grid_for(npix * ldd)), dim3(256), 0, (hipStream_t)stream,
                     (const uint8_t*)src, npix, C, (bf16_t*)dst, ldd);
  return launch_status();
}
