// The update of the denoise loop: one fused step kernel for the Euler step, the Euler step with a
// per-pixel keep mask and the table-driven samplers (Euler and DPM-Solver++ 2M on the denoised estimate), and the
// per-clip factor of guidance rescale.  Every per-step scalar is read through the device step counter, so one captured
// step replays for the whole schedule.  The stochastic samplers are one more rule of that kernel: their
// fresh noise is counter-based (philox.h), a function of the device seed and step, so the captured step still replays.
#include "philox.h"
#include "vst_common.h"

namespace vst {

// What differs between the steps.  A rule is a kernel argument: the host sets its pointers, load() fills the per-step
// scalars on the device for the thread's pixel (clip b, local frame f, pixel p of HW), update() gives lat' for the
// element of channel k (li indexes lat and every tensor of its shape; the channels come in order) and renoise() the
// value of a kept pixel.  Each rule's expressions decide its rounding (where the compiler may contract
// a * b + c into one FMA), so they change only with the bits.

// lat' = lat + (sigma[s+1] - sigma[s]) e  (EulerDiscreteScheduler.step, epsilon prediction)
struct EulerRule {
  float ds;
  __device__ __forceinline__ void load(const float* sigmas, int s, int, int, int, int) {
    ds = sigmas[s + 1] - sigmas[s];
  }
  __device__ __forceinline__ float update(float x, float e, size_t, int) const { return x + ds * e; }
  static __device__ __forceinline__ float renoise(float z0, float s1, float eps) { return z0 + s1 * eps; }
};

// coef rows are (a, b, c):  e *= factor[b];  D = lat - sigma[s] e;  lat' = a lat + b D + c hist;  hist = D
// hist is not read when c == 0 (the step a run enters at): whatever it holds then never reaches the latents.
struct TableRule {
  float* hist;
  const float* coef;
  const float* factor;  // per clip, or nullptr
  float sg, ca, cb, cc, fac;
  __device__ __forceinline__ void load_row(const float* sigmas, int s, int b, int cols) {
    sg = sigmas[s];
    ca = coef[cols * s], cb = coef[cols * s + 1], cc = coef[cols * s + 2];
    fac = factor ? factor[b] : 1.0f;
  }
  __device__ __forceinline__ void load(const float* sigmas, int s, int b, int, int, int) { load_row(sigmas, s, b, 3); }
  __device__ __forceinline__ float update(float x, float e, size_t li, int) const {
    const bool use_hist = cc != 0.0f;
    if (factor) e *= fac;
    const float D = x - sg * e;
    const float h = use_hist ? hist[li] : 0.0f;
    float ln = ca * x + cb * D;
    if (use_hist) ln += cc * h;
    hist[li] = D;
    return ln;
  }
  // z0 + s1 * eps rounded twice (product, then sum): the value torch computes, so a kept pixel is reproducible bit
  // for bit on the host at every step, not only where s1 == 0.
  static __device__ __forceinline__ float renoise(float z0, float s1, float eps) {
#pragma clang fp contract(off)
    const float t = s1 * eps;
    return z0 + t;
  }
};

// coef rows are (a, b, c, d):  TableRule's step, then lat' += d xi, xi the standard normal of philox.h at
// (*seed, s, stream 0, the element's place in the whole clip: this tensor holds frames [f0, f0 + F) of F_total).
// Where d == 0 xi is neither generated nor added, so lat' has TableRule's bits.  One Philox call serves 4 channels.
struct NoiseRule : TableRule {
  const uint64_t* seed;
  int F_total, f0;
  float cd;
  uint64_t key, pos;
  uint32_t step;
  float xi[4];
  __device__ __forceinline__ void load(const float* sigmas, int s, int b, int f, int p, int HW) {
    load_row(sigmas, s, b, 4);
    cd = coef[4 * s + 3];
    key = *seed;
    pos = noise_position(b, F_total, f0 + f, HW, p);
    step = (uint32_t)s;
  }
  __device__ __forceinline__ float update(float x, float e, size_t li, int k) {
    float ln = TableRule::update(x, e, li, k);
    if (cd != 0.0f) {
      const int lane = k & 3;
      if (lane == 0) noise_normal4(key, pos, step, 0u, (uint32_t)k >> 2, xi);
      const float n = lane == 0 ? xi[0] : lane == 1 ? xi[1] : lane == 2 ? xi[2] : xi[3];  // no indexed register array
      ln += cd * n;
    }
    return ln;
  }
};

// The 4 channels of one noise row: one 8-byte load where the rows are 8-byte aligned (vec), four 2-byte loads otherwise.
__device__ __forceinline__ u32x2 load_row4(const bf16_t* row, bool vec) {
  if (vec) return *reinterpret_cast<const u32x2*>(row);
  return u32x2{(uint32_t)row[0] | ((uint32_t)row[1] << 16), (uint32_t)row[2] | ((uint32_t)row[3] << 16)};
}

// One thread per pixel (b, f, p): the mask is read once, the pixel's noise row(s) once (CL4, Cl == 4: load_row4 per CFG
// copy, and the 4 channels unrolled, so the stored bits do not depend on the alignment of noise), then the Cl channel planes of lat / z0 / eps (and what the rule holds) are walked, each plane access coalesced
// in p.  noise rows are ((k*B + b)*F + f)*HW + p, Cl channels, k = 0 uncond, k = 1 cond:
//   e = u + g (c - u);  lat' = rule.update(lat, e);  MASKED: lat = m lat' + (1 - m) rule.renoise(z0, sigma[s+1], eps)
template <class Rule, bool CL4, bool MASKED>
__global__ __launch_bounds__(256) void denoise_step_kernel(const bf16_t* __restrict__ noise, int ncopy, float guidance,
                                                           float* __restrict__ lat, int B, int Cl, int F, int HW,
                                                           const float* __restrict__ sigmas,
                                                           const int* __restrict__ step, Rule rule,
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
  rule.load(sigmas, s, b, f, p, HW);
  float s1 = 0.0f, m = 1.0f, keep = 0.0f;
  if (MASKED) {
    s1 = sigmas[s + 1];
    m = mask[((size_t)(mask_clips == 1 ? 0 : b) * F + f) * HW + p];
    keep = 1.0f - m;
  }
  const size_t plane = (size_t)F * HW;
  size_t li = ((size_t)b * Cl * F + f) * HW + p;
  const bf16_t* nu = noise + t * Cl;           // uncond (or the only) row
  const bf16_t* nc = noise + (npix + t) * Cl;  // cond row (ncopy == 2)

  auto update = [&](float e, int k) {
    float ln = rule.update(lat[li], e, li, k);
    if (MASKED) ln = m * ln + keep * Rule::renoise(z0[li], s1, eps[li]);
    lat[li] = ln;
  };

  if (CL4) {
    const bool vec = ((uintptr_t)noise & 7) == 0;  // rows are 8 bytes apart: the base decides for all of them
    float e[4];
    unpack4(load_row4(nu, vec), e);
    if (ncopy == 2) {
      float c[4];
      unpack4(load_row4(nc, vec), c);
#pragma unroll
      for (int k = 0; k < 4; ++k) e[k] = cfg_mix(e[k], c[k], guidance);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k, li += plane) update(e[k], k);
  } else {
    for (int k = 0; k < Cl; ++k, li += plane) {
      float e = bf2f(nu[k]);
      if (ncopy == 2) e = cfg_mix(e, bf2f(nc[k]), guidance);
      update(e, k);
    }
  }
}

// The noise alone, one thread per pixel as the step walks it: out (B, Cl, F, HW) holds, per element, the Philox word
// of its channel (NORMAL false: the counter layout, checked exactly) or the normal the step adds (NORMAL true).
template <bool NORMAL>
__global__ __launch_bounds__(256) void noise_fill_kernel(uint32_t* __restrict__ out, const uint64_t* __restrict__ seed,
                                                         const int* __restrict__ step, uint32_t stream_id, int B,
                                                         int Cl, int F, int F_total, int f0, int HW) {
  const size_t npix = (size_t)B * F * HW;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= npix) return;
  const int p = (int)(t % HW);
  const size_t bf = t / HW;
  const int f = (int)(bf % F);
  const int b = (int)(bf / F);
  const uint64_t key = *seed;
  const uint32_t s = (uint32_t)*step;
  const uint64_t pos = noise_position(b, F_total, f0 + f, HW, p);
  const size_t plane = (size_t)F * HW;
  size_t li = ((size_t)b * Cl * F + f) * HW + p;
  for (int k0 = 0; k0 < Cl; k0 += 4) {
    uint32_t x[4];
    noise_bits4(key, pos, s, stream_id, (uint32_t)k0 >> 2, x);
    if (NORMAL) {
      float n[4];
      normals_of_bits4(x, n);
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = __float_as_uint(n[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j, li += plane)
      if (k0 + j < Cl) out[li] = x[j];
  }
}

// ---- guidance rescale: factor[b] = phi * std(cond_b) / std(e_b) + (1 - phi) ----
// A clip's cond rows and uncond rows are each one contiguous run of n = Cl * F * HW bf16 values, so the statistics are
// those of two flat arrays.  Partials are (count, mean, M2) merged with Chan's formula (a sum of squares would cancel
// on a noise tensor with a mean); every merge order is fixed by the indices alone: lanes by a shuffle-down tree,
// waves in order, blocks strided then by an LDS tree.  No atomics: a replayed graph gives the eager bits.
struct Moments {
  float n, mean, m2;
};

__device__ __forceinline__ Moments chan_merge(Moments a, Moments b) {
  const float n = a.n + b.n;
  const float w = n > 0.0f ? b.n / n : 0.0f;  // an empty side has mean 0 and M2 0 and leaves the other unchanged
  const float d = b.mean - a.mean;
  return {n, a.mean + d * w, a.m2 + b.m2 + d * d * a.n * w};
}

__device__ __forceinline__ Moments wave_merge(Moments v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const Moments other = {__shfl_down(v.n, o), __shfl_down(v.mean, o), __shfl_down(v.m2, o)};
    v = chan_merge(v, other);  // lane 0 ends with the tree over all 64 lanes; the other lanes' values are unused
  }
  return v;
}

constexpr int kRescalePer = 4;                       // values per thread
constexpr int kRescaleChunk = 256 * kRescalePer;     // values per block

__device__ __forceinline__ Moments moments_of(const float* x, int cnt) {
  float sum = 0.0f;
#pragma unroll
  for (int k = 0; k < kRescalePer; ++k) sum += k < cnt ? x[k] : 0.0f;
  const float mean = cnt > 0 ? sum / (float)cnt : 0.0f;
  float m2 = 0.0f;
#pragma unroll
  for (int k = 0; k < kRescalePer; ++k) {
    const float d = x[k] - mean;
    m2 += k < cnt ? d * d : 0.0f;
  }
  return {(float)cnt, mean, m2};
}

// grid (nblk, B): block (j, b) reduces values [j * chunk, min(n, (j + 1) * chunk)) of clip b into
// ws[(b * nblk + j) * 6 ..] = cond (count, mean, M2), e (count, mean, M2).  Thread t holds values base + k * 256 + t.
__global__ __launch_bounds__(256) void rescale_partials_kernel(const bf16_t* __restrict__ noise, float guidance, int B,
                                                               size_t n, float* __restrict__ ws) {
  __shared__ Moments part[2][4];
  const int b = blockIdx.y;
  const size_t base = (size_t)blockIdx.x * kRescaleChunk;
  const bf16_t* u = noise + (size_t)b * n;
  const bf16_t* c = noise + ((size_t)B + b) * n;
  float xc[kRescalePer], xe[kRescalePer];
  int cnt = 0;
#pragma unroll
  for (int k = 0; k < kRescalePer; ++k) {
    const size_t i = base + (size_t)k * 256 + threadIdx.x;
    xc[k] = xe[k] = 0.0f;
    if (i < n) {  // i grows with k: the values in range are the first cnt
      const float cv = bf2f(c[i]);
      xc[k] = cv;
      xe[k] = cfg_mix(bf2f(u[i]), cv, guidance);
      ++cnt;
    }
  }
  const Moments mc = wave_merge(moments_of(xc, cnt));
  const Moments me = wave_merge(moments_of(xe, cnt));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    part[0][wave] = mc;
    part[1][wave] = me;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    Moments acc = part[threadIdx.x][0];
    for (int w = 1; w < 4; ++w) acc = chan_merge(acc, part[threadIdx.x][w]);
    float* o = ws + ((size_t)b * gridDim.x + blockIdx.x) * 6 + threadIdx.x * 3;
    o[0] = acc.n;
    o[1] = acc.mean;
    o[2] = acc.m2;
  }
}

struct Moments64 {
  double n, mean, m2;
};

__device__ __forceinline__ Moments64 chan_merge64(Moments64 a, Moments64 b) {
  const double n = a.n + b.n;
  const double w = n > 0.0 ? b.n / n : 0.0;
  const double d = b.mean - a.mean;
  return {n, a.mean + d * w, a.m2 + b.m2 + d * d * a.n * w};
}

// grid B: thread t merges the block partials t, t + 256, ... of its clip in that order, then an LDS tree over the 256
// threads; in fp64, so a clip of any length keeps exact counts.  factor = 1 where std(e) == 0.
__global__ __launch_bounds__(256) void rescale_finalize_kernel(const float* __restrict__ ws, int nblk, float phi,
                                                               float* __restrict__ factor) {
  __shared__ Moments64 red[2][256];
  const int b = blockIdx.x, t = threadIdx.x;
  Moments64 acc[2] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  for (int j = t; j < nblk; j += 256) {
    const float* o = ws + ((size_t)b * nblk + j) * 6;
#pragma unroll
    for (int q = 0; q < 2; ++q) acc[q] = chan_merge64(acc[q], {(double)o[3 * q], (double)o[3 * q + 1], (double)o[3 * q + 2]});
  }
  red[0][t] = acc[0];
  red[1][t] = acc[1];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      red[0][t] = chan_merge64(red[0][t], red[0][t + o]);
      red[1][t] = chan_merge64(red[1][t], red[1][t + o]);
    }
    __syncthreads();
  }
  if (t == 0) {
    const double m2c = red[0][0].m2, m2e = red[1][0].m2;  // the n - 1 of the two unbiased estimators cancels
    factor[b] = m2e > 0.0 ? (float)((double)phi * sqrt(m2c / m2e) + (1.0 - (double)phi)) : 1.0f;
  }
}

}  // namespace vst

using namespace vst;

static inline int rescale_blocks(size_t n) { return (int)((n + kRescaleChunk - 1) / kRescaleChunk); }

// What every step takes, and the launch all three entry points share.  mask == nullptr: no blend.
struct StepArgs {
  const void* noise;
  int ncopy;
  float guidance;
  float* lat;
  int B, Cl, F, HW;
  const float* sigmas;
  const int* step_idx;
  const float *z0, *eps, *mask;
  int mask_clips;
  void* stream;
};

template <class Rule>
static int launch_step(const StepArgs& a, Rule rule) {
  if (!a.noise || !a.lat || !a.sigmas || !a.step_idx || (a.ncopy != 1 && a.ncopy != 2)) return VST_ERR_ARG;
  if (a.B <= 0 || a.Cl <= 0 || a.F <= 0 || a.HW <= 0) return VST_ERR_ARG;
  if (a.mask && (!a.z0 || !a.eps || (a.mask_clips != 1 && a.mask_clips != a.B))) return VST_ERR_ARG;
  const size_t npix = (size_t)a.B * a.F * a.HW;
  const dim3 grid((unsigned)((npix + 255) / 256));
  const bool cl4 = a.Cl == 4;
#define VST_STEP_LAUNCH(C4, M)                                                                                     \
  hipLaunchKernelGGL((denoise_step_kernel<Rule, C4, M>), grid, dim3(256), 0, (hipStream_t)a.stream,               \
                     (const bf16_t*)a.noise, a.ncopy, a.guidance, a.lat, a.B, a.Cl, a.F, a.HW, a.sigmas, a.step_idx, \
                     rule, a.z0, a.eps, a.mask, a.mask_clips)
  if (cl4 && a.mask) VST_STEP_LAUNCH(true, true);
  else if (cl4) VST_STEP_LAUNCH(true, false);
  else if (a.mask) VST_STEP_LAUNCH(false, true);
  else VST_STEP_LAUNCH(false, false);
#undef VST_STEP_LAUNCH
  return launch_status();
}

extern "C" int vst_euler_cfg_step(const void* noise, int ncopy, float guidance, float* lat, int B, int Cl, int F,
                                  int HW, const float* sigmas, const int* step_idx, void* stream) {
  return launch_step({noise, ncopy, guidance, lat, B, Cl, F, HW, sigmas, step_idx, nullptr, nullptr, nullptr, 0, stream},
                     EulerRule{});
}

extern "C" int vst_euler_cfg_step_masked(const void* noise, int ncopy, float guidance, float* lat, int B, int Cl,
                                         int F, int HW, const float* sigmas, const int* step_idx, const float* z0,
                                         const float* eps, const float* mask, int mask_clips, void* stream) {
  if (!mask) return VST_ERR_ARG;
  return launch_step({noise, ncopy, guidance, lat, B, Cl, F, HW, sigmas, step_idx, z0, eps, mask, mask_clips, stream},
                     EulerRule{});
}

extern "C" int vst_sampler_step(const void* noise, int ncopy, float guidance, float* lat, float* hist, int B, int Cl,
                                int F, int HW, const float* sigmas, const float* coef, const int* step_idx,
                                const float* factor, const float* z0, const float* eps, const float* mask,
                                int mask_clips, void* stream) {
  if (!hist || !coef || lat == hist) return VST_ERR_ARG;
  if (!mask && (z0 || eps)) return VST_ERR_ARG;
  if (factor && ncopy != 2) return VST_ERR_ARG;  // the rescale factor is defined on the CFG pair
  return launch_step({noise, ncopy, guidance, lat, B, Cl, F, HW, sigmas, step_idx, z0, eps, mask, mask_clips, stream},
                     TableRule{hist, coef, factor});
}

// What every noise entry refuses: the frames [f0, f0 + F) must lie in the clip, and the counter's last word holds the
// stream in its upper and the channel group (Cl / 4 of them) in its lower 16 bits.
static bool noise_args_ok(const void* seed, int stream_id, int Cl, int F, int F_total, int f0) {
  return seed && stream_id >= 0 && stream_id < (1 << 16) && Cl <= (1 << 18) && F > 0 && F_total > 0 && f0 >= 0 &&
         F <= F_total - f0;
}

extern "C" int vst_sampler_step_noise(const void* noise, int ncopy, float guidance, float* lat, float* hist, int B,
                                      int Cl, int F, int F_total, int f0, int HW, const float* sigmas,
                                      const float* coef4, const int* step_idx, const uint64_t* seed,
                                      const float* factor, const float* z0, const float* eps, const float* mask,
                                      int mask_clips, void* stream) {
  if (!hist || !coef4 || lat == hist) return VST_ERR_ARG;
  if (!mask && (z0 || eps)) return VST_ERR_ARG;
  if (factor && ncopy != 2) return VST_ERR_ARG;
  if (!noise_args_ok(seed, 0, Cl, F, F_total, f0)) return VST_ERR_ARG;
  NoiseRule rule{{hist, coef4, factor}, seed, F_total, f0};
  return launch_step({noise, ncopy, guidance, lat, B, Cl, F, HW, sigmas, step_idx, z0, eps, mask, mask_clips, stream},
                     rule);
}

template <bool NORMAL>
static int launch_noise_fill(void* out, const uint64_t* seed, const int* step_idx, int stream_id, int B, int Cl, int F,
                             int F_total, int f0, int HW, void* stream) {
  if (!out || !step_idx || B <= 0 || Cl <= 0 || HW <= 0) return VST_ERR_ARG;
  if (!noise_args_ok(seed, stream_id, Cl, F, F_total, f0)) return VST_ERR_ARG;
  const size_t npix = (size_t)B * F * HW;
  hipLaunchKernelGGL(noise_fill_kernel<NORMAL>, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (uint32_t*)out, seed, step_idx, (uint32_t)stream_id, B, Cl, F, F_total, f0, HW);
  return launch_status();
}

extern "C" int vst_noise_bits(uint32_t* out, const uint64_t* seed, const int* step_idx, int stream_id, int B, int Cl,
                              int F, int F_total, int f0, int HW, void* stream) {
  return launch_noise_fill<false>(out, seed, step_idx, stream_id, B, Cl, F, F_total, f0, HW, stream);
}

extern "C" int vst_noise_normal(float* out, const uint64_t* seed, const int* step_idx, int stream_id, int B, int Cl,
                                int F, int F_total, int f0, int HW, void* stream) {
  return launch_noise_fill<true>(out, seed, step_idx, stream_id, B, Cl, F, F_total, f0, HW, stream);
}

extern "C" size_t vst_cfg_rescale_factor_workspace_bytes(int B, int Cl, int F, int HW) {
  if (B <= 0 || Cl <= 0 || F <= 0 || HW <= 0) return 0;
  return (size_t)B * rescale_blocks((size_t)Cl * F * HW) * 6 * sizeof(float);
}

extern "C" int vst_cfg_rescale_factor(const void* noise, float guidance, float phi, int B, int Cl, int F, int HW,
                                      float* factor, void* workspace, void* stream) {
  if (!noise || !factor || !workspace) return VST_ERR_ARG;
  if (B <= 0 || B > 65535 || Cl <= 0 || F <= 0 || HW <= 0 || !(phi >= 0.0f && phi <= 1.0f)) return VST_ERR_ARG;
  const size_t n = (size_t)Cl * F * HW;
  const int nblk = rescale_blocks(n);
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(rescale_partials_kernel, dim3(nblk, B), dim3(256), 0, s, (const bf16_t*)noise, guidance, B, n,
                     (float*)workspace);
  hipLaunchKernelGGL(rescale_finalize_kernel, dim3(B), dim3(256), 0, s, (const float*)workspace, nblk, phi, factor);
  return launch_status();
}
