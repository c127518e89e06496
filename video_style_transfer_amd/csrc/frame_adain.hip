// StyleAligned AdaIN of the spatial self-attention's q/k(/v) to the anchor frame (Hertz et al., "Style
// Aligned Image Generation via Shared Attention", CVPR 2024: the adain_queries / adain_keys / adain_values step of its
// shared attention).  No line of the reference does this; the definition is this project's.
//
// Rows (b*F + f)*N + p of a bf16 view x[., 0..C).  Per clip b, frame f and column c, in fp32 from the bf16 values:
//   mu[b,f,c] = mean over the N tokens,  sd[b,f,c] = sqrt(sum (x - mu)^2 / (N - 1) + eps)
//   y[b,f,p,c] = bf16((x - mu[b,f,c]) * (sd[b,a,c] / sd[b,f,c]) + mu[b,a,c])   for f != a; frame a is not written.
// The mean is subtracted first: q/k have channels with a large mean, where x * s + t cancels badly.
//
// Two launches, no atomics, every sum in an order the shape alone fixes:
//   1. frame_adain_stats_kernel: one workgroup per (clip * frame, slab of 64 columns).  A row of the slab is 128
//      contiguous bytes, read as eight 16-byte loads; 256 threads cover 32 rows per pass.  The slab is read twice (mean,
//      then centred squares; N <= 4096 keeps it <= 512 KiB, so the second read comes from the L2), a one-pass sum of
//      squares loses the sd of channels with |mu| >> sd.  Lanes meet through the LDS in index order.
//   2. frame_adain_apply_kernel: one workgroup per (clip * non-anchor frame, slab, chunk of 256 rows); each thread
//      keeps the (mu_f, sd_a / sd_f, mu_a) of its 8 columns in registers.  Anchor frames are not in the grid.
#include <math.h>

#include "vst_common.h"

namespace vst {

constexpr int kAdainNT = 256;                  // threads of both kernels
constexpr int kAdainCG = 8;                    // 16-byte column groups of a slab: 64 columns, 128 bytes per row
constexpr int kAdainRP = kAdainNT / kAdainCG;  // rows of one pass
constexpr int kAdainChunk = 256;               // rows of one apply workgroup

// The sums of the 32 row lanes that share a column group, per column, in row-lane order; the result for all threads.
__device__ __forceinline__ void adain_block_sum(const float* acc, float (*part)[kAdainCG * 8 + 1], float* tot, int rl,
                                                int cg, int tid) {
#pragma unroll
  for (int c = 0; c < 8; ++c) part[rl][cg * 8 + c] = acc[c];
  __syncthreads();
  if (tid < kAdainCG * 8) {
    float v = part[0][tid];
#pragma unroll
    for (int r = 1; r < kAdainRP; ++r) v += part[r][tid];
    tot[tid] = v;
  }
  __syncthreads();
}

__global__ __launch_bounds__(kAdainNT) void frame_adain_stats_kernel(const bf16_t* __restrict__ x, int ldx, int N, int C,
                                                                     float eps, float* __restrict__ stats, int nslab) {
  __shared__ float part[kAdainRP][kAdainCG * 8 + 1];  // + 1: the row lanes of a wave on different banks
  __shared__ float tot[kAdainCG * 8];
  const int tid = threadIdx.x;
  const int cg = tid % kAdainCG, rl = tid / kAdainCG;
  const int bf = blockIdx.x / nslab, slab = blockIdx.x - bf * nslab;
  const int c0 = (slab * kAdainCG + cg) * 8;
  const bool col_ok = c0 < C;  // C % 8 == 0: a column group is whole or absent (partial last slab)
  // (element offsets fit 31 bits: the entry point refuses larger extents)
  const bf16_t* src = x + (uint32_t)bf * N * ldx + c0;

  float acc[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) acc[c] = 0.0f;
  if (col_ok) {
#pragma unroll 4
    for (int r = rl; r < N; r += kAdainRP) {
      float f[8];
      unpack8(*reinterpret_cast<const u32x4*>(src + (uint32_t)r * ldx), f);
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[c] += f[c];
    }
  }
  adain_block_sum(acc, part, tot, rl, cg, tid);
  float mu[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    mu[c] = tot[cg * 8 + c] / (float)N;
    acc[c] = 0.0f;
  }
  __syncthreads();  // tot is rewritten below
  if (col_ok) {
#pragma unroll 4
    for (int r = rl; r < N; r += kAdainRP) {
      float f[8];
      unpack8(*reinterpret_cast<const u32x4*>(src + (uint32_t)r * ldx), f);  // second read: from the L2
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const float d = f[c] - mu[c];
        acc[c] = fmaf(d, d, acc[c]);
      }
    }
  }
  adain_block_sum(acc, part, tot, rl, cg, tid);
  if (rl == 0 && col_ok) {
    float sd[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) sd[c] = sqrtf(tot[cg * 8 + c] / (float)(N - 1) + eps);
    float* dst = stats + (size_t)bf * 2 * C + c0;  // [mean row | sd row] of the frame
    *reinterpret_cast<f32x4*>(dst) = f32x4{mu[0], mu[1], mu[2], mu[3]};
    *reinterpret_cast<f32x4*>(dst + 4) = f32x4{mu[4], mu[5], mu[6], mu[7]};
    *reinterpret_cast<f32x4*>(dst + C) = f32x4{sd[0], sd[1], sd[2], sd[3]};
    *reinterpret_cast<f32x4*>(dst + C + 4) = f32x4{sd[4], sd[5], sd[6], sd[7]};
  }
}

__global__ __launch_bounds__(kAdainNT) void frame_adain_apply_kernel(bf16_t* x, int ldx, int F, int N, int C, int anchor,
                                                                     const float* __restrict__ stats, int nslab,
                                                                     int nchunk) {
  const int tid = threadIdx.x;
  const int cg = tid % kAdainCG, rl = tid / kAdainCG;
  int bid = blockIdx.x;
  const int chunk = bid % nchunk;
  bid /= nchunk;
  const int slab = bid % nslab;
  bid /= nslab;  // clip * (F - 1) + index among the clip's non-anchor frames
  const int b = bid / (F - 1), j = bid - b * (F - 1);
  const int f = j + (j >= anchor ? 1 : 0);
  const int c0 = (slab * kAdainCG + cg) * 8;
  if (c0 >= C) return;

  const float* sf = stats + (size_t)(b * F + f) * 2 * C + c0;
  const float* sa = stats + (size_t)(b * F + anchor) * 2 * C + c0;
  float mu_f[8], mu_a[8], ratio[8];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const f32x4 mf = *reinterpret_cast<const f32x4*>(sf + 4 * h), df = *reinterpret_cast<const f32x4*>(sf + C + 4 * h);
    const f32x4 ma = *reinterpret_cast<const f32x4*>(sa + 4 * h), da = *reinterpret_cast<const f32x4*>(sa + C + 4 * h);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      mu_f[4 * h + c] = mf[c];
      mu_a[4 * h + c] = ma[c];
      ratio[4 * h + c] = da[c] / df[c];  // sd >= sqrt(eps) > 0, or eps == 0 and the caller's columns vary
    }
  }
  bf16_t* base = x + (uint32_t)(b * F + f) * N * ldx + c0;
  const int r1 = min(N, (chunk + 1) * kAdainChunk);
#pragma unroll 4
  for (int r = chunk * kAdainChunk + rl; r < r1; r += kAdainRP) {
    u32x4* p = reinterpret_cast<u32x4*>(base + (uint32_t)r * ldx);
    float v[8];
    unpack8(*p, v);
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = fmaf(v[c] - mu_f[c], ratio[c], mu_a[c]);
    *p = pack8(v);
  }
}

}  // namespace vst

using namespace vst;

extern "C" int vst_frame_adain(void* x, int ldx, int nclip, int F, int N, int C, int anchor, float eps, float* stats,
                               void* stream) {
  if (!x || !stats || nclip <= 0 || F <= 0 || N < 2 || C <= 0 || C % 8) return VST_ERR_ARG;
  if (ldx < C || ldx % 8 || (((uintptr_t)x | (uintptr_t)stats) & 15)) return VST_ERR_ARG;
  if (anchor < 0 || anchor >= F || !(eps >= 0.0f) || !isfinite(eps)) return VST_ERR_ARG;
  const size_t frames = (size_t)nclip * F, rows = frames * N;
  if (rows > 0x7fffffffULL) return VST_ERR_ARG;
  Fit31 fit;
  fit(((rows - 1) * (size_t)ldx + C) * sizeof(bf16_t));
  fit(frames * 2 * (size_t)C * sizeof(float));
  if (fit.over) return VST_ERR_ARG;  // past the kernels' 31-bit offsets
  const int nslab = (C + kAdainCG * 8 - 1) / (kAdainCG * 8);
  const int nchunk = (N + kAdainChunk - 1) / kAdainChunk;
  const size_t nstat = frames * nslab, napply = (size_t)nclip * (F - 1) * nslab * nchunk;
  if (nstat > 0x7fffffffULL || napply > 0x7fffffffULL) return VST_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(frame_adain_stats_kernel, dim3((unsigned)nstat), dim3(kAdainNT), 0, st, (const bf16_t*)x, ldx, N,
                     C, eps, stats, nslab);
  if (F > 1)  // a single frame is its own anchor: statistics only
    hipLaunchKernelGGL(frame_adain_apply_kernel, dim3((unsigned)napply), dim3(kAdainNT), 0, st, (bf16_t*)x, ldx, F, N,
                       C, anchor, (const float*)stats, nslab, nchunk);
  return launch_status();
}
