// Normalisations on NHWC / token-major activations ([rows, C], C contiguous).
//
// GroupNorm (32 groups) as used by the denoise path:
//   * ResnetBlock2D norm1/norm2 (eps 1e-5, + SiLU), per frame;
//   * Transformer2DModel.norm (eps 1e-6), per frame (unziplora_unet/transformer_2d.py:222-235);
//   * motion-module norm (eps 1e-6) over the 5-D (B,C,F,H,W) tensor, i.e. statistics span
//     every frame of a clip (diffusers AnimateDiffTransformer3D);
//   * conv_norm_out (eps 1e-5, + SiLU).
// A "sample" is `rows_per_sample` consecutive rows (H*W for per-frame, F*H*W per clip).
// Three launches: partial (sum, sumsq) per (sample, chunk, group) -> merge to (mean, rstd)
// with Chan's parallel-variance combine -> apply (+optional SiLU), bf16 out.  The input may
// be two channel-concatenated sources (up-block skip concat), so the concat is never
// materialised for the normalised branch.
//
// LayerNorm over C per row (BasicTransformerBlock norm1/2/3, eps 1e-5), optionally adding the
// sinusoidal frame position table pe[(row / pe_div) % pe_mod] after the affine transform
// (motion-module blocks add the PE to the normed input before attn1 and attn2).
#include "vst_common.h"

#include <limits.h>

namespace vst {

constexpr int kGnStatsU = 8;  // independent 16-B loads in flight per thread, statistics pass
constexpr int kGnApplyU = 4;  // ... apply pass
constexpr int kLnlMI = 2;     // 16-row fragments per layernorm_lora workgroup

// A thread's place in the launch geometry of the row-walking GroupNorm kernels (GnGeom on the host side): grid
// (nchunk, nsamples), workgroup `chunk` of sample `s` owns rows [r_beg, r_end) of it and has rps x CH threads; this
// thread walks rows r_beg + rph, + rps, ... at channels [c, c + 8).
struct GnThread {
  int s, chunk, rps, r_beg, r_end, rph, c;
};
__device__ __forceinline__ GnThread gn_thread(int C, int rows_per_sample, int rpc) {
  const int CH = C / 8;
  GnThread t;
  t.s = blockIdx.y;
  t.chunk = blockIdx.x;
  t.rps = blockDim.x / CH;
  t.r_beg = t.chunk * rpc;
  t.r_end = min(rows_per_sample, t.r_beg + rpc);
  t.rph = threadIdx.x / CH;
  t.c = (threadIdx.x % CH) * 8;
  return t;
}

// x1: [rows, C1] (ld1), x2: [rows, C2] (ld2): base pointer / stride of the source holding channel c
__device__ __forceinline__ void gn_src(const bf16_t* x1, int ld1, int C1, const bf16_t* x2, int ld2, int c,
                                       const bf16_t*& base, int& ld) {
  if (c < C1) { base = x1 + c; ld = ld1; }
  else { base = x2 + (c - C1); ld = ld2; }
}

__global__ __launch_bounds__(512) void gn_stats_kernel(const bf16_t* __restrict__ x1, int ld1, int C1,
                                                       const bf16_t* __restrict__ x2, int ld2, int C2,
                                                       int rows_per_sample, int rpc, int groups,
                                                       float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float gsm[];  // [rps][C] sums then sumsqs
  const int C = C1 + C2;
  const GnThread t = gn_thread(C, rows_per_sample, rpc);
  const int s = t.s, chunk = t.chunk, nchunk = gridDim.x, rps = t.rps, rph = t.rph, c = t.c;
  const int tid = threadIdx.x;
  const bf16_t* base;
  int ld;
  gn_src(x1, ld1, C1, x2, ld2, c, base, ld);
  base += (size_t)s * rows_per_sample * ld;
  float a[8], q[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { a[e] = 0.f; q[e] = 0.f; }
  constexpr int U = kGnStatsU;
  for (int r = t.r_beg + rph; r < t.r_end; r += U * rps) {
    u32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int rr = r + u * rps;
      v[u] = rr < t.r_end ? *reinterpret_cast<const u32x4*>(base + (size_t)rr * ld) : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float f[8];
      unpack8(v[u], f);
#pragma unroll
      for (int e = 0; e < 8; ++e) { a[e] += f[e]; q[e] += f[e] * f[e]; }
    }
  }
  float* ssum = gsm;
  float* ssq = gsm + rps * C;
#pragma unroll
  for (int e = 0; e < 8; ++e) { ssum[rph * C + c + e] = a[e]; ssq[rph * C + c + e] = q[e]; }
  __syncthreads();
  // fold the row phases column-parallel into row 0, then one wave per group sums its Cg columns by
  // shuffles (a serial per-group loop over rps x Cg LDS reads was ~10 us of latency per workgroup)
  for (int cc = tid; cc < C; cc += blockDim.x) {
    float sa = ssum[cc], sq = ssq[cc];
    for (int rr = 1; rr < rps; ++rr) { sa += ssum[rr * C + cc]; sq += ssq[rr * C + cc]; }
    ssum[cc] = sa;
    ssq[cc] = sq;
  }
  __syncthreads();
  const int Cg = C / groups;
  const int lane = tid & 63, wave = tid >> 6, nwave = blockDim.x >> 6;  // full waves only
  for (int gi = wave; wave < nwave && gi < groups; gi += nwave) {
    float sa = 0.f, sq = 0.f;
    for (int cc = lane; cc < Cg; cc += 64) { sa += ssum[gi * Cg + cc]; sq += ssq[gi * Cg + cc]; }
    sa = wave_sum(sa);
    sq = wave_sum(sq);
    if (lane == 0) {
      float* o = part + (((size_t)s * nchunk + chunk) * groups + gi) * 2;
      o[0] = sa;
      o[1] = sq;
    }
  }
}

// Tail of gn_finalize_kernel, one 64-thread block per (sample b, group gi): a, q = this lane's part of
// the group's sum and sum of squares over `count` elements.  Butterfly in double, then the per-channel affine
// y = x * scale[b,c] + shift[b,c]  (scale = rstd*gamma, shift = beta - mean*rstd*gamma) so the apply pass is one
// FMA per element, and (backward) the optional (mean, rstd) per (sample, group).
__device__ __forceinline__ void gn_finalize_tail(double a, double q, double count, int b, int gi, int Cg, int C,
                                                 float eps, const float* __restrict__ gamma,
                                                 const float* __restrict__ beta, float* __restrict__ scale,
                                                 float* __restrict__ shift, float* __restrict__ stats) {
  const int lane = threadIdx.x;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o);
    q += __shfl_xor(q, o);
  }
  const double mean = a / count;
  const double var = fmax(q / count - mean * mean, 0.0);
  const float rstd = (float)(1.0 / sqrt(var + (double)eps));
  for (int c = gi * Cg + lane; c < (gi + 1) * Cg; c += 64) {
    const float sc = rstd * gamma[c];
    scale[(size_t)b * C + c] = sc;
    shift[(size_t)b * C + c] = beta[c] - (float)mean * sc;
  }
  if (stats != nullptr && lane == 0) {
    stats[(size_t)blockIdx.x * 2] = (float)mean;
    stats[(size_t)blockIdx.x * 2 + 1] = rstd;
  }
}

// Merge a sample's chunk partials (sum, sumsq) in one fixed order (lane-strided over (global frame, chunk), then the
// butterfly), read from the rank-major layout [P][nclips][Fl][nck][G][2].  Per-frame and per-clip GroupNorms of one
// launch (vst_groupnorm, vst_groupnorm_bwd) are P = 1, Fl = 1: [nsamples][nchunk][G][2].  The motion-module GroupNorm
// (statistics over every frame of a clip), frame-sharded or not, builds its statistics from per-FRAME chunk partials
// (gn_stats_kernel with one sample per frame, chunking that depends only on the frame's row count), so a rank
// holding some frames of a clip produces exactly the partials the unsharded forward produces for those frames, and
// the all-gather leaves them rank-major (P = 1: the unsharded layout): the sharded and unsharded statistics are the
// same bits whatever P is.
__global__ __launch_bounds__(64) void gn_finalize_kernel(const float* __restrict__ part, int P, int nclips, int Fl,
                                                         int nck, int groups, int Cg, double count, float eps,
                                                         const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float* __restrict__ scale,
                                                         float* __restrict__ shift, int C,
                                                         float* __restrict__ stats) {
  const int b = blockIdx.x / groups, gi = blockIdx.x - b * groups;
  const int per_rank = Fl * nck;  // a rank's partials of one clip are contiguous, in (frame, chunk) order
  double a = 0.0, q = 0.0;
  for (int c = threadIdx.x; c < P * per_rank; c += 64) {  // c: the clip's partials in (global frame, chunk) order
    const int r = P == 1 ? 0 : c / per_rank;
    const float* p = part + ((((size_t)r * nclips + b) * per_rank + (c - r * per_rank)) * groups + gi) * 2;
    a += p[0];
    q += p[1];
  }
  gn_finalize_tail(a, q, count, b, gi, Cg, C, eps, gamma, beta, scale, shift, stats);
}

// ---- GroupNorm backward (training path) ----
// z = x * scale + shift (the forward's affine, recomputed), dz = g (or g * silu'(z) with the fused SiLU).
// Pass 1 (gn_bwd_sums): per (sample, chunk) and channel, sum dz and dz * x (same geometry as gn_stats).
// Pass 2 (gn_bwd_finalize): per (sample, group), A = mean(gamma dz), B = mean(gamma dz x^) ->
//   dx = a_c dz + b0 + b1 x  with a_c = rstd gamma_c, b0 = rstd^2 mean B - rstd A, b1 = -rstd^2 B,
//   and the per-(sample, channel) sums for dgamma / dbeta.  Pass 3 (gn_bwd_apply) writes dx; gn_bwd_param sums
//   dgamma_c = sum_s rstd (S_dzx - mean S_dz), dbeta_c = sum_s S_dz in a fixed order.
__device__ __forceinline__ float silu_grad(float z) {
  const float sg = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-z * 1.4426950408889634f));
  return sg * (1.0f + z * (1.0f - sg));
}
__device__ __forceinline__ float gn_dz(float g, float x, float sc, float sh, int act) {
  return act ? g * silu_grad(x * sc + sh) : g;
}
// this thread's 8 channels of the forward's affine (sample s, channels [c, c + 8))
__device__ __forceinline__ void gn_load_affine(const float* __restrict__ scale, const float* __restrict__ shift,
                                               size_t sc0, float* sc, float* sh) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    sc[e] = scale[sc0 + e];
    sh[e] = shift[sc0 + e];
  }
}

__global__ __launch_bounds__(512) void gn_bwd_sums_kernel(const bf16_t* __restrict__ x, int ldx,
                                                          const bf16_t* __restrict__ g, int ldg, int C,
                                                          int rows_per_sample, int rpc, const float* __restrict__ scale,
                                                          const float* __restrict__ shift, int act,
                                                          float* __restrict__ part2) {
  extern __shared__ __attribute__((aligned(16))) float bsm[];  // [rps][C] sum dz, then [rps][C] sum dz*x
  const GnThread t = gn_thread(C, rows_per_sample, rpc);
  const int s = t.s, chunk = t.chunk, nchunk = gridDim.x, rps = t.rps, rph = t.rph, c = t.c;
  const int tid = threadIdx.x;
  const size_t row0 = (size_t)s * rows_per_sample;
  float sc[8], sh[8], a[8], q[8];
  gn_load_affine(scale, shift, (size_t)s * C + c, sc, sh);
#pragma unroll
  for (int e = 0; e < 8; ++e) { a[e] = 0.f; q[e] = 0.f; }
  for (int r = t.r_beg + rph; r < t.r_end; r += rps) {
    float xv[8], gv[8];
    unpack8(*reinterpret_cast<const u32x4*>(x + (row0 + r) * ldx + c), xv);
    unpack8(*reinterpret_cast<const u32x4*>(g + (row0 + r) * ldg + c), gv);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float dz = gn_dz(gv[e], xv[e], sc[e], sh[e], act);
      a[e] += dz;
      q[e] += dz * xv[e];
    }
  }
  float* s1 = bsm;
  float* s2 = bsm + rps * C;
#pragma unroll
  for (int e = 0; e < 8; ++e) { s1[rph * C + c + e] = a[e]; s2[rph * C + c + e] = q[e]; }
  __syncthreads();
  for (int cc = tid; cc < C; cc += blockDim.x) {
    float u = 0.f, v = 0.f;
    for (int rr = 0; rr < rps; ++rr) { u += s1[rr * C + cc]; v += s2[rr * C + cc]; }
    part2[(((size_t)s * nchunk + chunk) * 2) * C + cc] = u;
    part2[(((size_t)s * nchunk + chunk) * 2 + 1) * C + cc] = v;
  }
}

__global__ __launch_bounds__(64) void gn_bwd_finalize_kernel(const float* __restrict__ part2, int nchunk, int C,
                                                             int groups, int rows_per_sample,
                                                             const float* __restrict__ stats,
                                                             const float* __restrict__ gamma,
                                                             float* __restrict__ chsum, float* __restrict__ coef) {
  const int s = blockIdx.x / groups, gi = blockIdx.x - s * groups;
  const int lane = threadIdx.x;
  const int Cg = C / groups;
  const float mean = stats[(size_t)blockIdx.x * 2], rstd = stats[(size_t)blockIdx.x * 2 + 1];
  double A = 0.0, Bq = 0.0;
  for (int c = gi * Cg + lane; c < (gi + 1) * Cg; c += 64) {
    double sdz = 0.0, sdzx = 0.0;
    for (int ch = 0; ch < nchunk; ++ch) {
      sdz += part2[(((size_t)s * nchunk + ch) * 2) * C + c];
      sdzx += part2[(((size_t)s * nchunk + ch) * 2 + 1) * C + c];
    }
    chsum[((size_t)s * 2) * C + c] = (float)sdz;
    chsum[((size_t)s * 2 + 1) * C + c] = (float)(rstd * (sdzx - (double)mean * sdz));  // sum dz * x^
    A += gamma[c] * sdz;
    Bq += gamma[c] * (sdzx - (double)mean * sdz);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    A += __shfl_xor(A, o);
    Bq += __shfl_xor(Bq, o);
  }
  const double n = (double)rows_per_sample * Cg;
  const double Am = A / n, Bm = (double)rstd * Bq / n;
  const float b0 = (float)((double)rstd * rstd * mean * Bm - (double)rstd * Am);
  const float b1 = (float)(-(double)rstd * rstd * Bm);
  for (int c = gi * Cg + lane; c < (gi + 1) * Cg; c += 64) {
    coef[((size_t)s * C + c) * 3] = rstd * gamma[c];
    coef[((size_t)s * C + c) * 3 + 1] = b0;
    coef[((size_t)s * C + c) * 3 + 2] = b1;
  }
}

__global__ __launch_bounds__(512) void gn_bwd_apply_kernel(const bf16_t* __restrict__ x, int ldx,
                                                           const bf16_t* __restrict__ g, int ldg, int C,
                                                           int rows_per_sample, int rpc,
                                                           const float* __restrict__ scale,
                                                           const float* __restrict__ shift, int act,
                                                           const float* __restrict__ coef, bf16_t* __restrict__ dx,
                                                           int lddx) {
  const GnThread t = gn_thread(C, rows_per_sample, rpc);
  const int s = t.s, c = t.c;
  const size_t row0 = (size_t)s * rows_per_sample;
  float sc[8], sh[8], ca[8], c0[8], c1[8];
  gn_load_affine(scale, shift, (size_t)s * C + c, sc, sh);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    ca[e] = coef[((size_t)s * C + c + e) * 3];
    c0[e] = coef[((size_t)s * C + c + e) * 3 + 1];
    c1[e] = coef[((size_t)s * C + c + e) * 3 + 2];
  }
  for (int r = t.r_beg + t.rph; r < t.r_end; r += t.rps) {
    float xv[8], gv[8], o[8];
    unpack8(*reinterpret_cast<const u32x4*>(x + (row0 + r) * ldx + c), xv);
    unpack8(*reinterpret_cast<const u32x4*>(g + (row0 + r) * ldg + c), gv);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float dz = gn_dz(gv[e], xv[e], sc[e], sh[e], act);
      o[e] = ca[e] * dz + c0[e] + c1[e] * xv[e];
    }
    *reinterpret_cast<u32x4*>(dx + (row0 + r) * lddx + c) = pack8(o);
  }
}

__global__ __launch_bounds__(256) void gn_bwd_param_kernel(const float* __restrict__ chsum, int nsamples, int C,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float db = 0.f, dg = 0.f;
  for (int s = 0; s < nsamples; ++s) {
    db += chsum[((size_t)s * 2) * C + c];
    dg += chsum[((size_t)s * 2 + 1) * C + c];
  }
  dgamma[c] = dg;
  dbeta[c] = db;
}

__global__ __launch_bounds__(512) void gn_apply_kernel(const bf16_t* __restrict__ x1, int ld1, int C1,
                                                       const bf16_t* __restrict__ x2, int ld2, int C2,
                                                       int rows_per_sample, int rpc, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, int act,
                                                       bf16_t* __restrict__ y, int ldy) {
  const int C = C1 + C2;
  const GnThread t = gn_thread(C, rows_per_sample, rpc);
  const int s = t.s, rps = t.rps, r_end = t.r_end, c = t.c;
  const bf16_t* base;
  int ld;
  gn_src(x1, ld1, C1, x2, ld2, c, base, ld);
  const size_t row0 = (size_t)s * rows_per_sample;
  base += row0 * ld;
  bf16_t* yb = y + row0 * ldy + c;
  // this thread's 8 channels of one sample: the affine is loaded once
  const f32x4* sc = reinterpret_cast<const f32x4*>(scale + (size_t)s * C + c);
  const f32x4* sh = reinterpret_cast<const f32x4*>(shift + (size_t)s * C + c);
  const f32x4 a0 = sc[0], a1 = sc[1], b0 = sh[0], b1 = sh[1];
  constexpr int U = kGnApplyU;
  for (int r = t.r_beg + t.rph; r < r_end; r += U * rps) {
    u32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int rr = r + u * rps;
      v[u] = rr < r_end ? *reinterpret_cast<const u32x4*>(base + (size_t)rr * ld) : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int rr = r + u * rps;
      if (rr >= r_end) break;
      float f[8];
      unpack8(v[u], f);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        f[e] = f[e] * a0[e] + b0[e];
        f[e + 4] = f[e + 4] * a1[e] + b1[e];
      }
      if (act) {
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = silu(f[e]);
      }
      *reinterpret_cast<u32x4*>(yb + (size_t)rr * ldy) = pack8(f);
    }
  }
}

// One wave per row, lane l holding the 8-channel chunks l, l + 64, ... (up to MAXCH of them) -- the row layout of
// layernorm_kernel and layernorm_bwd_kernel.  Chunks past C, and every chunk of a row that is not `live`, are zeros.
template <int MAXCH>
__device__ __forceinline__ void ln_load_row(const bf16_t* __restrict__ row, bool live, int lane, int CH,
                                            float (&v)[MAXCH][8]) {
#pragma unroll
  for (int i = 0; i < MAXCH; ++i) {
    const int cc = lane + 64 * i;
    u32x4 raw = u32x4{0u, 0u, 0u, 0u};
    if (cc < CH && live) raw = *reinterpret_cast<const u32x4*>(row + cc * 8);
    unpack8(raw, v[i]);
  }
}
// Two-pass row statistics: sum -> mean, then squared deviations over the real channels only -> rstd.
template <int MAXCH>
__device__ __forceinline__ void ln_row_stats(const float (&v)[MAXCH][8], int lane, int CH, int C, float eps,
                                             float& mean, float& rstd) {
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < MAXCH; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) sum += v[i][e];  // zero-filled past C
  mean = wave_sum(sum) / C;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < MAXCH; ++i) {
    if (lane + 64 * i < CH) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = v[i][e] - mean; sq += d * d; }
    }
  }
  rstd = rsqrtf(wave_sum(sq) / C + eps);
}

// LayerNorm: each wave normalises ROWS rows (all their 16-B loads issued before any reduction, so
// ROWS x MAXCH loads are in flight per lane), up to MAXCH 8-channel chunks per lane and row.
template <int MAXCH, int ROWS>
__global__ __launch_bounds__(256) void layernorm_kernel(const bf16_t* __restrict__ x, int ldx, int C, int rows,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        float eps, const float* __restrict__ pe, int pe_div, int pe_mod,
                                                        bf16_t* __restrict__ y, int ldy) {
  const int lane = threadIdx.x & 63;
  const int row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * ROWS;
  if (row0 >= rows) return;
  const int CH = C / 8;
  float v[ROWS][MAXCH][8];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) ln_load_row<MAXCH>(x + (size_t)(row0 + r) * ldx, row0 + r < rows, lane, CH, v[r]);
  float gg[MAXCH][8], bb[MAXCH][8];
#pragma unroll
  for (int i = 0; i < MAXCH; ++i) {
    const int cc = lane + 64 * i;
    if (cc < CH) {
      const f32x4* g4 = reinterpret_cast<const f32x4*>(gamma + cc * 8);
      const f32x4* b4 = reinterpret_cast<const f32x4*>(beta + cc * 8);
      const f32x4 g0 = g4[0], g1 = g4[1], b0 = b4[0], b1 = b4[1];
#pragma unroll
      for (int e = 0; e < 4; ++e) { gg[i][e] = g0[e]; gg[i][e + 4] = g1[e]; bb[i][e] = b0[e]; bb[i][e + 4] = b1[e]; }
    }
  }
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    const int row = row0 + r;
    if (row >= rows) break;
    float mean, rstd;
    ln_row_stats<MAXCH>(v[r], lane, CH, C, eps, mean, rstd);
    const float* pr = pe ? pe + (size_t)((row / pe_div) % pe_mod) * C : nullptr;
#pragma unroll
    for (int i = 0; i < MAXCH; ++i) {
      const int cc = lane + 64 * i;
      if (cc < CH) {
        float o[8];
        if (pr) {
          const f32x4* p4 = reinterpret_cast<const f32x4*>(pr + cc * 8);
          const f32x4 p0 = p4[0], p1 = p4[1];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            o[e] = (v[r][i][e] - mean) * (rstd * gg[i][e]) + bb[i][e] + p0[e];
            o[e + 4] = (v[r][i][e + 4] - mean) * (rstd * gg[i][e + 4]) + bb[i][e + 4] + p1[e];
          }
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = (v[r][i][e] - mean) * (rstd * gg[i][e]) + bb[i][e];
        }
        *reinterpret_cast<u32x4*>(y + (size_t)row * ldy + cc * 8) = pack8(o);
      }
    }
  }
}

// LayerNorm for C = 40 * LPR (320 / 640 / 1280): LPR lanes per row, each holding CPL = 5 interleaved 16-B chunks
// (lane l of a row reads chunks l, l + LPR, ...: every load instruction covers whole 128-B+ row segments), so all 64
// lanes work for every C (the generic kernel above idles 37 % of its lanes at C = 320) and a wave normalises
// 64 / LPR rows per pass; RIT passes' loads are all issued before the first reduction.  Row statistics are two-pass
// (mean, then squared deviations), reduced over the row's LPR lanes by xor shuffles.
template <int LPR, int RIT>
__global__ __launch_bounds__(256) void layernorm_g_kernel(const bf16_t* __restrict__ x, int ldx, int C, int rows,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float eps,
                                                          const float* __restrict__ pe, int pe_div, int pe_mod,
                                                          bf16_t* __restrict__ y, int ldy) {
  constexpr int CPL = 5, RPW = 64 / LPR;
  __shared__ f32x4 sgb[2][CPL * LPR * 2];  // gamma, beta of the row (C = 40 LPR floats = 10 LPR f32x4)
  const int lane = threadIdx.x & 63, l = lane % LPR, rsub = lane / LPR;
  const int row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW * RIT;
  float v[RIT][CPL][8];
#pragma unroll
  for (int it = 0; it < RIT; ++it) {
    const int row = row0 + it * RPW + rsub;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      u32x4 raw = u32x4{0u, 0u, 0u, 0u};
      if (row < rows) raw = *reinterpret_cast<const u32x4*>(x + (size_t)row * ldx + (l + LPR * i) * 8);
      unpack8(raw, v[it][i]);
    }
  }
  // gamma / beta staged once per workgroup (every wave of it used to fetch the whole row's 10 LPR x 32 B through the
  // vector memory path per row pass: 4x the row's own bytes)
  for (int i = threadIdx.x; i < CPL * LPR * 2; i += 256) {
    sgb[0][i] = reinterpret_cast<const f32x4*>(gamma)[i];
    sgb[1][i] = reinterpret_cast<const f32x4*>(beta)[i];
  }
  __syncthreads();
  if (row0 >= rows) return;
  const float invc = 1.0f / (float)C;
#pragma unroll
  for (int it = 0; it < RIT; ++it) {
    const int row = row0 + it * RPW + rsub;
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i)
#pragma unroll
      for (int e = 0; e < 8; ++e) sum += v[it][i][e];
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    const float mean = sum * invc;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i)
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = v[it][i][e] - mean; sq = fmaf(d, d, sq); }
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
    const float rstd = rsqrtf(fmaf(sq, invc, eps));  // (explicit fmas: codegen-independent rounding)
    if (row >= rows) continue;
    const float* pr = pe ? pe + (size_t)((row / pe_div) % pe_mod) * C : nullptr;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const int c0 = (l + LPR * i) * 8;
      const f32x4 g0 = sgb[0][c0 / 4], g1 = sgb[0][c0 / 4 + 1];
      const f32x4 b0 = sgb[1][c0 / 4], b1 = sgb[1][c0 / 4 + 1];
      float o[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[e] = fmaf(v[it][i][e] - mean, rstd * g0[e], b0[e]);
        o[e + 4] = fmaf(v[it][i][e + 4] - mean, rstd * g1[e], b1[e]);
      }
      if (pr) {
        const f32x4 p0 = *reinterpret_cast<const f32x4*>(pr + c0), p1 = *reinterpret_cast<const f32x4*>(pr + c0 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { o[e] += p0[e]; o[e + 4] += p1[e]; }
      }
      *reinterpret_cast<u32x4*>(y + (size_t)row * ldy + c0) = pack8(o);
    }
  }
}

// LayerNorm fused with the UnZipLoRA down-projection of the projections that consume its output
// (BasicTransformerBlock norm1 -> attn1 q/k/v, norm2 -> attn2 q): y = LN(x) (bf16, as the reference's
// LayerNorm output) and u = y . Acat^T (Acat: [R, C] bf16, R <= 64 a multiple of 16), reading x once.
// A workgroup = 8 waves owns 32 rows; wave w holds the k32-chunks w, w+8, ... of both 16-row
// fragments in registers in the 16x16x32 MFMA operand layout (lane l: row l&15, 8 channels at
// chunk*32 + 8*(l>>4)).  Row statistics are two-pass (mean, then sum of squared deviations) reduced
// over the 4 lanes of a row by shuffles and over the 8 waves through LDS; the normalised bf16 values
// are stored (16 B per lane) and fed straight to the MFMAs; the 8 partial u tiles are summed via LDS.
template <int NJ, int MAXT>
__global__ __launch_bounds__(512, 2) void layernorm_lora_kernel(const bf16_t* __restrict__ x, int ldx, int C, int rows,
                                                                const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, float eps,
                                                                const bf16_t* __restrict__ A, int R,
                                                                bf16_t* __restrict__ y, int ldy, bf16_t* __restrict__ u,
                                                                int ldu) {
  constexpr int MI = kLnlMI, NW = 8;  // MAXT = ceil(C / 256) k32-chunks per wave (C <= 256 * MAXT)
  __shared__ f32x4 red[NW][MI][NJ][64];
  __shared__ float st[NW][MI][16];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 15, kc = (lane >> 4) * 8;
  const int m0 = blockIdx.x * 16 * MI;
  const int nk = C / 32;
  const auto rx = make_rsrc(x, (uint32_t)min<size_t>(((size_t)(rows - 1) * ldx + C) * 2, 0x7fffffffULL));
  u32x4 raw[MAXT][MI];  // x kept packed (bf16) in registers; unpacked per pass
  bool rowok[MI];
#pragma unroll
  for (int i = 0; i < MI; ++i) rowok[i] = m0 + 16 * i + r < rows;
#pragma unroll
  for (int t = 0; t < MAXT; ++t) {
    const int ks = w + NW * t;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int off = (ks < nk && rowok[i]) ? ((m0 + 16 * i + r) * ldx + ks * 32 + kc) * 2 : kOOB;
      raw[t][i] = buf_load16(rx, off);
    }
  }
  // ---- mean ----
  float s[MI];
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    s[i] = 0.f;
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
      float v[8];
      unpack8(raw[t][i], v);
#pragma unroll
      for (int e = 0; e < 8; ++e) s[i] += v[e];  // zero-filled beyond C
    }
    s[i] += __shfl_xor(s[i], 16);
    s[i] += __shfl_xor(s[i], 32);
    if (lane < 16) st[w][i][lane] = s[i];
  }
  __syncthreads();
  float mean[MI];
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    float a = 0.f;
#pragma unroll
    for (int q = 0; q < NW; ++q) a += st[q][i][r];
    mean[i] = a / C;
  }
  __syncthreads();
  // ---- variance (deviations from the mean, only over real channels) ----
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    float q2 = 0.f;
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
      if (w + NW * t < nk) {
        float v[8];
        unpack8(raw[t][i], v);
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float d = v[e] - mean[i]; q2 += d * d; }
      }
    }
    q2 += __shfl_xor(q2, 16);
    q2 += __shfl_xor(q2, 32);
    if (lane < 16) st[w][i][lane] = q2;
  }
  __syncthreads();
  float rstd[MI];
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    float a = 0.f;
#pragma unroll
    for (int q = 0; q < NW; ++q) a += st[q][i][r];
    rstd[i] = rsqrtf(a / C + eps);
  }
  // ---- normalise, store y, u partials on MFMA ----
  const auto ra = make_rsrc(A, (uint32_t)((size_t)R * C * 2));
  f32x4 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < MAXT; ++t) {
    const int ks = w + NW * t;
    if (ks >= nk) break;  // wave-uniform
    const int c = ks * 32 + kc;
    const f32x4* g4 = reinterpret_cast<const f32x4*>(gamma + c);
    const f32x4* b4 = reinterpret_cast<const f32x4*>(beta + c);
    const f32x4 g0 = g4[0], g1 = g4[1], b0 = b4[0], b1 = b4[1];
    u32x4 wf[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) wf[j] = buf_load16(ra, (16 * j + r) < R ? ((16 * j + r) * C + c) * 2 : kOOB);
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      float v[8], o[8];
      unpack8(raw[t][i], v);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[e] = (v[e] - mean[i]) * (rstd[i] * g0[e]) + b0[e];
        o[e + 4] = (v[e + 4] - mean[i]) * (rstd[i] * g1[e]) + b1[e];
      }
      const u32x4 pk = pack8(o);
      if (rowok[i]) *reinterpret_cast<u32x4*>(y + (size_t)(m0 + 16 * i + r) * ldy + c) = pk;
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(&wf[j]),
                                                            *reinterpret_cast<const bf16x8*>(&pk), acc[i][j], 0, 0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) red[w][i][j][lane] = acc[i][j];
  __syncthreads();
  if (w >= MI) return;
  const int i = w;
  const int m = m0 + 16 * i + r;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    f32x4 sum = red[0][i][j][lane];
#pragma unroll
    for (int q = 1; q < NW; ++q) sum += red[q][i][j][lane];
    const int n = 16 * j + 4 * (lane >> 4);  // sum[e] = u[m][n + e]
    if (m < rows && n < R) {
      u32x2 pv;
      pv[0] = pack2bf(sum[0], sum[1]);
      pv[1] = pack2bf(sum[2], sum[3]);
      *reinterpret_cast<u32x2*>(u + (size_t)m * ldu + n) = pv;
    }
  }
}


// LayerNorm backward (training path): one wave per row, grid-stride over rows.
//   x^ = (x - mean) * rstd (recomputed, two-pass), gg = g * gamma,
//   dx = rstd * (gg - mean(gg) - x^ * mean(gg * x^)),  dgamma += g * x^,  dbeta += g.
// The per-channel sums are kept per lane, folded over the 4 waves in LDS and written as one [2][C] partial per
// workgroup; layernorm_bwd_reduce_kernel sums the partials in a fixed order (deterministic).
template <int MAXCH>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const bf16_t* __restrict__ x, int ldx,
                                                            const bf16_t* __restrict__ g, int ldg, int C, int rows,
                                                            const float* __restrict__ gamma, float eps,
                                                            bf16_t* __restrict__ dx, int lddx, float* __restrict__ part) {
  __shared__ float red[4][2][MAXCH * 512];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int CH = C / 8;
  float gm[MAXCH][8], dg[MAXCH][8], db[MAXCH][8];
#pragma unroll
  for (int i = 0; i < MAXCH; ++i) {
    const int cc = lane + 64 * i;
#pragma unroll
    for (int e = 0; e < 8; ++e) { gm[i][e] = cc < CH ? gamma[cc * 8 + e] : 0.f; dg[i][e] = 0.f; db[i][e] = 0.f; }
  }
  for (int row = blockIdx.x * 4 + w; row < rows; row += gridDim.x * 4) {
    float xv[MAXCH][8], gv[MAXCH][8];
    ln_load_row<MAXCH>(x + (size_t)row * ldx, true, lane, CH, xv);
    ln_load_row<MAXCH>(g + (size_t)row * ldg, true, lane, CH, gv);
    float mean, rstd;
    ln_row_stats<MAXCH>(xv, lane, CH, C, eps, mean, rstd);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < MAXCH; ++i)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float xh = (xv[i][e] - mean) * rstd;
        const float gg = gv[i][e] * gm[i][e];
        xv[i][e] = xh;
        s1 += gg;
        s2 += gg * xh;
        dg[i][e] += gv[i][e] * xh;
        db[i][e] += gv[i][e];
      }
    s1 = wave_sum(s1) / C;
    s2 = wave_sum(s2) / C;
#pragma unroll
    for (int i = 0; i < MAXCH; ++i) {
      const int cc = lane + 64 * i;
      if (cc < CH) {
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = rstd * (gv[i][e] * gm[i][e] - s1 - xv[i][e] * s2);
        *reinterpret_cast<u32x4*>(dx + (size_t)row * lddx + cc * 8) = pack8(o);
      }
    }
  }
  if (!part) return;  // frozen LayerNorm (spatial path): no dgamma / dbeta
#pragma unroll
  for (int i = 0; i < MAXCH; ++i) {
    const int cc = lane + 64 * i;
#pragma unroll
    for (int e = 0; e < 8; ++e) { red[w][0][cc * 8 + e] = dg[i][e]; red[w][1][cc * 8 + e] = db[i][e]; }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) { a += red[q][0][c]; b += red[q][1][c]; }
    part[((size_t)blockIdx.x * 2) * C + c] = a;
    part[((size_t)blockIdx.x * 2 + 1) * C + c] = b;
  }
}

// 16 columns per workgroup x 16 partial-block stripes (a stripe reads 64 contiguous bytes), combined in a fixed
// order through LDS (deterministic).
__global__ __launch_bounds__(256) void layernorm_bwd_reduce_kernel(const float* __restrict__ part, int nblk, int C,
                                                                   float* __restrict__ dgamma, float* __restrict__ dbeta) {
  __shared__ float red[16][17];
  const int lc = threadIdx.x & 15, q = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + lc;
  float a = 0.f;
  if (c < 2 * C) {
    const int which = c / C, cc = c - which * C;
    for (int b = q; b < nblk; b += 16) a += part[((size_t)b * 2 + which) * C + cc];
  }
  red[q][lc] = a;
  __syncthreads();
  if (q == 0 && c < 2 * C) {
    const int which = c / C, cc = c - which * C;
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += red[k][lc];
    (which ? dbeta : dgamma)[cc] = t;
  }
}

}  // namespace vst

using namespace vst;

// rows per workgroup.  Forward GroupNorms: a function of the sample's (frame's) row count only -- never of how many
// samples share the launch -- so a frame's statistics are the same bits in a batch of any size (the frame-sharded
// forward runs 1/P of the frames per rank, tests/test_frame_shard.py asserts equality); rows / 8 gives >= 8 chunks
// per frame, >= 256 workgroups at the denoise step's 32 frames (the same chunking the old total-rows rule picked
// there: 32 / 128 / 256 rows at 16x16 / 32x32 / 64x64).  Backward (vst_groupnorm_bwd, per-clip samples of the
// training step): >= ~256 workgroups over the whole launch (swept 256..4096 with tools/norm_bench.py).
static inline int gn_rpc_rows(int rows_per_sample) {
  return std::max(8, std::min(256, (rows_per_sample + 7) / 8));
}
static inline int gn_rpc(int nsamples, int rows_per_sample) {
  constexpr long long target = 256;
  const long long total = (long long)nsamples * rows_per_sample;
  return (int)std::max<long long>(8, std::min<long long>(256, (total + target - 1) / target));
}

// Launch geometry shared by the row-walking passes (GnThread on the device side): grid (nchunk, nsamples), each
// workgroup owns `rpc` consecutive rows of one sample and has rps x CH threads (CH = C/8 16-B channel chunks per
// row, rps = 512 / CH rows in flight per step), so no lane idles whatever C is, and `rpc` is chosen by the rules
// above so that every launch has >= ~256 workgroups (the 16x16-latent GroupNorms have only 256 rows per frame: one
// 256-row chunk per sample gave 32 workgroups and 0.7 TB/s).
struct GnGeom {
  int C, CH, rps, rpc, nchunk;
  size_t lds;  // [2][rps][C] floats: the stats and backward-sums passes' row-phase fold
  GnGeom(int C_, int rows_per_sample, int rpc_)
      : C(C_), CH(C_ / 8), rps(std::max(1, 512 / std::max(1, C_ / 8))), rpc(rpc_),
        nchunk((rows_per_sample + rpc_ - 1) / rpc_), lds((size_t)2 * rps * C_ * sizeof(float)) {}
  dim3 grid(int nsamples) const { return dim3(nchunk, nsamples); }
  dim3 block() const { return dim3(rps * CH); }
  // floats of the [nsamples][nchunk][groups][2] partials, rounded up so what follows stays 16-B aligned
  size_t part_floats(int nsamples, int groups) const {
    return ((size_t)nsamples * nchunk * groups * 2 + 3) & ~(size_t)3;
  }
};
static inline GnGeom gn_fwd_geom(int C, int rows_per_sample) {
  return GnGeom(C, rows_per_sample, gn_rpc_rows(rows_per_sample));
}

static void launch_gn_stats(const GnGeom& gm, int nsamples, const void* x1, int ld1, int C1, const void* x2, int ld2,
                            int C2, int rows_per_sample, int groups, float* part, hipStream_t s) {
  hipLaunchKernelGGL(gn_stats_kernel, gm.grid(nsamples), gm.block(), gm.lds, s, (const bf16_t*)x1, ld1, C1,
                     (const bf16_t*)x2, ld2, C2, rows_per_sample, gm.rpc, groups, part);
}
static void launch_gn_apply(const GnGeom& gm, int nsamples, const void* x1, int ld1, int C1, const void* x2, int ld2,
                            int C2, int rows_per_sample, const float* scale, const float* shift, int silu_act, void* y,
                            int ldy, hipStream_t s) {
  hipLaunchKernelGGL(gn_apply_kernel, gm.grid(nsamples), gm.block(), 0, s, (const bf16_t*)x1, ld1, C1,
                     (const bf16_t*)x2, ld2, C2, rows_per_sample, gm.rpc, scale, shift, silu_act, (bf16_t*)y, ldy);
}

// the argument conditions every GroupNorm entry point shares; each adds its own
static int gn_check(const void* x1, int ld1, int C1, const void* x2, int ld2, int C2, int nsamples,
                    int rows_per_sample, int groups) {
  const int C = C1 + (x2 ? C2 : 0);
  if (!x1 || nsamples <= 0 || rows_per_sample <= 0 || groups <= 0) return VST_ERR_ARG;
  if (C % groups || C % 8 || C1 % 8 || (ld1 & 7) || (x2 && (ld2 & 7))) return VST_ERR_ARG;
  if (C > 4096) return VST_ERR_ARG;
  return VST_OK;
}

extern "C" size_t vst_groupnorm_workspace_bytes(int nsamples, int rows_per_sample, int groups, int C) {
  return (gn_fwd_geom(C, rows_per_sample).part_floats(nsamples, groups) + (size_t)2 * nsamples * C) * sizeof(float);
}

extern "C" int vst_groupnorm(const void* x1, int ld1, int C1, const void* x2, int ld2, int C2, int nsamples,
                             int rows_per_sample, int groups, float eps, const float* gamma, const float* beta,
                             int silu_act, void* y, int ldy, void* workspace, void* stream) {
  if (gn_check(x1, ld1, C1, x2, ld2, C2, nsamples, rows_per_sample, groups) || !y || !workspace || !gamma || !beta ||
      (ldy & 7))
    return VST_ERR_ARG;
  if (!x2) C2 = 0;
  const int C = C1 + C2;
  hipStream_t s = (hipStream_t)stream;
  const GnGeom gm = gn_fwd_geom(C, rows_per_sample);
  float* part = (float*)workspace;
  float* scale = part + gm.part_floats(nsamples, groups);
  float* shift = scale + (size_t)nsamples * C;
  launch_gn_stats(gm, nsamples, x1, ld1, C1, x2, ld2, C2, rows_per_sample, groups, part, s);
  hipLaunchKernelGGL(gn_finalize_kernel, dim3(nsamples * groups), dim3(64), 0, s, part, 1, nsamples, 1, gm.nchunk,
                     groups, C / groups, (double)rows_per_sample * (C / groups), eps, gamma, beta, scale, shift, C,
                     (float*)nullptr);
  launch_gn_apply(gm, nsamples, x1, ld1, C1, x2, ld2, C2, rows_per_sample, scale, shift, silu_act, y, ldy, s);
  return launch_status();
}

extern "C" int vst_groupnorm_frame_chunks(int rows_per_frame) {
  return rows_per_frame > 0 ? gn_fwd_geom(0, rows_per_frame).nchunk : 0;  // (the chunking does not depend on C)
}

extern "C" int vst_groupnorm_frame_partials(const void* x1, int ld1, int C1, int nframes, int rows_per_frame,
                                            int groups, float* part, void* stream) {
  if (gn_check(x1, ld1, C1, nullptr, 0, 0, nframes, rows_per_frame, groups) || !part) return VST_ERR_ARG;
  launch_gn_stats(gn_fwd_geom(C1, rows_per_frame), nframes, x1, ld1, C1, nullptr, 0, 0, rows_per_frame, groups, part,
                  (hipStream_t)stream);
  return launch_status();
}

extern "C" int vst_groupnorm_apply_partials(const void* x1, int ld1, int C1, int nclips, int frames_local,
                                            int rows_per_frame, int groups, const float* part, int nranks, float eps,
                                            const float* gamma, const float* beta, int silu_act, void* y, int ldy,
                                            float* scale_shift, void* stream) {
  if (gn_check(x1, ld1, C1, nullptr, 0, 0, nclips * frames_local, rows_per_frame, groups) || nclips <= 0 ||
      frames_local <= 0 || nranks <= 0 || !part || !y || !gamma || !beta || !scale_shift || (ldy & 7) ||
      ((uintptr_t)scale_shift & 15) || (nclips * C1) % 4)
    return VST_ERR_ARG;
  const int C = C1;
  hipStream_t s = (hipStream_t)stream;
  float* scale = scale_shift;
  float* shift = scale + (size_t)nclips * C;
  const int rpc = gn_rpc_rows(rows_per_frame);  // the frame's chunking, for the statistics and the apply alike
  const int nck = GnGeom(C, rows_per_frame, rpc).nchunk;
  const double count = (double)nranks * frames_local * rows_per_frame * (C / groups);
  hipLaunchKernelGGL(gn_finalize_kernel, dim3(nclips * groups), dim3(64), 0, s, part, nranks, nclips, frames_local,
                     nck, groups, C / groups, count, eps, gamma, beta, scale, shift, C, (float*)nullptr);
  const int rows_per_clip = frames_local * rows_per_frame;
  launch_gn_apply(GnGeom(C, rows_per_clip, rpc), nclips, x1, ld1, C1, nullptr, 0, 0, rows_per_clip, scale, shift,
                  silu_act, y, ldy, s);
  return launch_status();
}

extern "C" int vst_layernorm(const void* x, int ldx, int C, int rows, const float* gamma, const float* beta,
                             float eps, const float* pe, int pe_div, int pe_mod, void* y, int ldy, void* stream) {
  if (!x || !y || !gamma || !beta || rows <= 0 || C <= 0 || C % 8 || (ldx & 7) || (ldy & 7)) return VST_ERR_ARG;
  if (pe && (pe_div <= 0 || pe_mod <= 0)) return VST_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int CH = C / 8;
  const dim3 blk(256);
#define VST_LNG(LPR, RIT)                                                                                      \
  hipLaunchKernelGGL((layernorm_g_kernel<LPR, RIT>), dim3((rows + 4 * (64 / LPR) * RIT - 1) / (4 * (64 / LPR) * RIT)), \
                     blk, 0, s, (const bf16_t*)x, ldx, C, rows, gamma, beta, eps, pe, pe_div, pe_mod, (bf16_t*)y, ldy)
#define VST_LN(MC, R)                                                                                          \
  hipLaunchKernelGGL((layernorm_kernel<MC, R>), dim3((rows + 4 * R - 1) / (4 * R)), blk, 0, s, (const bf16_t*)x, ldx, \
                     C, rows, gamma, beta, eps, pe, pe_div, pe_mod, (bf16_t*)y, ldy)
  // A/B switch (tools/ab_bench.sh): on when the variable is set at all, whatever its value
  static const bool generic_only = env_int("VST_LN_GENERIC", INT_MIN) != INT_MIN;
  const bool g16 = !generic_only && ((uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)pe) % 16 == 0;
  // RIT = row passes per wave whose loads are all in flight before the first reduction.  C = 1280 (M = 8192 rows in the
  // step): 1 pass, 1024 workgroups: 9.8 -> 9.2 us per launch graph-timed, step -0.15..-0.2 ms same-box
  // (profiles/r3_ab_ln_rit.txt).
  if (g16 && C == 320) VST_LNG(8, 2);
  else if (g16 && C == 640) VST_LNG(16, 2);
  else if (g16 && C == 1280) VST_LNG(32, 1);
  else if (CH <= 64) VST_LN(1, 4);
  else if (CH <= 128) VST_LN(2, 2);
  else if (CH <= 256) VST_LN(4, 2);
  else return VST_ERR_ARG;
#undef VST_LNG
#undef VST_LN
  return launch_status();
}

extern "C" int vst_layernorm_lora(const void* x, int ldx, int C, int rows, const float* gamma, const float* beta,
                                  float eps, const void* A, int R, void* y, int ldy, void* u, int ldu, void* stream) {
  if (!x || !y || !u || !A || !gamma || !beta || rows <= 0 || C <= 0 || (C & 31) || C > 1280) return VST_ERR_ARG;
  if (R <= 0 || R > 64 || (R & 15) || (ldx & 7) || (ldy & 7) || (ldu & 3) || ldu < R) return VST_ERR_ARG;
  if (((size_t)(rows - 1) * ldx + C) * 2 > 0x7fffffffULL) return VST_ERR_ARG;  // x through a 32-bit buffer offset
  const dim3 grid((rows + 16 * kLnlMI - 1) / (16 * kLnlMI)), blk(512);
  hipStream_t s = (hipStream_t)stream;
#define VST_LNL(NJ, MT)                                                                                         \
  hipLaunchKernelGGL((layernorm_lora_kernel<NJ, MT>), grid, blk, 0, s, (const bf16_t*)x, ldx, C, rows, gamma, beta, \
                     eps, (const bf16_t*)A, R, (bf16_t*)y, ldy, (bf16_t*)u, ldu)
#define VST_LNL_T(NJ)             \
  if (C <= 256) VST_LNL(NJ, 1);   \
  else if (C <= 512) VST_LNL(NJ, 2); \
  else if (C <= 768) VST_LNL(NJ, 3); \
  else VST_LNL(NJ, 5);
  switch (R / 16) {
    case 1: VST_LNL_T(1); break;
    case 2: VST_LNL_T(2); break;
    case 3: VST_LNL_T(3); break;
    default: VST_LNL_T(4); break;
  }
#undef VST_LNL_T
#undef VST_LNL
  return launch_status();
}

// fp32 residual stream + LayerNorm (the CLIP text encoders, text_encoder.py): h_out = h + y (y bf16, optional),
// n = LN(h_out) in bf16 (the projection input).  The reference's text towers are fp32 modules under bf16 autocast:
// their residual stream stays fp32, only the matmul outputs are bf16 -- so this path keeps it fp32 too.  One
// workgroup of 256 threads per row, two-pass statistics (C <= 2048).
__global__ __launch_bounds__(256) void residual_layernorm_kernel(const float* __restrict__ h, int ldh,
                                                                 const bf16_t* __restrict__ y, int ldy, int C,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, float eps,
                                                                 float* __restrict__ ho, int ldho,
                                                                 bf16_t* __restrict__ n, int ldn) {
  __shared__ float red[4];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  float v[8];
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int c = tid + 256 * e;
    float x = 0.f;
    if (c < C) {
      x = h[(size_t)row * ldh + c];
      if (y) x += bf2f(y[(size_t)row * ldy + c]);
      ho[(size_t)row * ldho + c] = x;
    }
    v[e] = x;
    s += x;
  }
  s = wave_sum(s);
  if (lane == 0) red[w] = s;
  __syncthreads();
  const float mean = (red[0] + red[1] + red[2] + red[3]) / C;
  __syncthreads();
  float q = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e)
    if (tid + 256 * e < C) { const float d = v[e] - mean; q += d * d; }
  q = wave_sum(q);
  if (lane == 0) red[w] = q;
  __syncthreads();
  const float rstd = rsqrtf((red[0] + red[1] + red[2] + red[3]) / C + eps);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int c = tid + 256 * e;
    if (c < C) n[(size_t)row * ldn + c] = f2bf((v[e] - mean) * rstd * gamma[c] + beta[c]);
  }
}

extern "C" int vst_residual_layernorm(const float* h, int ldh, const void* y, int ldy, int rows, int C,
                                      const float* gamma, const float* beta, float eps, float* h_out, int ldho,
                                      void* n, int ldn, void* stream) {
  if (!h || !h_out || !n || !gamma || !beta || rows <= 0 || C <= 0 || C > 2048 || ldh < C || ldho < C || ldn < C ||
      (y && ldy < C))
    return VST_ERR_ARG;
  hipLaunchKernelGGL(residual_layernorm_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, h, ldh,
                     (const bf16_t*)y, ldy, C, gamma, beta, eps, h_out, ldho, (bf16_t*)n, ldn);
  return launch_status();
}

// ---- LayerNorm backward (training path) ----
static inline int lnb_grid(int rows) { return std::max(1, std::min(512, (rows + 3) / 4)); }

extern "C" size_t vst_layernorm_bwd_workspace_bytes(int C, int rows) {
  return (size_t)lnb_grid(rows) * 2 * C * sizeof(float);
}

extern "C" int vst_layernorm_bwd(const void* x, int ldx, const void* g, int ldg, int C, int rows, const float* gamma,
                                 float eps, void* dx, int lddx, float* dgamma, float* dbeta, void* workspace,
                                 void* stream) {
  // dgamma == dbeta == NULL: dx only (frozen affine), no workspace needed
  if (!x || !g || !dx || !gamma || (!dgamma) != (!dbeta) || (dgamma && !workspace) || rows <= 0 || C <= 0 ||
      C % 8 || (ldx & 7) || (ldg & 7) || (lddx & 7) || C > 2048)
    return VST_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int grid = lnb_grid(rows);
  float* part = dgamma ? (float*)workspace : nullptr;
  const int CH = C / 8;
#define VST_LNB(MC)                                                                                            \
  hipLaunchKernelGGL((layernorm_bwd_kernel<MC>), dim3(grid), dim3(256), 0, s, (const bf16_t*)x, ldx, (const bf16_t*)g, \
                     ldg, C, rows, gamma, eps, (bf16_t*)dx, lddx, part)
  if (CH <= 64) VST_LNB(1);
  else if (CH <= 128) VST_LNB(2);
  else VST_LNB(4);
#undef VST_LNB
  if (dgamma)
    hipLaunchKernelGGL(layernorm_bwd_reduce_kernel, dim3((2 * C + 15) / 16), dim3(256), 0, s, part, grid, C, dgamma,
                       dbeta);
  return launch_status();
}

// ---- GroupNorm backward host side ----
// Workspace carve, in floats, every piece 16-B aligned: part | scale, shift | stats | part2 | chsum | coef.
struct GnBwdWs {
  size_t scale, stats, part2, chsum, coef, total;  // (part is at 0, shift at scale + nsamples * C)
};
static GnBwdWs gn_bwd_ws(const GnGeom& gm, int nsamples, int groups) {
  auto up = [](size_t n) { return (n + 3) / 4 * 4; };
  const size_t nsC = (size_t)nsamples * gm.C;
  GnBwdWs w;
  w.scale = gm.part_floats(nsamples, groups);
  w.stats = w.scale + up(2 * nsC);
  w.part2 = w.stats + up((size_t)2 * nsamples * groups);
  w.chsum = w.part2 + up((size_t)nsamples * gm.nchunk * 2 * gm.C);
  w.coef = w.chsum + up(2 * nsC);
  w.total = w.coef + up(3 * nsC);
  return w;
}

extern "C" size_t vst_groupnorm_bwd_workspace_bytes(int nsamples, int rows_per_sample, int groups, int C) {
  const GnGeom gm(C, rows_per_sample, gn_rpc(nsamples, rows_per_sample));
  return gn_bwd_ws(gm, nsamples, groups).total * sizeof(float);
}

extern "C" int vst_groupnorm_bwd(const void* x, int ldx, const void* g, int ldg, int C, int nsamples,
                                 int rows_per_sample, int groups, float eps, const float* gamma, const float* beta,
                                 int silu_act, void* dx, int lddx, float* dgamma, float* dbeta, void* workspace,
                                 void* stream) {
  if (gn_check(x, ldx, C, nullptr, 0, 0, nsamples, rows_per_sample, groups) || !g || !dx || !gamma || !beta ||
      !dgamma || !dbeta || !workspace || (ldg & 7) || (lddx & 7))
    return VST_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const GnGeom gm(C, rows_per_sample, gn_rpc(nsamples, rows_per_sample));
  const GnBwdWs w = gn_bwd_ws(gm, nsamples, groups);
  float* part = (float*)workspace;
  float* scale = part + w.scale;
  float* shift = scale + nsamples * (size_t)C;
  float* stats = part + w.stats;
  float* part2 = part + w.part2;
  float* chsum = part + w.chsum;
  float* coef = part + w.coef;
  launch_gn_stats(gm, nsamples, x, ldx, C, nullptr, 0, 0, rows_per_sample, groups, part, s);
  hipLaunchKernelGGL(gn_finalize_kernel, dim3(nsamples * groups), dim3(64), 0, s, part, 1, nsamples, 1, gm.nchunk,
                     groups, C / groups, (double)rows_per_sample * (C / groups), eps, gamma, beta, scale, shift, C,
                     stats);
  hipLaunchKernelGGL(gn_bwd_sums_kernel, gm.grid(nsamples), gm.block(), gm.lds, s, (const bf16_t*)x, ldx,
                     (const bf16_t*)g, ldg, C, rows_per_sample, gm.rpc, scale, shift, silu_act, part2);
  hipLaunchKernelGGL(gn_bwd_finalize_kernel, dim3(nsamples * groups), dim3(64), 0, s, part2, gm.nchunk, C, groups,
                     rows_per_sample, stats, gamma, chsum, coef);
  hipLaunchKernelGGL(gn_bwd_apply_kernel, gm.grid(nsamples), gm.block(), 0, s, (const bf16_t*)x, ldx,
                     (const bf16_t*)g, ldg, C, rows_per_sample, gm.rpc, scale, shift, silu_act, coef, (bf16_t*)dx, lddx);
  hipLaunchKernelGGL(gn_bwd_param_kernel, dim3((C + 255) / 256), dim3(256), 0, s, chsum, nsamples, C, dgamma, dbeta);
  return launch_status();
}
