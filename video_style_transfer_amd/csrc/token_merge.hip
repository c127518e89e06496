// Token merging for the spatial transformer blocks (Bolya & Hoffman, "Token Merging for Fast Stable
// Diffusion", CVPR-W 2023: bipartite_soft_matching_random2d of the tomesd package, restated with a row layout that does
// not depend on a sort order).  No line of the reference does this; the definition is this project's.
//
// Tokens of one image are rows p = y*W + x of a bf16 view.  The image is cut into (H/sy) x (W/sx) whole cells of
// sy x sx tokens; one token per cell, at in-cell offset o(cell), is a destination (Nd of them, in raster order of the
// cells), every other token is a source (Ns = N - Nd, in ascending token index).  o = 0, or with a device seed
//   o(cell) = Philox4x32-10(counter (cell, 0, *step, 2 << 16 | layer), key *seed)[0] % (sy*sx),  (oy, ox) = (o / sx, o % sx)
// (stream 2 of the noise counters of philox.h), never a function of the image: every image of a call shares the pattern.
//
// vst_tome_match, four launches, no atomics, nothing data-dependent in a launch size:
//   1. tome_index_kernel   (one workgroup per image): dst_tok / src_tok and slot[] of the destinations;
//   2. tome_norm_kernel    (one wave per token): 1/|x_p| in fp32, lane-strided squares, then the xor butterfly;
//   3. tome_score_kernel   (one wave per 16 sources): s = <a, b> on v_mfma_f32_16x16x32_bf16 with the 16 sources'
//      fragments kept in registers and the destinations walked in tiles of 16, scaled by the two inverse norms; each
//      lane keeps the running (max, lowest j) of its 4 sources over its destination column, then 16 lanes meet by xor;
//   4. tome_select_kernel  (one workgroup per image): rank counting of `best` in the LDS (ties to the lower index),
//      the r best become merged; prefix sums give the kept sources' rows and the member lists (CSR) of the destinations.
// vst_tome_merge and vst_tome_unmerge_add: one thread per (row, 8 columns); members are summed in ascending token order.
//
// The plan, 6 N + 4 int32 per image (vst_tome_plan_bytes), at these offsets of the image's block:
//   0        slot[N]      merged row of token p: destinations 0 .. Nd-1 (cell raster), kept sources Nd .. N-r-1 (ascending)
//   N        dst_tok[Nd], then src_tok[Ns]
//   2N       node[Ns]     the destination index j of source i's best match (of every source, merged or not)
//   3N       start[Nd + 1], then list[r]: the merged sources' tokens of destination j are list[start[j] .. start[j+1]),
//            ascending (up to N + 1 ints; the section is N + 4 long)
//   4N + 4   kept_tok[Ns - r]: the token of merged row Nd + k
//   5N + 4   inv[N]       fp32 bits: 1 / |x_p|, 0 for a zero row
// The merge and the unmerge clamp what they read from a plan to the image, so a plan of another call cannot send them
// outside the views.
#include <math.h>

#include "philox.h"
#include "vst_common.h"

namespace vst {

constexpr int kTomeMaxN = 4096;
constexpr int kTomeMaxC = 1280;
constexpr int kTomeNT = 1024;  // threads of the per-image kernels

struct TomeGeom {
  int H, W, sy, sx, N, Nd, Ns, r, hc, wc;
};

// offsets (ints) of the plan's sections inside one image's block
__host__ __device__ inline size_t tome_plan_ints(int N) { return (size_t)6 * N + 4; }
__host__ __device__ inline int tome_off_order(int N) { return N; }
__host__ __device__ inline int tome_off_node(int N) { return 2 * N; }
__host__ __device__ inline int tome_off_start(int N) { return 3 * N; }
__host__ __device__ inline int tome_off_kept(int N) { return 4 * N + 4; }
__host__ __device__ inline int tome_off_inv(int N) { return 5 * N + 4; }

__device__ __forceinline__ int tome_clamp(int v, int n) { return min(max(v, 0), n - 1); }

// Exclusive prefix sum of one int per thread over the workgroup, in thread order; `total` is the sum.  wtot: LDS [32].
__device__ __forceinline__ int block_scan_excl(int v, int* wtot, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  __syncthreads();  // wtot may still be read from an earlier call
  if (lane == 63) wtot[wave] = inc;
  __syncthreads();
  int base = 0, tot = 0;
  for (int w = 0; w < nw; ++w) {
    const int t = wtot[w];
    if (w < wave) base += t;
    tot += t;
  }
  total = tot;
  return base + inc - v;
}

__device__ __forceinline__ bool tome_is_dst(const TomeGeom& g, int p, uint64_t seed, uint32_t step, int layer,
                                            bool rnd, int& cell) {
  const int y = p / g.W, x = p - y * g.W;
  const int cy = y / g.sy, cx = x / g.sx;
  if (cy >= g.hc || cx >= g.wc) return false;
  cell = cy * g.wc + cx;
  int o = 0;
  if (rnd) {
    uint32_t w[4];
    noise_bits4(seed, (uint64_t)cell, step, 2u, (uint32_t)layer, w);
    o = (int)(w[0] % (uint32_t)(g.sy * g.sx));
  }
  return (y - cy * g.sy) == o / g.sx && (x - cx * g.sx) == o % g.sx;
}

__global__ __launch_bounds__(kTomeNT) void tome_index_kernel(TomeGeom g, int* __restrict__ plan,
                                                             const uint64_t* __restrict__ seed,
                                                             const int* __restrict__ step_idx, int layer) {
  __shared__ int wtot[32];
  int* pl = plan + (size_t)blockIdx.x * tome_plan_ints(g.N);
  int* order = pl + tome_off_order(g.N);
  const bool rnd = seed != nullptr;
  const uint64_t sd = rnd ? *seed : 0;
  const uint32_t st = rnd ? (uint32_t)*step_idx : 0;
  int base = 0;
  for (int p0 = 0; p0 < g.N; p0 += kTomeNT) {  // (uniform trip count: the scan holds barriers)
    const int p = p0 + (int)threadIdx.x;
    int cell = 0;
    const bool in = p < g.N;
    const bool dst = in && tome_is_dst(g, p, sd, st, layer, rnd, cell);
    int total;
    const int i = base + block_scan_excl(in && !dst ? 1 : 0, wtot, total);
    if (dst) {
      pl[p] = cell;
      order[cell] = p;
    } else if (in) {
      order[g.Nd + i] = p;
    }
    base += total;
  }
}

__global__ __launch_bounds__(256) void tome_norm_kernel(const bf16_t* __restrict__ x, int ldx, int C, int N, int rows,
                                                        int* __restrict__ plan) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const bf16_t* src = x + (size_t)row * ldx;
  float ss = 0.0f;
  for (int c = lane * 8; c < C; c += 512) {
    float f[8];
    unpack8(*reinterpret_cast<const u32x4*>(src + c), f);
#pragma unroll
    for (int k = 0; k < 8; ++k) ss = fmaf(f[k], f[k], ss);
  }
  ss = wave_sum(ss);
  if (lane == 0) {
    const int img = row / N, p = row - img * N;
    const float inv = ss > 0.0f ? 1.0f / sqrtf(ss) : 0.0f;
    plan[(size_t)img * tome_plan_ints(N) + tome_off_inv(N) + p] = __float_as_int(inv);
  }
}

// One wave per 16 sources, KMAX >= C / 32 k-steps of fragments in registers.
template <int KMAX>
__global__ __launch_bounds__(256) void tome_score_kernel(const bf16_t* __restrict__ x, int ldx, int C, TomeGeom g,
                                                         int* __restrict__ plan, float* __restrict__ best) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int img = blockIdx.y;
  const int i0 = (blockIdx.x * 4 + wave) * 16;
  if (i0 >= g.Ns) return;  // (no barrier below)
  const int N = g.N;
  int* pl = plan + (size_t)img * tome_plan_ints(N);
  const int* dst_tok = pl + tome_off_order(N);
  const int* src_tok = dst_tok + g.Nd;
  const float* inv = reinterpret_cast<const float*>(pl + tome_off_inv(N));
  const bf16_t* xi = x + (size_t)img * N * ldx;
  const int nks = C / 32;
  const int r16 = lane & 15, q = lane >> 4;

  bf16x8 af[KMAX];
  {
    const int i = min(i0 + r16, g.Ns - 1);  // rows past Ns repeat the last source; their results are not stored
    const bf16_t* a = xi + (size_t)src_tok[i] * ldx + 8 * q;
#pragma unroll
    for (int ks = 0; ks < KMAX; ++ks)
      if (ks < nks) af[ks] = *reinterpret_cast<const bf16x8*>(a + 32 * ks);
  }
  float ia[4], bs[4];
  int bj[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    ia[t] = inv[src_tok[min(i0 + 4 * q + t, g.Ns - 1)]];
    bs[t] = -INFINITY;
    bj[t] = 0;
  }
  for (int j0 = 0; j0 < g.Nd; j0 += 16) {
    const int j = j0 + r16;
    const int tok = dst_tok[min(j, g.Nd - 1)];
    const bf16_t* b = xi + (size_t)tok * ldx + 8 * q;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int ks = 0; ks < KMAX; ++ks)
      if (ks < nks)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks], *reinterpret_cast<const bf16x8*>(b + 32 * ks), acc, 0, 0,
                                                      0);
    // acc[t]: source row 4 q + t, destination column r16
    const float ib = inv[tok];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      float s = (acc[t] * ia[t]) * ib;
      if (!(s == s)) s = 0.0f;  // an overflowed dot against a zero row: never NaN
      if (j < g.Nd && s > bs[t]) {
        bs[t] = s;
        bj[t] = j;
      }
    }
  }
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float s2 = __shfl_xor(bs[t], o);
      const int j2 = __shfl_xor(bj[t], o);
      if (s2 > bs[t] || (s2 == bs[t] && j2 < bj[t])) {
        bs[t] = s2;
        bj[t] = j2;
      }
    }
  }
  if (r16 == 0) {
    int* node = pl + tome_off_node(N);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int i = i0 + 4 * q + t;
      if (i < g.Ns) {
        best[(size_t)img * g.Ns + i] = bs[t];
        node[i] = bj[t];
      }
    }
  }
}

__global__ __launch_bounds__(kTomeNT) void tome_select_kernel(TomeGeom g, int* __restrict__ plan,
                                                              const float* __restrict__ best) {
  __shared__ float sbest[kTomeMaxN];
  __shared__ int snode[kTomeMaxN];  // the destination of a merged source, -1 for a kept one
  __shared__ int wtot[32];
  const int N = g.N, Ns = g.Ns, Nd = g.Nd, r = g.r;
  const int tid = threadIdx.x;
  int* pl = plan + (size_t)blockIdx.x * tome_plan_ints(N);
  const int* src_tok = pl + tome_off_order(N) + Nd;
  const int* node = pl + tome_off_node(N);
  int* start = pl + tome_off_start(N);
  int* list = start + Nd + 1;
  int* kept_tok = pl + tome_off_kept(N);
  const float* bi = best + (size_t)blockIdx.x * Ns;

  for (int i = tid; i < Ns; i += kTomeNT) sbest[i] = bi[i];
  __syncthreads();
  // rank counting: source i is merged when fewer than r sources beat it (larger best; equal best and lower index)
  for (int i = tid; i < Ns; i += kTomeNT) {
    const float b = sbest[i];
    int c = 0;
    for (int k = 0; k < Ns; ++k) {
      const float o = sbest[k];
      c += (o > b || (o == b && k < i)) ? 1 : 0;
    }
    snode[i] = c < r ? node[i] : -1;
  }
  __syncthreads();
  // rows of the sources: a merged one goes to its destination's row, the kept ones follow the destinations in order
  int base = 0;
  for (int i0 = 0; i0 < Ns; i0 += kTomeNT) {
    const int i = i0 + tid;
    const bool kept = i < Ns && snode[i] < 0;
    int total;
    const int k = base + block_scan_excl(kept ? 1 : 0, wtot, total);
    if (i < Ns) {
      const int tok = src_tok[i];
      if (kept) {
        pl[tok] = Nd + k;
        kept_tok[k] = tok;
      } else {
        pl[tok] = snode[i];
      }
    }
    base += total;
  }
  // member lists of the destinations: counts, their prefix sums, then the tokens in ascending source order
  base = 0;
  for (int j0 = 0; j0 < Nd; j0 += kTomeNT) {
    const int j = j0 + tid;
    int cnt = 0;
    if (j < Nd)
      for (int i = 0; i < Ns; ++i) cnt += snode[i] == j ? 1 : 0;
    int total;
    int at = base + block_scan_excl(cnt, wtot, total);
    if (j < Nd) {
      start[j] = at;
      if (cnt)
        for (int i = 0; i < Ns; ++i)
          if (snode[i] == j) list[at++] = src_tok[i];
    }
    base += total;
  }
  if (tid == 0) start[Nd] = base;
}

__global__ __launch_bounds__(256) void tome_merge_kernel(const bf16_t* __restrict__ x, int ldx, int C, TomeGeom g,
                                                         const int* __restrict__ plan, bf16_t* __restrict__ y, int ldy,
                                                         size_t total) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int cgs = C / 8, Nm = g.N - g.r;
  const int cg = (int)(idx % cgs);
  const size_t row = idx / cgs;
  const int img = (int)(row / Nm), m = (int)(row - (size_t)img * Nm);
  const int* pl = plan + (size_t)img * tome_plan_ints(g.N);
  const bf16_t* xi = x + (size_t)img * g.N * ldx + cg * 8;
  u32x4* out = reinterpret_cast<u32x4*>(y + row * ldy + cg * 8);
  if (m >= g.Nd) {  // a kept source
    *out = *reinterpret_cast<const u32x4*>(xi + (size_t)tome_clamp(pl[tome_off_kept(g.N) + m - g.Nd], g.N) * ldx);
    return;
  }
  const int d = tome_clamp(pl[tome_off_order(g.N) + m], g.N);
  const int* start = pl + tome_off_start(g.N);
  const int* list = start + g.Nd + 1;
  const int s0 = tome_clamp(start[m], g.r + 1), s1 = max(s0, tome_clamp(start[m + 1], g.r + 1));
  const u32x4 dv = *reinterpret_cast<const u32x4*>(xi + (size_t)d * ldx);
  if (s1 == s0) {  // nobody merged into it
    *out = dv;
    return;
  }
  float acc[8], f[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) acc[c] = 0.0f;
  bool added = false;
  for (int s = s0; s < s1; ++s) {
    const int t = tome_clamp(list[s], g.N);
    if (!added && d < t) {  // the destination takes its place in the ascending token order
      unpack8(dv, f);
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[c] += f[c];
      added = true;
    }
    unpack8(*reinterpret_cast<const u32x4*>(xi + (size_t)t * ldx), f);
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] += f[c];
  }
  if (!added) {
    unpack8(dv, f);
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] += f[c];
  }
  const float n = (float)(s1 - s0 + 1);
#pragma unroll
  for (int c = 0; c < 8; ++c) acc[c] = acc[c] / n;
  *out = pack8(acc);
}

__global__ __launch_bounds__(256) void tome_unmerge_kernel(const bf16_t* __restrict__ o, int ldo, int C, int N, int Nm,
                                                           const int* __restrict__ plan, const bf16_t* res, int ldr,
                                                           bf16_t* y, int ldy, size_t total) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int cgs = C / 8;
  const int cg = (int)(idx % cgs);
  const size_t row = idx / cgs;
  const int img = (int)(row / N), p = (int)(row - (size_t)img * N);
  const int m = tome_clamp(plan[(size_t)img * tome_plan_ints(N) + p], Nm);
  const u32x4 ov = *reinterpret_cast<const u32x4*>(o + ((size_t)img * Nm + m) * ldo + cg * 8);
  u32x4* out = reinterpret_cast<u32x4*>(y + row * ldy + cg * 8);
  if (!res) {
    *out = ov;
    return;
  }
  float a[8], b[8];
  unpack8(*reinterpret_cast<const u32x4*>(res + row * ldr + cg * 8), a);
  unpack8(ov, b);
#pragma unroll
  for (int c = 0; c < 8; ++c) a[c] += b[c];
  *out = pack8(a);
}

// The geometry of a call, or a status: 1 for a bad argument, 3 for a size past the kernels' plan.
inline int tome_geom(int nimg, int H, int W, int C, int sy, int sx, int r, TomeGeom& g) {
  if (nimg <= 0 || H <= 0 || W <= 0 || C <= 0 || sy <= 0 || sx <= 0 || r < 0) return VST_ERR_ARG;
  if (sy > H || sx > W || (size_t)sy * sx > 65536) return VST_ERR_ARG;
  if ((size_t)H * W > kTomeMaxN || C % 64 || C > kTomeMaxC) return VST_ERR_UNSUPPORTED;
  g.H = H, g.W = W, g.sy = sy, g.sx = sx, g.N = H * W;
  g.hc = H / sy, g.wc = W / sx;
  g.Nd = g.hc * g.wc, g.Ns = g.N - g.Nd, g.r = r;
  if (r > g.Ns) return VST_ERR_ARG;
  if ((size_t)nimg * g.N > 0x7fffffffULL || nimg > 65535) return VST_ERR_ARG;
  return VST_OK;
}

inline bool tome_view_ok(const void* p, int ld, int C) { return p && ld >= C && ld % 8 == 0 && ((uintptr_t)p & 15) == 0; }

}  // namespace vst

using namespace vst;

extern "C" size_t vst_tome_plan_bytes(int nimg, int N, int r) {
  if (nimg <= 0 || N <= 0 || r < 0 || r > N) return 0;
  return (size_t)nimg * tome_plan_ints(N) * sizeof(int);
}

extern "C" int vst_tome_match(const void* x, int ldx, int nimg, int H, int W, int C, int sy, int sx, int r,
                              const uint64_t* seed, const int* step_idx, int layer, int* plan, float* best,
                              void* stream) {
  TomeGeom g;
  if (const int rc = tome_geom(nimg, H, W, C, sy, sx, r, g)) return rc;
  if (!tome_view_ok(x, ldx, C) || !plan || !best || ((uintptr_t)plan & 15) || ((uintptr_t)best & 3)) return VST_ERR_ARG;
  if ((seed == nullptr) != (step_idx == nullptr) || ((uintptr_t)seed & 7) || ((uintptr_t)step_idx & 3))
    return VST_ERR_ARG;
  if (layer < 0 || layer > 65535) return VST_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int rows = nimg * g.N;
  hipLaunchKernelGGL(tome_index_kernel, dim3(nimg), dim3(kTomeNT), 0, st, g, plan, seed, step_idx, layer);
  hipLaunchKernelGGL(tome_norm_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, (const bf16_t*)x, ldx, C, g.N, rows,
                     plan);
  if (g.Ns > 0) {
    const dim3 grid((g.Ns + 63) / 64, nimg);
    if (C <= 128)
      hipLaunchKernelGGL(tome_score_kernel<4>, grid, dim3(256), 0, st, (const bf16_t*)x, ldx, C, g, plan, best);
    else if (C <= 640)
      hipLaunchKernelGGL(tome_score_kernel<20>, grid, dim3(256), 0, st, (const bf16_t*)x, ldx, C, g, plan, best);
    else
      hipLaunchKernelGGL(tome_score_kernel<40>, grid, dim3(256), 0, st, (const bf16_t*)x, ldx, C, g, plan, best);
  }
  hipLaunchKernelGGL(tome_select_kernel, dim3(nimg), dim3(kTomeNT), 0, st, g, plan, (const float*)best);
  return launch_status();
}

extern "C" int vst_tome_merge(const void* x, int ldx, const int* plan, int nimg, int H, int W, int C, int sy, int sx,
                              int r, void* y, int ldy, void* stream) {
  TomeGeom g;
  if (const int rc = tome_geom(nimg, H, W, C, sy, sx, r, g)) return rc;
  if (!tome_view_ok(x, ldx, C) || !tome_view_ok(y, ldy, C) || !plan || ((uintptr_t)plan & 15)) return VST_ERR_ARG;
  const size_t total = (size_t)nimg * (g.N - r) * (C / 8);
  if ((total + 255) / 256 > 0x7fffffffULL) return VST_ERR_ARG;
  hipLaunchKernelGGL(tome_merge_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)x, ldx, C, g, plan, (bf16_t*)y, ldy, total);
  return launch_status();
}

extern "C" int vst_tome_unmerge_add(const void* o, int ldo, const int* plan, int nimg, int N, int r, int C,
                                    const void* res, int ldr, void* y, int ldy, void* stream) {
  if (nimg <= 0 || N <= 0 || r < 0 || r >= N || C <= 0) return VST_ERR_ARG;
  if (N > kTomeMaxN || C % 64 || C > kTomeMaxC) return VST_ERR_UNSUPPORTED;
  if (!tome_view_ok(o, ldo, C) || !tome_view_ok(y, ldy, C) || (res && !tome_view_ok(res, ldr, C)) || !plan ||
      ((uintptr_t)plan & 15))
    return VST_ERR_ARG;
  if ((size_t)nimg * N > 0x7fffffffULL) return VST_ERR_ARG;
  const size_t total = (size_t)nimg * N * (C / 8);
  if ((total + 255) / 256 > 0x7fffffffULL) return VST_ERR_ARG;
  hipLaunchKernelGGL(tome_unmerge_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)o, ldo, C, N, N - r, plan, (const bf16_t*)res, ldr, (bf16_t*)y, ldy, total);
  return launch_status();
}
