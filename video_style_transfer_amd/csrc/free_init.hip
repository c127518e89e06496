// FreeInit's frequency mix (Wu et al., "FreeInit: Bridging Initialization Gap in Video Diffusion
// Models", ECCV 2024; diffusers' FreeInitMixin._apply_free_init): per (clip, channel) volume of F x H x W fp32 values,
//   z = x + init - r,   out = r + L z,   L = IDFT3 o (filt .) o DFT3,
// filt the low-pass mask in unshifted DFT order, symmetric under k -> -k (free_init.dft_order), so that L is a real
// operator and the W axis needs only the W / 2 + 1 bins of a real transform.
//
// Nothing here is a fast transform: every axis is a dense DFT in fp32 on a (cos, sin)(2 pi j / N) table indexed by
// (k n) mod N exactly, so any size runs the same code and every sum has an order fixed by (F, H, W) alone.  Three
// launches, the spectrum [B Cl][F][H][W / 2 + 1] (re, im) in the caller's workspace between them:
//   1. plane forward: one workgroup per (b, c, f) plane builds z in the LDS (r from `noise`, or regenerated from the
//      Philox counters of philox.h), transforms the rows (real input, half spectrum), then the columns;
//   2. frame axis: one workgroup per 64 spectrum points of a (b, c) volume: length-F transform, times
//      filt / (F H W), inverse length-F transform, in place;
//   3. plane inverse: columns, then rows back to real values, `+ r` at the store (r generated again, never stored).
// LDS lanes run along the W axis of the spectrum in the column passes (consecutive float2: no bank conflict) and the
// operand that differs per row is read at an odd row stride.
#include "philox.h"
#include "vst_common.h"

namespace vst {

// threads of a plane workgroup: the 64 x 33 bins of a 64 x 64 plane in three rounds, so that the few workgroups of a
// short clip (64 at 16 frames x 4 channels, on 256 CUs) finish sooner
constexpr int kMixPlaneNT = 1024;
constexpr int kMixNT = 256;    // threads of a frame-axis workgroup
constexpr int kMixMaxN = 128;  // longest axis
constexpr int kMixPts = 64;    // spectrum points per workgroup of the frame-axis pass (one per lane)
constexpr int kMixMaxLds = 160 * 1024;

struct MixArgs {
  const float* x;
  const float* init;   // NULL: z = x - r
  const float* noise;  // NULL: r from the Philox counters
  float* out;
  const float* filt;
  float scale;
  const uint64_t* seed;
  const int* iter;
  uint32_t stream_id;
  int B, Cl, F, H, W;
  float2* spec;
};

// (cos, sin)(2 pi j / n), j < n, rounded once from double
__device__ __forceinline__ void fill_twiddle(float2* tw, int n, int tid, int nt) {
  for (int j = tid; j < n; j += nt) {
    double sn, cs;
    sincospi(2.0 * j / n, &sn, &cs);
    tw[j] = make_float2((float)cs, (float)sn);
  }
}

// The next index of a walk through a twiddle table of n entries in steps of `step` < n: (k step) mod n, exactly and
// without a division.
__device__ __forceinline__ int tw_next(int j, int step, int n) {
  j += step;
  return j >= n ? j - n : j;
}

// a += v t (INV) or v conj(t)
template <bool INV>
__device__ __forceinline__ void cfma(float2& a, const float2 v, const float2 t) {
  if (INV) {
    a.x = fmaf(v.x, t.x, fmaf(-v.y, t.y, a.x));
    a.y = fmaf(v.y, t.x, fmaf(v.x, t.y, a.y));
  } else {
    a.x = fmaf(v.x, t.x, fmaf(v.y, t.y, a.x));
    a.y = fmaf(v.y, t.x, fmaf(-v.x, t.y, a.y));
  }
}

// sum_{k < n} v[k stride] e^{-+ 2 pi i k step / n} (INV: +): even and odd k in two accumulators (two shorter sums, and
// two independent FMA chains), added at the end; the order is a function of n alone.
template <bool INV>
__device__ __forceinline__ float2 dense_dft(const float2* v, int stride, const float2* tw, int step, int n) {
  float2 a0 = make_float2(0.0f, 0.0f), a1 = a0;
  int j = 0, k = 0;
  for (; k + 1 < n; k += 2) {
    const float2 t0 = tw[j];
    j = tw_next(j, step, n);
    const float2 t1 = tw[j];
    j = tw_next(j, step, n);
    cfma<INV>(a0, v[k * stride], t0);
    cfma<INV>(a1, v[(k + 1) * stride], t1);
  }
  if (k < n) cfma<INV>(a0, v[k * stride], tw[j]);
  return make_float2(a0.x + a1.x, a0.y + a1.y);
}

// r of element (b, c, f, p): scale * noise[g], or scale * the normal vst_noise_normal stores there.  One product,
// never contracted into what follows, so both launches that need r (and both sources of it) hold the same bits.
struct MixNoise {
  const float* noise;
  float scale;
  uint64_t key, pos0;
  uint32_t step, stream_id, group;
  bool hi, odd;
  __device__ __forceinline__ MixNoise(const MixArgs& a, int b, int c, int f)
      : noise(a.noise), scale(a.scale), key(0), pos0(0), step(0), stream_id(a.stream_id), group((uint32_t)c >> 2),
        hi((c & 2) != 0), odd((c & 1) != 0) {
    if (!noise) {
      key = *a.seed;
      step = (uint32_t)*a.iter;
      pos0 = noise_position(b, a.F, f, a.H * a.W, 0);
    }
  }
  __device__ __forceinline__ float operator()(size_t g, int p) const {
#pragma clang fp contract(off)
    float n;
    if (noise) {
      n = noise[g];
    } else {
      uint32_t w[4];
      float nn[4];
      noise_bits4(key, pos0 + (uint64_t)p, step, stream_id, group, w);
      if (hi) w[0] = w[2], w[1] = w[3];  // the pair of this channel first: the other pair's Box-Muller is dead code
      normals_of_bits4(w, nn);
      n = odd ? nn[1] : nn[0];
    }
    return scale * n;
  }
};

// ---- 1. z = x + init - r of one (b, c, f) plane, rows then columns, to spec[plane][kh][kw] ----
__global__ __launch_bounds__(kMixPlaneNT) void mix_plane_fwd_kernel(MixArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int H = a.H, W = a.W, Wh = W / 2 + 1, Whp = Wh | 1, Wp = W | 1;
  float2* A = reinterpret_cast<float2*>(smem);  // [H][Whp] row spectra
  float2* twW = A + (size_t)H * Whp;            // [W]
  float2* twH = twW + W;                        // [H]
  float* z = reinterpret_cast<float*>(twH + H);  // [H][Wp]
  const int tid = threadIdx.x;
  const size_t plane = blockIdx.x;  // (b * Cl + c) * F + f
  const int f = (int)(plane % a.F);
  const int bc = (int)(plane / a.F);
  const int c = bc % a.Cl, b = bc / a.Cl;
  const int HW = H * W;
  const size_t g0 = plane * (size_t)HW;

  fill_twiddle(twW, W, tid, kMixPlaneNT);
  fill_twiddle(twH, H, tid, kMixPlaneNT);
  const MixNoise r(a, b, c, f);
  for (int i = tid; i < HW; i += kMixPlaneNT) {
#pragma clang fp contract(off)
    const int h = i / W, w = i - h * W;
    float v = a.x[g0 + i];
    if (a.init) v += a.init[g0 + i];
    z[h * Wp + w] = v - r(g0 + i, i);
  }
  __syncthreads();

  // rows: A[h][kw] = sum_w z[h][w] e^{-2 pi i kw w / W}, kw <= W / 2 (lanes along kw: z[h][w] is a broadcast)
  for (int i = tid; i < H * Wh; i += kMixPlaneNT) {
    const int h = i / Wh, kw = i - h * Wh;
    const float* zr = z + h * Wp;
    float2 a0 = make_float2(0.0f, 0.0f), a1 = a0;  // even and odd w, as dense_dft
    int j = 0, w = 0;
    for (; w + 1 < W; w += 2) {
      const float2 t0 = twW[j];
      j = tw_next(j, kw, W);
      const float2 t1 = twW[j];
      j = tw_next(j, kw, W);
      a0.x = fmaf(zr[w], t0.x, a0.x), a0.y = fmaf(-zr[w], t0.y, a0.y);
      a1.x = fmaf(zr[w + 1], t1.x, a1.x), a1.y = fmaf(-zr[w + 1], t1.y, a1.y);
    }
    if (w < W) a0.x = fmaf(zr[w], twW[j].x, a0.x), a0.y = fmaf(-zr[w], twW[j].y, a0.y);
    const float re = a0.x + a1.x, im = a0.y + a1.y;
    A[h * Whp + kw] = make_float2(re, im);
  }
  __syncthreads();

  // columns: S[kh][kw] = sum_h A[h][kw] e^{-2 pi i kh h / H} (lanes along kw: consecutive float2 of one row of A)
  float2* dst = a.spec + plane * (size_t)(H * Wh);
  for (int i = tid; i < H * Wh; i += kMixPlaneNT) {
    const int kh = i / Wh, kw = i - kh * Wh;
    dst[i] = dense_dft<false>(A + kw, Whp, twH, kh, H);
  }
}

// ---- 2. the frame axis of 64 spectrum points: forward, times filt / (F H W), inverse, in place ----
__global__ __launch_bounds__(kMixNT) void mix_frames_kernel(MixArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int F = a.F, H = a.H, W = a.W, Wh = W / 2 + 1, NP = H * Wh;
  float2* S = reinterpret_cast<float2*>(smem);  // [F][64]
  float2* T = S + (size_t)F * kMixPts;          // [F][64]
  float2* twF = T + (size_t)F * kMixPts;        // [F]
  const int tid = threadIdx.x, pl = tid & (kMixPts - 1), row0 = tid / kMixPts;
  constexpr int kRows = kMixNT / kMixPts;
  const int p = blockIdx.x * kMixPts + pl;  // this thread's point in every pass
  const bool live = p < NP;
  float2* vol = a.spec + (size_t)blockIdx.y * F * NP;

  fill_twiddle(twF, F, tid, kMixNT);
  for (int f = row0; f < F; f += kRows) S[f * kMixPts + pl] = live ? vol[(size_t)f * NP + p] : make_float2(0.0f, 0.0f);
  __syncthreads();

  const int kh = live ? p / Wh : 0, kw = live ? p - kh * Wh : 0;
  const float inv = 1.0f / ((float)F * (float)H * (float)W);
  for (int kf = row0; kf < F; kf += kRows) {  // kf is uniform in a wave: the twiddle is a broadcast
    const float2 v = dense_dft<false>(S + pl, kMixPts, twF, kf, F);
    const float m = live ? a.filt[((size_t)kf * H + kh) * W + kw] * inv : 0.0f;
    T[kf * kMixPts + pl] = make_float2(v.x * m, v.y * m);
  }
  __syncthreads();

  for (int f = row0; f < F; f += kRows) {
    if (live) vol[(size_t)f * NP + p] = dense_dft<true>(T + pl, kMixPts, twF, f, F);
  }
}

// ---- 3. one (b, c, f) plane back: columns, then rows to real values, out = r + that ----
__global__ __launch_bounds__(kMixPlaneNT) void mix_plane_inv_kernel(MixArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int H = a.H, W = a.W, Wh = W / 2 + 1, Whp = Wh | 1;
  float2* Sp = reinterpret_cast<float2*>(smem);  // [H][Wh] the plane's spectrum
  float2* G = Sp + (size_t)H * Wh;               // [H][Whp] after the columns
  float2* twW = G + (size_t)H * Whp;             // [W]
  float2* twH = twW + W;                         // [H]
  const int tid = threadIdx.x;
  const size_t plane = blockIdx.x;
  const int f = (int)(plane % a.F);
  const int bc = (int)(plane / a.F);
  const int c = bc % a.Cl, b = bc / a.Cl;
  const int HW = H * W;
  const size_t g0 = plane * (size_t)HW;

  fill_twiddle(twW, W, tid, kMixPlaneNT);
  fill_twiddle(twH, H, tid, kMixPlaneNT);
  const float2* src = a.spec + plane * (size_t)(H * Wh);
  for (int i = tid; i < H * Wh; i += kMixPlaneNT) Sp[i] = src[i];
  __syncthreads();

  // columns: G[h][kw] = sum_kh S[kh][kw] e^{+2 pi i kh h / H}
  for (int i = tid; i < H * Wh; i += kMixPlaneNT) {
    const int h = i / Wh, kw = i - h * Wh;
    G[h * Whp + kw] = dense_dft<true>(Sp + kw, Wh, twH, h, H);
  }
  __syncthreads();

  // rows: the value is real, G[h][W - kw] = conj G[h][kw]:
  //   o[h][w] = Re G[0] + 2 sum_{0 < kw < W / 2} Re(G[kw] e^{+2 pi i kw w / W}) + (W even) (-1)^w Re G[W / 2]
  const MixNoise r(a, b, c, f);
  const int npair = (W - 1) / 2;
  for (int i = tid; i < HW; i += kMixPlaneNT) {
#pragma clang fp contract(off)
    const int h = i / W, w = i - h * W;
    const float2* g = G + h * Whp;
    float acc = 0.0f, acc1 = 0.0f;  // odd and even kw, as dense_dft
    int j = w, kw = 1;
    for (; kw + 1 <= npair; kw += 2) {
      const float2 t0 = twW[j];
      j = tw_next(j, w, W);
      const float2 t1 = twW[j];
      j = tw_next(j, w, W);
      acc = fmaf(g[kw].x, t0.x, fmaf(-g[kw].y, t0.y, acc));
      acc1 = fmaf(g[kw + 1].x, t1.x, fmaf(-g[kw + 1].y, t1.y, acc1));
    }
    if (kw <= npair) acc = fmaf(g[kw].x, twW[j].x, fmaf(-g[kw].y, twW[j].y, acc));
    acc += acc1;
    float o = g[0].x + 2.0f * acc;
    if (!(W & 1)) o += (w & 1) ? -g[W / 2].x : g[W / 2].x;
    a.out[g0 + i] = r(g0 + i, i) + o;
  }
}

static size_t mix_spec_bytes(int B, int Cl, int F, int H, int W) {
  return (size_t)B * Cl * F * H * (W / 2 + 1) * sizeof(float2);
}

// Host side: [lo, hi) of an operand in bytes.
struct MixSpan {
  uintptr_t lo, hi;
  MixSpan(const void* p, size_t bytes) : lo((uintptr_t)p), hi((uintptr_t)p + bytes) {}
  bool overlaps(const MixSpan& o) const { return lo && o.lo && lo < o.hi && o.lo < hi; }
};

template <class Kern>
static bool mix_lds_attr(Kern k) {
  return hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, kMixMaxLds) == hipSuccess;
}

}  // namespace vst

using namespace vst;

extern "C" int vst_free_init_mix(const float* x, const float* init, const float* noise, float* out, const float* filt,
                                 float scale, const uint64_t* seed, const int* iter, int stream_id, int B, int Cl,
                                 int F, int H, int W, void* workspace, size_t ws_bytes, void* stream) {
  if (!x || !out || !filt || !workspace) return VST_ERR_ARG;
  if (noise ? (seed || iter) : (!seed || !iter)) return VST_ERR_ARG;  // r has exactly one source
  if (B <= 0 || Cl <= 0 || F <= 0 || H <= 0 || W <= 0) return VST_ERR_ARG;
  if (stream_id < 0 || stream_id >= (1 << 16) || Cl > (1 << 18)) return VST_ERR_ARG;
  if (F > kMixMaxN || H > kMixMaxN || W > kMixMaxN) return VST_ERR_UNSUPPORTED;
  const size_t planes = (size_t)B * Cl * F;
  if (planes > 0x7fffffffULL || (size_t)B * Cl > 65535) return VST_ERR_ARG;  // grid.x of 1 and 3, grid.y of 2
  const size_t n = planes * H * W, need = mix_spec_bytes(B, Cl, F, H, W);
  if (ws_bytes < need) return VST_ERR_ARG;
  if ((((uintptr_t)x | (uintptr_t)init | (uintptr_t)noise | (uintptr_t)out | (uintptr_t)filt) & 3) ||
      ((uintptr_t)workspace & 15) || ((uintptr_t)seed & 7) || ((uintptr_t)iter & 3))
    return VST_ERR_ARG;
  const MixSpan sx(x, n * 4), si(init, n * 4), sn(noise, n * 4), so(out, n * 4), sf(filt, (size_t)F * H * W * 4),
      sw(workspace, need), ss(seed, 8), st(iter, 4);
  if ((out != x && so.overlaps(sx)) || so.overlaps(si) || so.overlaps(sn) || so.overlaps(sf) || so.overlaps(ss) ||
      so.overlaps(st))
    return VST_ERR_ARG;
  if (sw.overlaps(sx) || sw.overlaps(si) || sw.overlaps(sn) || sw.overlaps(so) || sw.overlaps(sf) ||
      sw.overlaps(ss) || sw.overlaps(st))
    return VST_ERR_ARG;

  static const bool attr = mix_lds_attr(mix_plane_fwd_kernel) && mix_lds_attr(mix_frames_kernel) &&
                           mix_lds_attr(mix_plane_inv_kernel);
  if (!attr) return VST_ERR_LAUNCH;
  const int Wh = W / 2 + 1, Whp = Wh | 1, Wp = W | 1;
  const size_t lds1 = ((size_t)H * Whp + W + H) * sizeof(float2) + (size_t)H * Wp * sizeof(float);
  const size_t lds2 = ((size_t)2 * F * kMixPts + F) * sizeof(float2);
  const size_t lds3 = ((size_t)H * Wh + (size_t)H * Whp + W + H) * sizeof(float2);
  if (lds1 > (size_t)kMixMaxLds || lds2 > (size_t)kMixMaxLds || lds3 > (size_t)kMixMaxLds) return VST_ERR_UNSUPPORTED;

  const MixArgs a{x, init, noise, out, filt, scale, seed, iter, (uint32_t)stream_id, B, Cl, F, H, W,
                  (float2*)workspace};
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(mix_plane_fwd_kernel, dim3((unsigned)planes), dim3(kMixPlaneNT), lds1, s, a);
  hipLaunchKernelGGL(mix_frames_kernel, dim3((unsigned)((H * Wh + kMixPts - 1) / kMixPts), (unsigned)(B * Cl)),
                     dim3(kMixNT), lds2, s, a);
  hipLaunchKernelGGL(mix_plane_inv_kernel, dim3((unsigned)planes), dim3(kMixPlaneNT), lds3, s, a);
  return launch_status();
}
