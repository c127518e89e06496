// FreeU in the up path: the backbone scale and the skip's low-frequency filter of diffusers'
// apply_freeu (diffusers.utils.torch_utils), which the reference's up blocks call before every skip concatenation of
// their first two stages (animatediff/unet_block.py:399-417, unziplora_unet/unet_block.py:853-867).
//
// fourier_filter(x, threshold 1, scale s) scales the four frequency bins {-1, 0} x {-1, 0} of every (image, channel)
// map, so it is a rank-4 correction of the map and needs no FFT: with th = 2 pi h / H, ph = 2 pi w / W and
//   m0 = sum x, a = sum x cos th, b = sum x sin th, c = sum x cos ph, d = sum x sin ph,
//   e = sum x cos(th + ph), f = sum x sin(th + ph)
//   y[h, w] = x[h, w] + (s - 1) / (H W) (m0 + a cos th + b sin th + c cos ph + d sin ph
//                                        + e cos(th + ph) + f sin(th + ph)).
// One workgroup takes the H W rows of one image x one slab of CG * 8 channels (NHWC bf16, 16-byte loads of 8
// channels), keeps what it loaded in registers (the skip is read from memory once), reduces the seven sums per channel
// in an order fixed by the shape alone, and applies the correction from the registers.  The backbone scale
// (x_out[:, :Cx/2] = bf16(x * b)) runs in further workgroups of the same launch.
#include "vst_common.h"

namespace vst {

constexpr int kFreeuKeep = 8;      // 16-byte pieces a thread keeps between the reduce and the apply pass
constexpr int kFreeuMaxHW1 = 4096;  // H + W entries of the (cos, sin) table in the LDS

// the seven terms of one pixel: 1, (cos, sin) th, (cos, sin) ph, (cos, sin)(th + ph)
__device__ __forceinline__ void freeu_terms(const float2 th, const float2 ph, float* t) {
  t[0] = 1.0f;
  t[1] = th.x;
  t[2] = th.y;
  t[3] = ph.x;
  t[4] = ph.y;
  t[5] = th.x * ph.x - th.y * ph.y;  // cos(th + ph)
  t[6] = th.y * ph.x + th.x * ph.y;  // sin(th + ph)
}

// Sum over the lanes of a 16-lane row that share lane % CG, in every lane (DPP row rotations: no LDS traffic).
template <int CG>
__device__ __forceinline__ float row16_sum(float v) {
  static_assert(CG == 4 || CG == 8, "8 or 4 channel groups per slab");
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false));
  if (CG == 4)  // (the sum above has period 8 in the row, so lane i and lane i + 4 add the same two values)
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false));
  return v;
}

// 4 waves per SIMD (<= 128 VGPRs): every workgroup of the step's shapes is resident at once.
template <int NT, int CG, bool KEEP>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(4))) void freeu_kernel(
    const bf16_t* x, int ldx, int Cx, bf16_t* xo, int ldxo, int inplace, const bf16_t* __restrict__ sk, int lds, int Cs,
    bf16_t* __restrict__ so, int ldso, int nimg, int H, int W, const float* __restrict__ table, int stage, int nslab,
    int nfilter) {
  constexpr int RPI = NT / CG;  // rows of one pass over the slab
  constexpr int NW = NT / 64;
  const int tid = threadIdx.x;
  const float s = table[2 * stage], b = table[2 * stage + 1];
  const int HW = H * W;

  if ((int)blockIdx.x >= nfilter) {
    // backbone: 16-byte groups of the first Cx/2 channels scaled, the rest copied (not touched when x_out is x)
    const int half = Cx >> 4, gpr = inplace ? half : Cx >> 3;
    const uint32_t total = (uint32_t)nimg * HW * gpr;
    const uint32_t step = (gridDim.x - nfilter) * NT;
    for (uint32_t i = (blockIdx.x - nfilter) * NT + tid; i < total; i += step) {
      const uint32_t row = i / gpr;
      const int g = i - row * gpr;
      u32x4 v = *reinterpret_cast<const u32x4*>(x + (size_t)row * ldx + g * 8);
      if (g < half) {
        float f[8];
        unpack8(v, f);
#pragma unroll
        for (int c = 0; c < 8; ++c) f[c] *= b;
        v = pack8(f);
      }
      *reinterpret_cast<u32x4*>(xo + (size_t)row * ldxo + g * 8) = v;
    }
    return;
  }

  extern __shared__ float2 trig[];  // [H] (cos, sin)(2 pi h / H), then [W] (cos, sin)(2 pi w / W)
  __shared__ float part[NW * 4][CG * 56];  // per 16-lane row of every wave
  __shared__ float tot[CG * 56];
  for (int i = tid; i < H + W; i += NT) {
    const int n = i < H ? H : W, k = i < H ? i : i - H;
    double sn, cs;
    sincospi(2.0 * k / n, &sn, &cs);
    trig[i] = make_float2((float)cs, (float)sn);
  }
  __syncthreads();

  // consecutive slabs of an image on one XCD: the two 64-byte halves of a 128-byte line meet in one L2
  const int bid = xcd_remap(blockIdx.x, nfilter);
  const int img = bid / nslab, slab = bid - img * nslab;
  const int cg = tid % CG, rl = tid / CG;
  const int c0 = (slab * CG + cg) * 8;
  const bool col_ok = c0 < Cs;
  const bf16_t* src = sk + (size_t)img * HW * lds + c0;
  bf16_t* dst = so + (size_t)img * HW * ldso + c0;

  // KEEP: two passes of 4 channels over the kept rows (28 sums live beside the 32 kept registers); else one pass of 8
  constexpr int NC = KEEP ? 4 : 8, NP = 8 / NC;
  u32x4 keep[kFreeuKeep];
  int hw[kFreeuKeep];  // (h << 16) | w of the kept rows: one division per row, not one per use
  const int passes = KEEP ? kFreeuKeep : (HW + RPI - 1) / RPI;
  if (KEEP) {
#pragma unroll
    for (int k = 0; k < kFreeuKeep; ++k) {
      const int r = rl + k * RPI, h = r / W;
      hw[k] = (h << 16) | (r - h * W);
      if (col_ok && r < HW) keep[k] = *reinterpret_cast<const u32x4*>(src + (size_t)r * lds);
    }
  }
  // f: channels [p * NC, (p + 1) * NC) of the piece v; t: the seven terms of pixel (h, w)
  auto row_of = [&](const u32x4& v, int p, int h, int w, float* f, float* t) {
#pragma unroll
    for (int i = 0; i < NC / 2; ++i) {
      f[2 * i] = __uint_as_float(v[p * (NC / 2) + i] << 16);
      f[2 * i + 1] = __uint_as_float(v[p * (NC / 2) + i] & 0xffff0000u);
    }
    freeu_terms(trig[h], trig[H + w], t);
  };

  // sums: a thread's rows in pass order, the lanes of a 16-lane row that share cg (lane = rl * CG + cg) by row
  // rotations, then the NW * 4 rows of the workgroup in index order -- an order the shape alone fixes
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    float acc[7][NC];
#pragma unroll
    for (int j = 0; j < 7; ++j)
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[j][c] = 0.0f;
    auto reduce_row = [&](const u32x4& v, int h, int w) {
      float f[NC], t[7];
      row_of(v, p, h, w, f, t);
#pragma unroll
      for (int j = 0; j < 7; ++j)
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[j][c] = fmaf(f[c], t[j], acc[j][c]);
    };
    if (KEEP) {
#pragma unroll
      for (int k = 0; k < kFreeuKeep; ++k) {
        const int r = rl + k * RPI;
        if (col_ok && r < HW) reduce_row(keep[k], hw[k] >> 16, hw[k] & 0xffff);
      }
    } else {
      for (int k = 0; k < passes; ++k) {
        const int r = rl + k * RPI, h = r / W;
        if (col_ok && r < HW) reduce_row(*reinterpret_cast<const u32x4*>(src + (size_t)r * lds), h, r - h * W);
      }
    }
#pragma unroll
    for (int j = 0; j < 7; ++j)
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[j][c] = row16_sum<CG>(acc[j][c]);
    if ((tid & 15) < CG) {
#pragma unroll
      for (int j = 0; j < 7; ++j)
#pragma unroll
        for (int c = 0; c < NC; ++c) part[tid >> 4][(cg * 7 + j) * 8 + p * NC + c] = acc[j][c];
    }
  }
  __syncthreads();
  const float scale = (s - 1.0f) / (float)HW;
  for (int i = tid; i < CG * 56; i += NT) {
    float v = part[0][i];
#pragma unroll
    for (int w = 1; w < NW * 4; ++w) v += part[w][i];
    tot[i] = v * scale;
  }
  __syncthreads();
  if (!col_ok) return;

  const bool ident = s == 1.0f;  // the input's bits, -0 included
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    float acc[7][NC];
#pragma unroll
    for (int j = 0; j < 7; ++j)
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[j][c] = tot[(cg * 7 + j) * 8 + p * NC + c];
    // v's channels of pass p replaced by bf16(x + correction): one rounding, at the store
    auto apply_row = [&](u32x4& v, int h, int w) {
      float f[NC], t[7];
      row_of(v, p, h, w, f, t);
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        float corr = acc[0][c];
#pragma unroll
        for (int j = 1; j < 7; ++j) corr = fmaf(acc[j][c], t[j], corr);
        f[c] += corr;
      }
      if (!ident) {
#pragma unroll
        for (int i = 0; i < NC / 2; ++i) v[p * (NC / 2) + i] = pack2bf(f[2 * i], f[2 * i + 1]);
      }
    };
    if (KEEP) {
#pragma unroll
      for (int k = 0; k < kFreeuKeep; ++k) {
        const int r = rl + k * RPI;
        if (r < HW) apply_row(keep[k], hw[k] >> 16, hw[k] & 0xffff);
      }
    } else {
      for (int k = 0; k < passes; ++k) {
        const int r = rl + k * RPI, h = r / W;
        if (r < HW) {
          u32x4 v = *reinterpret_cast<const u32x4*>(src + (size_t)r * lds);  // second read: from L2
          apply_row(v, h, r - h * W);
          *reinterpret_cast<u32x4*>(dst + (size_t)r * ldso) = v;
        }
      }
    }
  }
  if (KEEP) {
#pragma unroll
    for (int k = 0; k < kFreeuKeep; ++k) {
      const int r = rl + k * RPI;
      if (r < HW) *reinterpret_cast<u32x4*>(dst + (size_t)r * ldso) = keep[k];
    }
  }
}

// Host side: [lo, hi) in bytes of a bf16 [rows, C] view with row stride ld.
struct ByteSpan {
  uintptr_t lo, hi;
  ByteSpan(const void* p, size_t rows, int C, int ld)
      : lo((uintptr_t)p), hi((uintptr_t)p + ((rows - 1) * (size_t)ld + C) * sizeof(bf16_t)) {}
  bool overlaps(const ByteSpan& o) const { return lo < o.hi && o.lo < hi; }
};

template <int NT, int CG, bool KEEP>
static int launch_freeu(const bf16_t* x, int ldx, int Cx, bf16_t* xo, int ldxo, int inplace, const bf16_t* sk, int lds,
                        int Cs, bf16_t* so, int ldso, int nimg, int H, int W, const float* table, int stage,
                        hipStream_t stream) {
  const int nslab = (Cs + CG * 8 - 1) / (CG * 8);
  const int nfilter = nimg * nslab;
  const size_t groups = (size_t)nimg * H * W * (inplace ? Cx / 16 : Cx / 8);
  const int nback = (int)std::min<size_t>((groups + NT * 4 - 1) / (NT * 4), 2048);
  hipLaunchKernelGGL((freeu_kernel<NT, CG, KEEP>), dim3(nfilter + nback), dim3(NT), (H + W) * sizeof(float2), stream,
                     x, ldx, Cx, xo, ldxo, inplace, sk, lds, Cs, so, ldso, nimg, H, W, table, stage, nslab, nfilter);
  return launch_status();
}

}  // namespace vst

using namespace vst;

extern "C" int vst_freeu(const void* x, int ldx, int Cx, const void* skip, int lds, int Cs, void* x_out, int ldxo,
                         void* skip_out, int ldso, int nimg, int H, int W, const float* table, int stage,
                         void* stream) {
  if (!x || !skip || !x_out || !skip_out || !table) return VST_ERR_ARG;
  if (nimg <= 0 || H < 2 || W < 2 || Cs <= 0 || Cs % 8 || Cx <= 0 || Cx % 16 || (stage != 0 && stage != 1))
    return VST_ERR_ARG;
  if (ldx < Cx || ldxo < Cx || lds < Cs || ldso < Cs || (ldx | ldxo | lds | ldso) % 8) return VST_ERR_ARG;
  if (((uintptr_t)x | (uintptr_t)skip | (uintptr_t)x_out | (uintptr_t)skip_out) & 15) return VST_ERR_ARG;
  if (H + W > kFreeuMaxHW1) return VST_ERR_UNSUPPORTED;
  const size_t rows = (size_t)nimg * H * W;
  if (rows * (size_t)(Cx / 8) > 0x7fffffffULL || rows > 0x7fffffffULL) return VST_ERR_ARG;
  const ByteSpan bx(x, rows, Cx, ldx), bs(skip, rows, Cs, lds), bxo(x_out, rows, Cx, ldxo),
      bso(skip_out, rows, Cs, ldso);
  const bool inplace = x_out == x && ldxo == ldx;  // the backbone scale may run in place, element for element
  if (bso.overlaps(bs) || bso.overlaps(bx) || bso.overlaps(bxo) || bxo.overlaps(bs) || (!inplace && bxo.overlaps(bx)))
    return VST_ERR_ARG;
  const bf16_t *xp = (const bf16_t*)x, *sp = (const bf16_t*)skip;
  bf16_t *xop = (bf16_t*)x_out, *sop = (bf16_t*)skip_out;
  hipStream_t st = (hipStream_t)stream;
  // the slab follows H W alone (never nimg): a map's sums, and so its bits, are those of the same map in any batch
  if (H * W <= 256)  // 16^2: 64 channels x 256 rows in 256 threads' registers
    return launch_freeu<256, 8, true>(xp, ldx, Cx, xop, ldxo, inplace, sp, lds, Cs, sop, ldso, nimg, H, W, table,
                                      stage, st);
  if (H * W <= 1024)  // 32^2: 32 channels x 1024 rows in 512 threads' registers
    return launch_freeu<512, 4, true>(xp, ldx, Cx, xop, ldxo, inplace, sp, lds, Cs, sop, ldso, nimg, H, W, table,
                                      stage, st);
  return launch_freeu<512, 4, false>(xp, ldx, Cx, xop, ldxo, inplace, sp, lds, Cs, sop, ldso, nimg, H, W, table, stage,
                                     st);
}
