// The GEMM front end: the small kernels beside the ring kernel (gemm_big.hip) and the 8-phase kernel (gemm_p8.hip),
// the policy that turns one call into one plan (plan_gemm, gemm_plan.h), and the C entry points (include/vst.h).
// Kernels here, each for a corner where a 256-wide MFMA tile has nothing to do:
//   conv_gather_kernel         3x3 conv whose channel count does not allow 16-byte loads (conv_in of UNet and VAE)
//   gemm_skinny_kernel         N <= 64 without an epilogue (the UnZipLoRA down-projection)
//   gemm_rows_kernel           M <= 8 (time-embedding MLPs)
//   gemm_splitk_reduce_kernel  sum of the ring kernel's split-K slabs + epilogue
// Operand layouts: gemm_common.h; epilogues and rounding points: gemm_epilogue.h.
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <set>
#include <string>

#include "gemm_plan.h"

namespace vst {

constexpr int BM = 128, BK = 64;  // (BK is also the alignment the host asks of an A source split)
constexpr int GBN = 64;           // the gather conv's tile: 128 x 64 x 64
constexpr int A_TILE = BM * BK * 2, B_TILE = GBN * BK * 2, STAGE = A_TILE + B_TILE;
constexpr int GATHER_LDS = 2 * STAGE;  // 48 KiB: two stages; the fp32 epilogue tile (32 KiB) reuses them
static_assert(GATHER_LDS >= BM * GBN * 4, "epilogue tile fits the stages");

// 3x3 conv (gemm_common.h conv A, one source) for channel counts that are no multiple of 8: each of a thread's
// 16-byte A chunks is gathered as 8 scalar loads, k = (tap, ci) padded to a multiple of 8 (the weight rows too).
// 256 threads = 4 waves (2 x 2), each wave 64 x 32 via v_mfma_f32_16x16x32_bf16; register-staged double-buffered LDS
// (load early, write late) in XOR-swizzled 128-byte rows; XCD-aware tile order; the fp32 tile goes through LDS to
// 16-byte stores with the ring kernel's rounding points (gemm_epilogue.h).
__global__ __launch_bounds__(256, 2) void conv_gather_kernel(GemmArgs p) {
  constexpr int NT = GBN / 32;   // 16-wide n tiles per wave
  constexpr int BCH = GBN / 32;  // B staging chunks per thread
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  const int nbn = (p.N + GBN - 1) / GBN, nbm = (p.M + BM - 1) / BM;
  const int wg = xcd_remap(blockIdx.x, nbn * nbm);
  const int bm = wg / nbn, bn = wg - bm * nbn;
  const int m0 = bm * BM, n0 = bn * GBN;

  const auto ra = make_rsrc(p.A1, p.a1_bytes);
  const auto rw = make_rsrc(p.Wt, p.w_bytes);

  const int sc = tid & 7, sr = tid >> 3;  // staging chunk / base row
  int img[4], oyv[4], oxv[4];             // per-staged-row A geometry (fixed over the K loop)
#pragma unroll
  for (int i = 0; i < 4; ++i) conv_row(p, m0 + sr + 32 * i, img[i], oyv[i], oxv[i]);
  int rowB[BCH];
#pragma unroll
  for (int i = 0; i < BCH; ++i) {
    const int n = n0 + sr + 32 * i;
    rowB[i] = n < p.N ? n : -1;
  }

  u32x4 va[4], vb[BCH];
  const int nk = (p.K + BK - 1) / BK;

  auto load_tile = [&](int kt) {
    const int k = kt * BK + sc * 8;
#pragma unroll
    for (int i = 0; i < BCH; ++i) {
      const int off = (rowB[i] >= 0 && k < p.K) ? (rowB[i] * p.ldw + k) * 2 : kOOB;
      vb[i] = buf_load16(rw, off);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      uint16_t e[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int kj = k + j;
        const int tap = kj / p.C1, ci = kj - tap * p.C1;
        const int ky = tap / 3, kx = tap - ky * 3;
        int px;  // (kj >= K1 = 9 C1: the K padding)
        const bool ok = conv_tap_pixel(p, img[i], oyv[i], oxv[i], ky, kx, px, kj < p.K1);
        e[j] = buf_load2(ra, ok ? (px * p.C1 + ci) * 2 : kOOB);
      }
      va[i] = u32x4{(uint32_t)e[0] | ((uint32_t)e[1] << 16), (uint32_t)e[2] | ((uint32_t)e[3] << 16),
                    (uint32_t)e[4] | ((uint32_t)e[5] << 16), (uint32_t)e[6] | ((uint32_t)e[7] << 16)};
    }
  };

  auto store_tile = [&](int buf) {
    char* As = smem + buf * STAGE;
    char* Bs = As + A_TILE;
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4*>(As + swz(sr + 32 * i, sc)) = va[i];
#pragma unroll
    for (int i = 0; i < BCH; ++i) *reinterpret_cast<u32x4*>(Bs + swz(sr + 32 * i, sc)) = vb[i];
  };

  f32x4 acc[4][NT];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fq = lane >> 4;
  if (nk > 0) {
    load_tile(0);
    store_tile(0);
  }
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) load_tile(kt + 1);
    const char* As = smem + cur * STAGE;
    const char* Bs = As + A_TILE;
    // skip the second 32-deep half when it lies wholly beyond K (Cin = 3 / 4: K = 32 / 40)
    const int nkk = (kt * BK + 32 < p.K) ? 2 : 1;
    for (int kk = 0; kk < nkk; ++kk) {
      bf16x8 af[4], bfr[NT];
      const int chunk = kk * 4 + fq;
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = *reinterpret_cast<const bf16x8*>(As + swz(wr * 64 + i * 16 + fr, chunk));
#pragma unroll
      for (int j = 0; j < NT; ++j)
        bfr[j] = *reinterpret_cast<const bf16x8*>(Bs + swz(wc * (GBN / 2) + j * 16 + fr, chunk));
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) store_tile(cur ^ 1);
    __syncthreads();
  }

  // ---------------- epilogue: fp32 tile through LDS ----------------
  float* Cs = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wr * 64 + i * 16 + fq * 4 + r;
        const int col = wc * (GBN / 2) + j * 16 + fr;
        Cs[row * GBN + col] = acc[i][j][r];
      }
  __syncthreads();

  constexpr int CPR = GBN / 8;  // 8-column chunks per tile row
  const auto rr = make_rsrc(p.R ? p.R : p.Wt, p.R ? p.r_bytes : 0u);
#pragma unroll 2
  for (int it = 0; it < BM * CPR / 256; ++it) {
    const int idx = tid + 256 * it;
    const int row = idx / CPR, cc = idx - row * CPR;
    const int m = m0 + row, n = n0 + cc * 8;
    if (m >= p.M || n >= p.N) continue;
    float v[8];
    const f32x4 c0 = *reinterpret_cast<const f32x4*>(Cs + row * GBN + cc * 8);
    const f32x4 c1 = *reinterpret_cast<const f32x4*>(Cs + row * GBN + cc * 8 + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[e] = c0[e]; v[e + 4] = c1[e]; }
    const int nv = min(8, p.N - n);
    if (p.bias) {
#pragma unroll
      for (int e = 0; e < 8; ++e) if (e < nv) v[e] += p.bias[n + e];
    }
    if (p.rbias || p.R) {  // same rounding points as the ring kernel: bf16 conv output, then the adds
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = round_bf(v[e]);
    }
    if (p.rbias) {
      const float* rb = p.rbias + (size_t)(m / p.rbias_div) * p.ldrb + n;
#pragma unroll
      for (int e = 0; e < 8; ++e) if (e < nv) v[e] += rb[e];
    }
    if (nv == 8) {
      if (p.R) {
        float r8[8];
        unpack8(buf_load16(rr, (m * p.ldr + n) * 2), r8);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += r8[e];
      }
      *reinterpret_cast<u32x4*>(p.C + (size_t)m * p.ldc + n) = pack8(v);
    } else {  // Cout < 8 (conv_out-like widths), or the last chunk of a Cout that is no multiple of 8
      for (int e = 0; e < nv; ++e) {
        float x = v[e];
        if (p.R) x += bf2f(p.R[(size_t)m * p.ldr + n + e]);
        p.C[(size_t)m * p.ldc + n + e] = f2bf(x);
      }
    }
  }
}

static int launch_gather(const GemmArgs& a, hipStream_t s) {
  const int nwg = ((a.M + BM - 1) / BM) * ((a.N + GBN - 1) / GBN);
  hipLaunchKernelGGL(conv_gather_kernel, dim3(nwg), dim3(256), GATHER_LDS, s, a);
  return launch_status();
}


// Skinny GEMM for the UnZipLoRA down-projection u = x . Acat^T (N = padded 2r per projection <= 64,
// no epilogue): HBM/MALL-bound on reading x once.  A workgroup = 8 waves owns 32 rows (two 16-row
// MFMA fragments) and all N columns; wave w takes the k32-steps w, w+8, ..., issuing a whole group
// of fragment-shaped loads before its MFMAs (lane l reads 16 B of row l&15 at k-chunk l>>4, which IS
// the 16x16x32 operand layout: no LDS staging).  Each W fragment feeds two row fragments, so the W
// bytes read per x byte are N/32 (the L2 traffic that bounded the 16-row version).  The 8 partial
// accumulators are summed through LDS (64 KiB at N = 64).  ceil(M/32) workgroups (256 at M = 8192), 2 per CU.
constexpr int kSkinnyMI = 2;  // 16-row fragments per workgroup

template <int NJ>
__global__ __launch_bounds__(512, 2) void gemm_skinny_kernel(GemmArgs p) {
  constexpr int MI = kSkinnyMI, NW = 8;
  constexpr int SK = NJ <= 2 ? 6 : 3;  // k32-steps per wave per load group (all in flight at once)
  __shared__ f32x4 red[NW][MI][NJ][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int m0 = blockIdx.x * 16 * MI;
  const auto ra = make_rsrc(p.A1, p.a1_bytes);
  const auto rw = make_rsrc(p.Wt, p.w_bytes);
  const int r = lane & 15, kc = (lane >> 4) * 8;
  uint32_t abase[MI];
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int arow = m0 + 16 * i + r;
    abase[i] = arow < p.M ? (uint32_t)(arow * p.lda1 + kc) * 2u : (uint32_t)kOOB;
  }
  uint32_t wbase[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j)
    wbase[j] = (16 * j + r) < p.N ? (uint32_t)((16 * j + r) * p.ldw + kc) * 2u : (uint32_t)kOOB;
  f32x4 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nk = (p.K + 31) / 32;
  for (int g = w; g < nk; g += NW * SK) {
    u32x4 a[SK][MI], b[SK][NJ];
#pragma unroll
    for (int t = 0; t < SK; ++t) {
      const int ks = g + NW * t;
      const bool kin = ks < nk && ks * 32 + kc < p.K;
#pragma unroll
      for (int i = 0; i < MI; ++i) a[t][i] = buf_load16(ra, kin ? (int)(abase[i] + ks * 64u) : kOOB);
#pragma unroll
      for (int j = 0; j < NJ; ++j) b[t][j] = buf_load16(rw, kin ? (int)(wbase[j] + ks * 64u) : kOOB);
    }
    // keep the whole group's loads in flight: one memory round trip per group, not one per k-step
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < SK; ++t)
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<bf16x8*>(&b[t][j]),
                                                              *reinterpret_cast<bf16x8*>(&a[t][i]), acc[i][j], 0, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) red[w][i][j][lane] = acc[i][j];
  __syncthreads();
  if (w >= MI) return;
  // wave i (< MI) sums row fragment i over the 8 waves and stores it
  const int i = w;
  f32x4 sum[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    sum[j] = red[0][i][j][lane];
#pragma unroll
    for (int q = 1; q < NW; ++q) sum[j] += red[q][i][j][lane];
  }
  // sum[j][e] = C[m0 + 16i + (lane&15)][16j + 4(lane>>4) + e]
  const int m = m0 + 16 * i + r;
  if (m >= p.M) return;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int n = 16 * j + 4 * (lane >> 4);
    if (n >= p.N) continue;
    bf16_t* dst = p.C + (size_t)m * p.ldc + n;
    if (n + 4 <= p.N) {
      u32x2 v;
      v[0] = pack2bf(sum[j][0], sum[j][1]);
      v[1] = pack2bf(sum[j][2], sum[j][3]);
      *reinterpret_cast<u32x2*>(dst) = v;
    } else {
      for (int e = 0; e < p.N - n; ++e) dst[e] = f2bf(sum[j][e]);
    }
  }
}

static int launch_skinny(const GemmArgs& a, hipStream_t s) {
  const dim3 grid((a.M + 16 * kSkinnyMI - 1) / (16 * kSkinnyMI));
  switch ((a.N + 15) / 16) {
    case 1: hipLaunchKernelGGL(gemm_skinny_kernel<1>, grid, dim3(512), 0, s, a); break;
    case 2: hipLaunchKernelGGL(gemm_skinny_kernel<2>, grid, dim3(512), 0, s, a); break;
    case 3: hipLaunchKernelGGL(gemm_skinny_kernel<3>, grid, dim3(512), 0, s, a); break;
    case 4: hipLaunchKernelGGL(gemm_skinny_kernel<4>, grid, dim3(512), 0, s, a); break;
    default: return VST_ERR_ARG;
  }
  return launch_status();
}

// Row-vector GEMM for M <= 8 (the time-embedding MLPs and the batched time_emb_proj of every ResnetBlock2D: M = the
// CFG pair, unet_motion.UNetMotionModel.embed / batched_temb; diffusers TimestepEmbedding, ResnetBlock2D).  These
// read N x K weights once to make 2 x N outputs: HBM-bound on W, nothing for MFMA to do.  The 128x128 split-K tiles
// they used to run on spent 46 us per launch on 2 live rows of 128 (0.4 TF/s, profiles/r3s9_kernel_stats.csv).
// A wave owns CPW output columns: lane l reads 16-B k-chunks l, l + 64, ... of each weight row (NT chunks per row in
// flight at once) and the same chunks of the M activation rows (L1/L2 hits: every wave reads the same x), sums in
// fp32, reduces across the wave, then the ring epilogue's rounding points: bias (+GELU) -> bf16 -> + row bias
// + residual -> bf16.  Each output's k order is fixed by (K, lane), so a column's value does not depend on N:
// the batched time_emb_proj equals the per-resnet Linear bit for bit.
template <int MR>
__global__ __launch_bounds__(256) void gemm_rows_kernel(GemmArgs p) {
  constexpr int CPW = 2, NT = MR <= 2 ? 4 : 2;
  const int lane = threadIdx.x & 63;
  const int nb = (blockIdx.x * 4 + (threadIdx.x >> 6)) * CPW;
  if (nb >= p.N) return;  // no barriers below
  const auto ra = make_rsrc(p.A1, p.a1_bytes);
  const auto rw = make_rsrc(p.Wt, p.w_bytes);
  float acc[MR][CPW];
#pragma unroll
  for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int c = 0; c < CPW; ++c) acc[m][c] = 0.f;
  const int nch = p.K >> 3;
  for (int q0 = 0; q0 < nch; q0 += 64 * NT) {
    u32x4 wv[NT][CPW], xv[NT][MR];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int q = q0 + t * 64 + lane;
      const bool in = q < nch;
#pragma unroll
      for (int c = 0; c < CPW; ++c)
        wv[t][c] = buf_load16(rw, in && nb + c < p.N ? ((nb + c) * p.ldw + q * 8) * 2 : kOOB);
#pragma unroll
      for (int m = 0; m < MR; ++m) xv[t][m] = buf_load16(ra, in && m < p.M ? (m * p.lda1 + q * 8) * 2 : kOOB);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int c = 0; c < CPW; ++c) {
        float w8[8];
        unpack8(wv[t][c], w8);
#pragma unroll
        for (int m = 0; m < MR; ++m) {
          float x8[8];
          unpack8(xv[t][m], x8);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[m][c] = fmaf(x8[e], w8[e], acc[m][c]);
        }
      }
  }
  float v = 0.f;
#pragma unroll
  for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int c = 0; c < CPW; ++c) {
      const float s = wave_sum(acc[m][c]);
      if (lane == m * CPW + c) v = s;
    }
  const int m = lane / CPW, n = nb + lane % CPW;
  if (lane >= MR * CPW || m >= p.M || n >= p.N) return;
  if (p.bias) v += p.bias[n];
  if (p.act) v = gelu_erf(v);
  if (p.rbias || p.R) {
    v = round_bf(v);
    if (p.rbias) v += p.rbias[(size_t)(m / p.rbias_div) * p.ldrb + n];
    if (p.R) v += bf2f(p.R[(size_t)m * p.ldr + n]);
  }
  p.C[(size_t)m * p.ldc + n] = f2bf(v);
}

static bool rows_applies(int M, int N, int K) { return M >= 1 && M <= 8 && N >= 1 && K >= 8 && !(K & 7); }

static int launch_rows(const GemmArgs& a, hipStream_t s) {
  const dim3 grid((a.N + 7) / 8);
  if (a.M <= 2) hipLaunchKernelGGL(gemm_rows_kernel<2>, grid, dim3(256), 0, s, a);
  else if (a.M <= 4) hipLaunchKernelGGL(gemm_rows_kernel<4>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(gemm_rows_kernel<8>, grid, dim3(256), 0, s, a);
  return launch_status();
}

// Sum the ring kernel's split-K slabs and apply the epilogue.  geglu: slab columns are the interleaved
// [h(32) | g(32)] blocks; each thread produces 8 output columns.
__global__ __launch_bounds__(256) void gemm_splitk_reduce_kernel(GemmArgs p, int geglu) {
  const int Nout = geglu ? p.N / 2 : p.N;
  const int CPR = (Nout + 7) / 8;
  const size_t total = (size_t)p.M * CPR;
  const size_t slab = (size_t)p.M * p.N;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int m = (int)(idx / CPR);
    const int n = (int)(idx - (size_t)m * CPR) * 8;
    const int nv = min(8, Nout - n);
    float v[8];
    if (!geglu) {
      const float* src = p.ws + (size_t)m * p.N + n;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = 0.f;
      for (int z = 0; z < p.splits; ++z) {
        const float* s = src + z * slab;
        if (nv == 8) {
          const f32x4 a = *reinterpret_cast<const f32x4*>(s), b = *reinterpret_cast<const f32x4*>(s + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) { v[e] += a[e]; v[e + 4] += b[e]; }
        } else {
          for (int e = 0; e < nv; ++e) v[e] += s[e];
        }
      }
      for (int e = 0; e < nv; ++e) {
        if (p.bias) v[e] += p.bias[n + e];
        if (p.rbias || p.R) v[e] = round_bf(v[e]);  // rounding points of the ring kernel's epilogue
        if (p.rbias) v[e] += p.rbias[(size_t)(m / p.rbias_div) * p.ldrb + n + e];
        if (p.R) v[e] += bf2f(p.R[(size_t)m * p.ldr + n + e]);
        if (p.act) v[e] = gelu_erf(v[e]);
      }
    } else {
      const int blk = n / 32, c = n - blk * 32;
      const int hc = blk * 64 + c, gc = hc + 32;
      float h[8], g[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) { h[e] = 0.f; g[e] = 0.f; }
      for (int z = 0; z < p.splits; ++z) {
        const float* s = p.ws + z * slab + (size_t)m * p.N;
#pragma unroll
        for (int e = 0; e < 8; ++e) { h[e] += s[hc + e]; g[e] += s[gc + e]; }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (p.bias) { h[e] += p.bias[hc + e]; g[e] += p.bias[gc + e]; }
        v[e] = round_bf(h[e]) * gelu_erf(round_bf(g[e]));
      }
    }
    bf16_t* dst = p.C + (size_t)m * p.ldc + n;
    if (nv == 8 && !((uintptr_t)dst & 15)) {
      *reinterpret_cast<u32x4*>(dst) = pack8(v);
    } else {
      for (int e = 0; e < nv; ++e) dst[e] = f2bf(v[e]);
    }
  }
}

// Weight fold of the folded upsample conv (gemm_common.h conv_row_folded): Wt [Cout][3][3][C] -> Wf [4][Cout][2][2][C],
//   Wf[2 py + px][co][a][b][ci] = sum of Wt[co][ky][kx][ci] over ky in S(py, a), kx in S(px, b),
//   S(0, 0) = {0}, S(0, 1) = {1, 2}, S(1, 0) = {0, 1}, S(1, 1) = {2},
// summed in fp32 in ascending (ky, kx) order and rounded once to bf16.  One thread per 8 channels of one output row.
__global__ __launch_bounds__(256) void fold_upsample_weight_kernel(const bf16_t* __restrict__ Wt, bf16_t* __restrict__ Wf,
                                                                   int Cout, int C) {
  const int C8 = C / 8;
  const size_t total = (size_t)16 * Cout * C8;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int c8 = (int)(idx % C8);
    const size_t t = idx / C8;  // (class, co, tap), the output's row order
    const int tap = (int)(t & 3), co = (int)((t >> 2) % Cout), cls = (int)((t >> 2) / Cout);
    const int py = cls >> 1, px = cls & 1, a = tap >> 1, b = tap & 1;
    const int ky0 = a == 0 ? 0 : (py == 0 ? 1 : 2), ky1 = a == 0 ? (py == 0 ? 0 : 1) : 2;
    const int kx0 = b == 0 ? 0 : (px == 0 ? 1 : 2), kx1 = b == 0 ? (px == 0 ? 0 : 1) : 2;
    float acc[8];
    bool first = true;
    for (int ky = ky0; ky <= ky1; ++ky)
      for (int kx = kx0; kx <= kx1; ++kx) {
        float w8[8];
        unpack8(*reinterpret_cast<const u32x4*>(Wt + ((size_t)co * 9 + ky * 3 + kx) * C + c8 * 8), w8);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = first ? w8[e] : acc[e] + w8[e];
        first = false;
      }
    *reinterpret_cast<u32x4*>(Wf + idx * 8) = pack8(acc);
  }
}

// ---------------- dispatch: one query -> one plan (gemm_plan.h) ----------------
// Everything the choice of a kernel depends on.  vst_gemm_ex and conv3x3_impl fill it from their arguments;
// vst_gemm_kernel_name, which sees sizes only, assumes one A source, a packed C inside the 32-bit offsets (a larger
// one is launched as row chunks), for convs C1 = K / 9 and C2 = 0, and for kind 0 no epilogue at all.
struct GemmQuery {
  int M, N, K, K1;
  bool two_src;       // A split along K into two sources (convs: channel concat)
  int epi;            // GemmPlan::epi
  bool no_epi;        // one source, no bias / row bias / residual / activation: all the skinny kernel can do
  int tile, splits;   // the caller's: public tile code 0-10 (0 auto), splits 0 auto / >= 1 forced
  size_t slab_bytes;  // usable split-K workspace
  size_t c_bytes;     // byte extent of C (M * ldc * 2)
  bool conv, vec;     // 3x3 conv; its channels allow 16-byte loads
  int C1, C2;
  bool fold;          // conv: the folded upsample conv (K = 4 C1, M = 4 padded class rows, one source, no split-K)
};

GemmKnobs& gemm_knobs() {
  static GemmKnobs k = {env_int("VST_GEMM_P8", -1),      env_int("VST_P8_BN", 0),        env_int("VST_P8_320", 0),
                        env_int("VST_P8_CONV", 1),       env_int("VST_P8_PERSIST", 1),   env_int("VST_P8_LORA_PERSIST", 1),
                        env_int("VST_LORA_INGEMM", 1),   env_int("VST_XATTN_FUSE", 1),   env_int("VST_GEMM_PERSIST", -1),
                        env_int("VST_GEMM_GROUP_M", 0),  env_int("VST_GEMM_ABLATE", 0)};
  return k;
}

constexpr int kCUs = 256;  // the CU count choose() and p8_auto were tuned against

int device_cus() {
  static int n = 0;
  if (n <= 0) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = kCUs;
  }
  return n;
}

// 256x160 ring tiles for Cout = 320 / 640 convs on full grids: Cout splits into 160-column tiles without the
// 256-wide tiles' padding (Cout = 320: 37.5 % of the MFMA work wasted, 640: 17 %).  Measured in the denoise step
// (tools/ab_bench.sh, profiles/r2_ab_t160.txt): convs 13.1 -> 12.4 ms per step.  The same tiles for N = 640 / 1280
// projections win in isolation (tools/tile_ab.py: 32768x640x672 50.1 -> 43.8 us) but lose in the step
// (74.0 -> 74.7 ms: operands arrive cold), so projections stay on the 8-phase kernel; Cout = 1280 convs gain
// nothing; GEGLU needs 64-column [h | g] blocks.
static bool t160_auto(int M, int N, bool geglu, bool conv) {
  if (geglu || N % 160) return false;
  const bool n_ok = conv && (N == 320 || N == 640);
  const int mb = (M + 255) / 256;
  return n_ok && mb * ((N + 255) / 256) >= kCUs / 2;
}

// Ring tile (when p.bm == 0: none forced) and split-K count of a ring plan.  splits: 0 auto, >= 1 forced.
static void choose(const GemmQuery& q, int splits, GemmPlan& p) {
  const int M = q.M, N = q.N, K = q.K;
  const bool geglu = q.epi == 1;
  const int nk = (K + BK - 1) / BK;
  const int t256 = ((M + 255) / 256) * ((N + 255) / 256);
  const int nk32 = (K + 31) / 32;  // ring kernel k-tiles
  auto set = [&p](int bm, int bn) { p.bm = bm, p.bn = bn; };
  // Tile policy (MI355X, measured in one process per comparison: tools/gemm_ablate.py TILES=..., bench.py):
  // the 256x256 ping-pong ring wins every projection / FF / GEGLU / conv shape of the path with at least a
  // quarter-wave of tiles, including the under-filled M = 8192, N = 1280 grids (160 tiles on 256 CUs:
  // 38 us vs 56 us for 192x256 at K = 1312, 116 vs 190 us at K = 5120; whole step 88.6 vs 92.9 ms);
  // tiny-M GEMMs (text states, temb) use 128x128 with split-K; conv_out (Cout = 4) 128x64.
  // Below half a wave of 256x256 tiles (the training step's 16x16 level: M = 4096, N = 1280 -> 80 tiles) the
  // 128x128 tile's 4x larger grid wins (tools/tile_ab.py: 4096x1280x1312 44.6 -> 30.7 us, x5120 112 -> 82 us).
  if (p.bm == 0) {
    if (q.conv && N <= 64) set(128, 64);
    else if (t160_auto(M, N, geglu, q.conv)) set(256, 160);
    // under-filled conv grids (the 16x16 level's Cout = 1280 convs: 160 tiles of 256x256): 192x256 tiles, 215 of
    // them, 4.12 -> 3.85 ms per step (profiles/r2_ab_conv_192x256.txt)
    else if (q.conv && t256 >= kCUs / 2 && t256 < kCUs) set(192, 256);
    else if (t256 >= kCUs / 2) set(256, 256);
    else set(128, 128);
  }
  if (geglu && (p.bn == 64 || p.bn == 160)) set(128, 128);
  const int tiles = ((M + p.bm - 1) / p.bm) * ((N + p.bn - 1) / p.bn);
  if (splits == 0) {
    splits = 1;
    if (tiles < kCUs / 2 && nk32 >= 8) {
      splits = std::min(std::min((2 * kCUs + tiles - 1) / tiles, nk32 / 4), 16);
      if (splits < 2) splits = 1;
    }
  }
  if (splits > nk32) splits = nk32;
  if (splits > 1) {
    const size_t need = (size_t)splits * M * N * sizeof(float);
    if (need > q.slab_bytes) splits = 1;
    if (splits > nk) splits = nk;
  }
  p.splits = splits;
}

// Automatic choice of the 8-phase kernel (tile 0).  Measured in the denoise step (tools/ab_bench.sh, VST_BENCH_SHAPES,
// one MI355X): it beats the ring on every projection / GEGLU shape -- first at K < 2048 (the 16x16-level
// out-projection 8192x1280x1312 9.53 -> 8.55 ms per step, GEGLU 8192x10240x1280 14.29 -> 13.93, the K = 320 shapes of
// the 64x64 level 3-7 %), and since its loop lost the per-piece K checks also at K >= 2048 (ff.net.2: ring 10.6 ->
// 9.1 ms per step, profiles/r2_ab_p8_all_k.txt).
// VST_GEMM_P8 = 0 off, unset / 1 every shape with at least half a wave of 256x256 tiles.
static bool p8_auto(int M, int N, int K) {
  if (gemm_knobs().p8 == 0) return false;
  const int t256 = ((M + 255) / 256) * ((N + 255) / 256);
  return t256 >= kCUs / 2 && K >= 128;
}

// 256x192 tiles for the 8-phase kernel (tile code 9, and tile 0 wherever it wins the round count): N = 1280 gives
// 7 column tiles (224 workgroups at M = 8192) instead of 5 (160 of 256 CUs), N = 640 two full rounds instead of
// 1.5, N = 320 a 192 + 128 split instead of 256 + 64.  A 256x192 tile costs ~0.8 of a 256x256 one (its fill and
// epilogue do not shrink with it), so it is taken when ceil(tiles192 / CUs) * 0.8 beats ceil(tiles256 / CUs).
// VST_P8_BN=256 keeps every shape on 256x256 (A/B).
// Forced 8-phase tile width (256 / 192 / 320, 0 = the policy below): VST_P8_BN, or vst_p8_force_bn (tests, A/B).
static bool p8_bn192(int M, int N, bool geglu) {
  const int env = gemm_knobs().p8_bn;
  if (geglu || env == 256 || env == 320) return false;
  const int mb = (M + 255) / 256, cus = device_cus();
  const int r256 = (mb * ((N + 255) / 256) + cus - 1) / cus, r192 = (mb * ((N + 191) / 192) + cus - 1) / cus;
  return env == 192 || 0.8 * r192 < 0.97 * r256;
}

// 128x320 tiles of the 8-phase kernel (tile code 10): every SDXL width (320 / 640 / 1280 / 1920 / 3840) splits into
// 320-column tiles without padding, and M = 8192 gives exactly one full round (256 tiles on 256 CUs) where 256x192
// gives 224.  A 128x320 tile is 0.625 of a 256x256 one in work.  VST_P8_320 = 1 takes it wherever its round count
// times 0.7 beats the 256 / 192 choice; VST_P8_BN = 320 wherever it is legal (A/B).
static bool p8_bn320(int M, int N, bool geglu) {
  const int env = gemm_knobs().p8_bn;
  if (geglu || N % 320) return false;
  if (env == 320) return true;
  if (!gemm_knobs().p8_320 || env == 256 || env == 192) return false;
  const int cus = device_cus();
  const int mb = (M + 255) / 256;
  const int r256 = (mb * ((N + 255) / 256) + cus - 1) / cus, r192 = (mb * ((N + 191) / 192) + cus - 1) / cus;
  const int r320 = (((M + 127) / 128) * (N / 320) + cus - 1) / cus;
  const double best = p8_bn192(M, N, false) ? 0.8 * r192 : r256;
  return 0.7 * r320 < 0.97 * best;
}

static int p8_bn(int M, int N, bool geglu) {
  return p8_bn320(M, N, geglu) ? 320 : p8_bn192(M, N, geglu) ? 192 : 256;
}

// Convs whose Cout is a multiple of 128 (not of 320) on which the 8-phase policy would take 192-wide tiles -- the VAE's
// Cout = 128 convs at 512^2 (a third of every 192-wide tile padding) and its Cout = 512 convs at 64^2 (256x128 tiles fill
// exactly one round of 256 CUs) -- run on the ring kernel's 256x128 tiles: same k order, same bits, 10-12 % faster
// per launch (tools/vae_conv_ab.py, profiles/r6_vae_conv_ab.txt).  No UNet conv qualifies (Cout 320 / 640 / 1280 / 4).
static bool conv_ring128(int M, int N) { return N % 128 == 0 && N % 320 != 0 && p8_bn(M, N, false) == 192; }

// the 8-phase kernel: dense A, no split-K, a 64-aligned A source split
static bool p8_applies(int K1, bool two_src) {
  return !two_src || (K1 & 63) == 0;
}

// Whether the 8-phase kernel runs on its persistent grid (gemm_p8.hip launch_p8_persist; VST_P8_PERSIST=0: never):
// at least two tiles per workgroup, K a multiple of 64 and >= 128 (the stream hands over two whole k-tiles), whole
// 8-column output chunks, one A source, and a C the epilogue's buffer descriptor can address.
static bool p8_persist_applies(int M, int N, int K, int epi, int bn, bool two_src = false, size_t c_bytes = 0) {
  if (!gemm_knobs().p8_persist || (epi != 0 && epi != 1 && epi != 3) || two_src || c_bytes >= 0x7fff0000u) return false;
  const int bm = bn == 320 ? 128 : 256;
  const long tiles = (long)((M + bm - 1) / bm) * ((N + bn - 1) / bn);
  return tiles >= 2L * p8_cus() && K >= 128 && (K & 63) == 0 && (N % (epi == 1 ? 16 : 8)) == 0;
}

// The in-GEMM LoRA kernels on the persistent grid (128x320 tiles only: a pass of the staged epilogue must hold whole
// row quadrants of the rotated LoRA accumulators), wherever p8_persist_applies: the 32x32 level's q/k/v 123 -> 108 us
// and out-projection 48 -> 43 us per launch, bitwise equal (profiles/r5_ab_lora_persist.txt).  VST_P8_LORA_PERSIST=0
// restores one workgroup per tile (A/B).
static bool p8_lora_persist_on() { return gemm_knobs().p8_persist && gemm_knobs().p8_lora_persist; }

// Stream-K (one workgroup per CU over equal shares of the (tile, k-step) space, partial tiles summed by their
// owner) was built for both the ring and the 8-phase kernel in rounds 1-3 and measured slower on every shape of this
// path (8192x1280x1312: 8.56 -> 11.1 ms per step).  Its cross-workgroup hand-off also depended on
// every workgroup being resident at once, which concurrent streams do not guarantee, so it was removed.

// The one place a kernel is chosen.  family == kNone: the request is not legal.
static GemmPlan plan_gemm(const GemmQuery& q) {
  // public tile codes (include/vst.h); 0 = the policy below
  static const GemmPlan codes[11] = {{kNone},          {kRing, 128, 128}, {kRing, 128, 64},  {kRing, 256, 256},
                                     {kRing, 256, 128}, {kSkinny},         {kRing, 256, 160}, {kRing, 192, 256},
                                     {kP8, 256, 256},   {kP8, 256, 192},   {kP8, 128, 320}};
  if (q.tile < 0 || q.tile > 10 || q.splits < 0) return {};
  const int M = q.M, N = q.N, K = q.K;
  const bool any = q.tile == 0, geglu = q.epi == 1;
  GemmPlan p = codes[q.tile];
  p.epi = q.epi, p.splits = 1, p.conv = q.conv;
  // splits 1 = no split-K (a row's bits then never depend on M: the denoise forward's row-invariant policy); the
  // 8-phase kernel, which never splits, is chosen the same way under 0 and 1
  const bool p8_ok = any && q.splits <= 1 && q.epi != 2 && p8_auto(M, N, K);
  auto p8_tile = [&p](int family, int bn) { p.family = family, p.bm = bn == 320 ? 128 : 256, p.bn = bn; };
  if (q.conv) {
    if (p.family == kP8 || p.family == kSkinny) return {};  // convs take the ring's tile codes only
    if (q.fold && (!q.vec || q.C2 || q.splits != 1 || q.epi != 0)) return {};
    p.fold = q.fold;
    if (!q.vec) {
      p.family = kGather, p.bm = BM, p.bn = 64;  // (conv_in): register-staged kernel, no split
    } else {
      // 3x3 convs with both sources a multiple of 64 channels run on the 8-phase kernel (implicit im2col; 128x320
      // tiles where Cout is a multiple of 320, else the projection policy's width); VST_P8_CONV=0 restores the ring
      const bool p8 = p8_ok && gemm_knobs().p8_conv && !(q.C1 & 63) && !(q.C2 & 63) && !(N & 63) &&
                      K == (q.fold ? 4 : 9) * (q.C1 + q.C2);
      const bool ring128 = p8 && conv_ring128(M, N);
      if (ring128) p.bm = 256, p.bn = 128;
      if (p8 && !ring128) p8_tile(kP8Conv, N % 320 == 0 ? 320 : p8_bn(M, N, false));
      else p.family = kRing, choose(q, ring128 ? 1 : q.splits, p);
      // folded rows: a tile must divide the class padding (kFoldRowAlign), which the 192-row ring tile does not
      if (q.fold && p.family == kRing && p.bm == 192) p.bm = 256;
    }
    return p;
  }
  if (p.family == kP8 && (!p8_applies(q.K1, q.two_src) || (geglu && p.bn != 256) || (p.bn == 320 && N % 320))) return {};
  if (p.family == kSkinny && !(q.no_epi && N <= 64)) return {};
  if (any) {
    if (!q.two_src && (q.epi == 0 || q.epi == 3) && rows_applies(M, N, K)) p.family = kRows;
    else if (q.no_epi && N <= 64 && M >= 1024) p.family = kSkinny;  // LoRA down-projection
    else if (p8_ok && p8_applies(q.K1, q.two_src)) p8_tile(kP8, p8_bn(M, N, geglu));
  }
  if (p.family == kP8) p.persist = p8_persist_applies(M, N, K, q.epi, p.bn, q.two_src, q.c_bytes);
  if (p.family == kNone || p.family == kRing) p.family = kRing, choose(q, q.splits, p);
  return p;
}

// The plan as the name bench.py and tools/pmc_traffic.py group launches by:
// <family><BMxBN[,geglu][,splitk|,persist|,conv|,upfold]>, "" for no plan
static const char* plan_name(const GemmPlan& p) {
  static const char* const fixed[] = {"", "gemm_rows", "gemm_skinny", "gemm_kernel<conv_in>"};
  if (p.family <= kGather) return fixed[p.family];
  const bool split = p.splits > 1;
  char buf[64];
  snprintf(buf, sizeof buf, "%s<%dx%d%s%s>", p.family == kRing ? "gemm_ring" : "gemm_p8", p.bm, p.bn,
           p.epi == 1 && !split ? ",geglu" : "", split ? ",splitk" : p.persist ? ",persist" : p.fold ? ",upfold" : p.conv ? ",conv" : "");
  static std::mutex mu;
  static std::set<std::string> names;  // (the returned pointer stays valid: set nodes do not move)
  std::lock_guard<std::mutex> lock(mu);
  return names.insert(buf).first->c_str();
}

static int launch_plan(GemmArgs& a, const GemmPlan& p, hipStream_t s) {
  const GemmKnobs& k = gemm_knobs();
  a.ablate = p.family == kP8Conv ? 0 : k.ablate;
  a.group_m = k.group_m;
  // Ring kernel's persistent launch: measured (tools/gemm_persist.sh) 4-10 % faster for the GEGLU epilogue and neutral
  // for the others, so it is the default for GEGLU only.  VST_GEMM_PERSIST=1 forces it on, =0 off.
  a.persist = (k.ring_persist > 0 || (k.ring_persist < 0 && p.epi == 1)) ? device_cus() : 0;
  a.splits = p.splits;
  switch (p.family) {
    case kRows: return launch_rows(a, s);
    case kSkinny: return launch_skinny(a, s);
    case kGather: return launch_gather(a, s);
    case kP8: return launch_gemm_p8(a, p, s);
    case kP8Conv: return p.fold ? launch_gemm_p8_conv_folded(a, p, s) : launch_gemm_p8_conv(a, p, s);
    case kRing: break;
    default: return VST_ERR_ARG;
  }
  const int rc = launch_gemm_ring(a, p, s);
  if (rc || p.splits <= 1) return rc;
  const int Nout = p.epi == 1 ? a.N / 2 : a.N;
  const size_t chunks = (size_t)a.M * ((Nout + 7) / 8);
  const int grid = (int)std::min<size_t>((chunks + 255) / 256, 4096);
  hipLaunchKernelGGL(gemm_splitk_reduce_kernel, dim3(grid), dim3(256), 0, s, a, p.epi == 1 ? 1 : 0);
  return launch_status();
}

}  // namespace vst

using namespace vst;

// Force the 8-phase kernel's tile width for every later GEMM of this process (256 / 192 / 320 where legal; 0 = the
// automatic policy); returns the previous setting.  For tests and A/B runs.
extern "C" int vst_p8_force_bn(int bn) {
  const int prev = gemm_knobs().p8_bn;
  gemm_knobs().p8_bn = (bn == 256 || bn == 192 || bn == 320) ? bn : 0;
  return prev;
}

// Route 3x3 convs with 64-multiple channel sources to the 8-phase kernel (1) or the ring kernel (0) for every later
// conv of this process; returns the previous setting.  For tests and A/B runs.
extern "C" int vst_p8_conv(int on) {
  const int prev = gemm_knobs().p8_conv ? 1 : 0;
  gemm_knobs().p8_conv = on ? 1 : 0;
  return prev;
}

// The 8-phase kernel's persistent grid (1) or one workgroup per tile (0) for every later GEMM of this process; returns
// the previous setting.  For tests and A/B runs.
extern "C" int vst_p8_persist(int on) {
  const int prev = gemm_knobs().p8_persist ? 1 : 0;
  gemm_knobs().p8_persist = on ? 1 : 0;
  return prev;
}

// Workspace (caller-owned): the fp32 split-K slabs [splits][M][N] of a ring launch of this shape.
extern "C" size_t vst_gemm_workspace_bytes(int M, int N, int K) {
  GemmQuery q{};
  q.M = M, q.N = N, q.K = q.K1 = K, q.epi = 2, q.slab_bytes = (size_t)-1;
  const int splits = plan_gemm(q).splits;
  return splits > 1 ? (size_t)splits * M * N * sizeof(float) : 0;
}

// ---------------- entry points ----------------
constexpr size_t kMaxExtent = 0x7fffffffULL;  // the largest byte extent a buffer descriptor's 32-bit offsets reach

// GemmArgs of a dense call: A [M][K1] (row stride lda; vst_gemm_ex adds the second source), W [N][K], bias, C, the
// operands' extents through fit, one split, stride 1.  Everything else is zero.
static GemmArgs dense_args(Fit31& fit, const void* A, int lda, int K1, const void* W, int ldw, int M, int N, int K,
                           const float* bias, void* C, int ldc) {
  GemmArgs a{};
  a.A1 = (const bf16_t*)A; a.lda1 = lda; a.K1 = K1;
  a.Wt = (const bf16_t*)W; a.ldw = ldw; a.M = M; a.N = N; a.K = K;
  a.bias = bias; a.C = (bf16_t*)C; a.ldc = ldc;
  a.a1_bytes = fit(((size_t)(M - 1) * lda + K1) * 2);
  a.w_bytes = fit(((size_t)(N - 1) * ldw + K) * 2);
  a.stride = 1; a.splits = 1;
  return a;
}

// The in-GEMM LoRA block (GemmArgs::la ...) and the row gate on u, on top of dense_args
static void lora_args(GemmArgs& a, Fit31& fit, const void* Acat, int ld_acat, int P, int group_n, int group_r,
                      bool gated, const float* gate, int ld_gate, int gate_div) {
  a.wtail_bytes = fit(((size_t)(a.N - 1) * a.ldw + a.K + P) * 2);
  a.la = (const bf16_t*)Acat; a.lda_la = ld_acat; a.la_p = P; a.la_gn = group_n; a.la_gr = group_r;
  a.la_bytes = fit((size_t)P * ld_acat * 2);
  if (gated) { a.gate = gate; a.ld_gate = ld_gate; a.gate_div = gate_div; }
}

// ---- fused base + LoRA projection with the down-projection inside the 8-phase GEMM (gemm_p8.hip LORA) ----
// VST_LORA_INGEMM=0 turns it off (the host then runs the separate down-projection pass, A/B).
// 0 = not supported (the host falls back to u = x.Acat^T + vst_gemm_ex), else the 8-phase tile width (256 / 192 /
// 320).  Every tile's output columns must need u columns inside one 16-aligned block of 16.  Whether the in-GEMM
// path is taken depends on the SHAPE only (N, K, the projection groups), never on M: it runs whenever some tile width
// keeps every tile inside one u block (the policy's width first, then 192, 256, 320 -- every SDXL width is a multiple
// of 320, so the 32x32 q/k/v, which straddles q/k on 256-wide tiles, runs on 128x320 tiles).  So a frame-sharded rank
// (fewer rows) takes the same path as the unsharded forward, and the two agree bit for bit: the tile width itself
// does not change any output bit (same k order).
static bool lora_tiles_ok(int N, int P, int gn, int gr, int bn) {
  for (int n0 = 0; n0 < N; n0 += bn) {
    const int g0 = n0 / gn, g1 = (std::min(n0 + bn, N) - 1) / gn;
    const int lo = (g0 * gr) & ~15, hi = (g1 + 1) * gr;
    if (hi > lo + 16 || lo + 16 > P) return false;
  }
  return true;
}

static int lora_ingemm_bn(int M, int N, int K, int P, int gn, int gr, int force_bn = 0) {
  if (!gemm_knobs().lora_ingemm || M <= 0 || N <= 0 || K < 128 || (K & 7) || P <= 0 || (P & 15) || P > 256 || gn <= 0 ||
      gr <= 0 || N % gn || (N / gn) * gr > P)
    return 0;
  if (force_bn) return lora_tiles_ok(N, P, gn, gr, force_bn) && (force_bn != 320 || N % 320 == 0) ? force_bn : 0;
  const int cand[4] = {p8_bn(M, N, false), 192, 256, 320};
  int bn = 0;
  for (int c : cand)
    if ((c != 320 || N % 320 == 0) && lora_tiles_ok(N, P, gn, gr, c)) {
      bn = c;
      break;
    }
  // a multi-round grid of 256-row tiles (the 32x32 out-projection) moves to the persistent LoRA grid, which runs
  // 128x320 tiles only (p8_lora_persist_on); a grid under two rounds keeps its tiles (the 16x16 q/k/v:
  // 480 tiles of 256x256, 76 us against 89 on 128x320 persistent, profiles/r5_ab_lora_persist.txt)
  if (bn && bn != 320 && p8_lora_persist_on() && N % 320 == 0 && lora_tiles_ok(N, P, gn, gr, 320) &&
      (long)((M + 255) / 256) * ((N + bn - 1) / bn) >= 2L * device_cus() && p8_persist_applies(M, N, K, 0, 320))
    bn = 320;
  return bn;
}

extern "C" int vst_gemm_lora_supported(int M, int N, int K, int P, int group_n, int group_r) {
  return lora_ingemm_bn(M, N, K, P, group_n, group_r);
}

// The row gate of the _gated entries (GemmArgs::gate): checked before any launch; the same for both entries
static bool lora_gate_args_ok(const float* gate, int ld_gate, int gate_div, int P) {
  return gate && gate_div > 0 && ld_gate >= P && !(ld_gate & 3) && !((uintptr_t)gate & 15);
}

// vst_gemm_lora (gated = false, gate NULL) and vst_gemm_lora_gated: one implementation, the same tile either way
static int gemm_lora_impl(const void* x, int ldx, const void* Acat, int ld_acat, int P, int group_n, int group_r,
                          const void* W, int ldw, int M, int N, int K, const float* bias, const void* R, int ldr,
                          void* C, int ldc, bool gated, const float* gate, int ld_gate, int gate_div, void* stream) {
  Fit31 fit;
  if (!x || !Acat || !W || !C || M <= 0 || N <= 0 || K <= 0) return VST_ERR_ARG;
  if (gated && !lora_gate_args_ok(gate, ld_gate, gate_div, P)) return VST_ERR_ARG;
  if ((ldx & 7) || (ld_acat & 7) || (ldw & 7) || (ldc & 7) || ldx < K || ld_acat < K || ldw < K + P) return VST_ERR_ARG;
  if (R && ((ldr & 7) || ldr < N)) return VST_ERR_ARG;
  const int bn = lora_ingemm_bn(M, N, K, P, group_n, group_r);
  if (!bn) return VST_ERR_UNSUPPORTED;
  GemmArgs a = dense_args(fit, x, ldx, K, W, ldw, M, N, K, bias, C, ldc);
  a.R = (const bf16_t*)R; a.ldr = ldr;
  a.r_bytes = R ? fit(((size_t)(M - 1) * ldr + N) * 2) : 0;
  lora_args(a, fit, Acat, ld_acat, P, group_n, group_r, gated, gate, ld_gate, gate_div);
  if (fit.over) return VST_ERR_ARG;  // past the 32-bit buffer offsets (not chunked here): refuse
  a.ablate = gemm_knobs().ablate;  // (reaches the kernel in the diagnostics build only, -DVST_P8_TRACE)
  a.group_m = gemm_knobs().group_m;
  const bool persist = bn == 320 && p8_lora_persist_on() && p8_persist_applies(M, N, K, 0, bn, false, (size_t)M * ldc * 2);
  return launch_gemm_p8_lora(a, bn, persist, (hipStream_t)stream);
}

extern "C" int vst_gemm_lora(const void* x, int ldx, const void* Acat, int ld_acat, int P, int group_n, int group_r,
                             const void* W, int ldw, int M, int N, int K, const float* bias, const void* R, int ldr,
                             void* C, int ldc, void* stream) {
  return gemm_lora_impl(x, ldx, Acat, ld_acat, P, group_n, group_r, W, ldw, M, N, K, bias, R, ldr, C, ldc, false,
                        nullptr, 0, 1, stream);
}

extern "C" int vst_gemm_lora_gated(const void* x, int ldx, const void* Acat, int ld_acat, int P, int group_n,
                                   int group_r, const void* W, int ldw, int M, int N, int K, const float* bias,
                                   const void* R, int ldr, void* C, int ldc, const float* gate, int ld_gate,
                                   int gate_div, void* stream) {
  return gemm_lora_impl(x, ldx, Acat, ld_acat, P, group_n, group_r, W, ldw, M, N, K, bias, R, ldr, C, ldc, true, gate,
                        ld_gate, gate_div, stream);
}

// ---- attn2: q projection (+ in-GEMM LoRA) with the cross-attention over the text tokens as its epilogue ----
// VST_XATTN_FUSE=0 turns it off (the host then runs the q GEMM and vst_spatial_attention, A/B).
// Shape-only decision (not M: a frame-sharded rank fuses exactly where the unsharded forward does).
static bool xattn_ok(int M, int N, int K, const void* Acat, int P, int gn, int gr, int Nq, int Nk) {
  if (!gemm_knobs().xattn_fuse || M <= 0 || N <= 0 || N % 64 || K < 128 || (K & 7) || Nq <= 0 || Nq % 256 || M % Nq || Nk < 1 ||
      Nk > 80)
    return false;
  return !Acat || lora_ingemm_bn(M, N, K, P, gn, gr, 192) == 192;
}

extern "C" int vst_gemm_cross_attention_supported(int M, int N, int K, int lora, int P, int group_n, int group_r,
                                                  int Nq, int Nk) {
  return xattn_ok(M, N, K, lora ? (const void*)1 : nullptr, P, group_n, group_r, Nq, Nk) ? 1 : 0;
}

static int gemm_cross_attention_impl(const void* x, int ldx, const void* Acat, int ld_acat, int P, int group_n,
                                     int group_r, const void* W, int ldw, const float* bias, int M, int N, int K,
                                     const void* Kt, const void* Vt, int ldkv, int nkv_rows, int Nq, int Nk,
                                     int kv_div, float scale, void* O, int ldo, bool gated, const float* gate,
                                     int ld_gate, int gate_div, void* stream) {
  Fit31 fit;
  if (!x || !W || !Kt || !Vt || !O || M <= 0 || N <= 0 || K <= 0 || kv_div <= 0 || nkv_rows <= 0) return VST_ERR_ARG;
  if (gated && (!Acat || !lora_gate_args_ok(gate, ld_gate, gate_div, P))) return VST_ERR_ARG;  // (the gate scales u)
  if ((ldx & 7) || (ldw & 7) || (ldo & 7) || (ldkv & 7) || ldx < K || ldo < N || ldkv < N) return VST_ERR_ARG;
  if (Acat && ((ld_acat & 7) || ld_acat < K || ldw < K + P)) return VST_ERR_ARG;
  if (!Acat && ldw < K) return VST_ERR_ARG;
  if (!xattn_ok(M, N, K, Acat, P, group_n, group_r, Nq, Nk)) return VST_ERR_UNSUPPORTED;
  if ((M / Nq - 1) / kv_div >= nkv_rows / Nk) return VST_ERR_ARG;  // every frame's text batch inside K/V
  GemmArgs a = dense_args(fit, x, ldx, K, W, ldw, M, N, K, bias, O, ldo);
  if (Acat) lora_args(a, fit, Acat, ld_acat, P, group_n, group_r, gated, gate, ld_gate, gate_div);
  a.xa_k = (const bf16_t*)Kt; a.xa_v = (const bf16_t*)Vt; a.xa_ldkv = ldkv; a.xa_nk = Nk; a.xa_nq = Nq;
  a.xa_kvdiv = kv_div; a.xa_scale_log2 = scale * kLog2e;
  a.xa_kv_bytes = fit(((size_t)(nkv_rows - 1) * ldkv + N) * 2);
  if (fit.over) return VST_ERR_ARG;  // past the 32-bit buffer offsets (not chunked here): refuse
  a.ablate = gemm_knobs().ablate;  // (diagnostics build only)
  return launch_gemm_p8_xattn(a, (hipStream_t)stream);
}

extern "C" int vst_gemm_cross_attention(const void* x, int ldx, const void* Acat, int ld_acat, int P, int group_n,
                                        int group_r, const void* W, int ldw, const float* bias, int M, int N, int K,
                                        const void* Kt, const void* Vt, int ldkv, int nkv_rows, int Nq, int Nk,
                                        int kv_div, float scale, void* O, int ldo, void* stream) {
  return gemm_cross_attention_impl(x, ldx, Acat, ld_acat, P, group_n, group_r, W, ldw, bias, M, N, K, Kt, Vt, ldkv,
                                   nkv_rows, Nq, Nk, kv_div, scale, O, ldo, false, nullptr, 0, 1, stream);
}

extern "C" int vst_gemm_cross_attention_gated(const void* x, int ldx, const void* Acat, int ld_acat, int P,
                                              int group_n, int group_r, const void* W, int ldw, const float* bias,
                                              int M, int N, int K, const void* Kt, const void* Vt, int ldkv,
                                              int nkv_rows, int Nq, int Nk, int kv_div, float scale, void* O, int ldo,
                                              const float* gate, int ld_gate, int gate_div, void* stream) {
  return gemm_cross_attention_impl(x, ldx, Acat, ld_acat, P, group_n, group_r, W, ldw, bias, M, N, K, Kt, Vt, ldkv,
                                   nkv_rows, Nq, Nk, kv_div, scale, O, ldo, true, gate, ld_gate, gate_div, stream);
}

// The motion modules' q/k/v projection + frame-axis attention in one launch (EPI 5 of the 8-phase kernel): 16 frames
// per clip, heads of 40 (two per 256-column tile: an even head count) or 80 (one per tile), pixels per frame a
// multiple of 16.
static int tattn_hpt(int head_dim) { return head_dim == 40 ? 2 : head_dim == 80 ? 1 : 0; }
static bool tattn_ok(int M, int K, int nclip, int F, int HW, int heads, int head_dim) {
  const int hpt = tattn_hpt(head_dim);
  if (!hpt || F != 16 || heads <= 0 || heads % hpt || HW <= 0 || (HW & 15) || nclip <= 0) return false;
  // (shape-only, like the other fused paths: a frame-sharded rank decides as the unsharded forward does)
  return (long)M == (long)nclip * F * HW && !(K & 63) && K >= 128 && gemm_knobs().p8 != 0;
}

extern "C" int vst_gemm_temporal_attention_supported(int M, int K, int nclip, int F, int HW, int heads,
                                                     int head_dim) {
  return tattn_ok(M, K, nclip, F, HW, heads, head_dim) ? 1 : 0;
}

extern "C" int vst_gemm_temporal_attention(const void* x, int ldx, const void* Wt, int ldw, const float* bias, int M,
                                           int K, int nclip, int F, int HW, int heads, int head_dim, float scale,
                                           void* O, int ldo, void* stream) {
  Fit31 fit;
  if (!x || !Wt || !O || M <= 0 || K <= 0) return VST_ERR_ARG;
  if ((ldx & 7) || (ldw & 7) || (ldo & 7) || ldx < K || ldw < K || ldo < heads * head_dim) return VST_ERR_ARG;
  if (!tattn_ok(M, K, nclip, F, HW, heads, head_dim)) return VST_ERR_UNSUPPORTED;
  const int N = heads / tattn_hpt(head_dim) * 256;
  GemmArgs a = dense_args(fit, x, ldx, K, Wt, ldw, M, N, K, bias, O, ldo);
  if (fit.over) return VST_ERR_ARG;  // past the 32-bit buffer offsets (not chunked here): refuse
  a.ta_hw = HW; a.ta_heads = heads; a.ta_d = head_dim; a.ta_scale_log2 = scale * kLog2e;
  return launch_gemm_p8_tattn(a, (hipStream_t)stream);
}

// Name of the kernel a vst_gemm_ex / vst_conv3x3_ex call with these arguments launches (the
// symbol rocprofv3 reports), so per-launch timings can be attributed to kernels.  kind: 0 linear,
// 1 GEGLU linear, 2 vectorized conv, 3 scalar-gather conv, 4 folded upsample conv (M = its GEMM rows, four padded
// classes; K = 4 C; tile and splits are not the caller's there).  Returns a static string.
extern "C" const char* vst_gemm_kernel_name(int M, int N, int K, int kind, int tile, int splits, size_t ws_bytes) {
  if (kind < 0 || kind > 4) return "";
  GemmQuery q{};
  q.M = M, q.N = N, q.K = q.K1 = K, q.epi = kind == 1, q.no_epi = kind == 0, q.tile = tile, q.splits = splits;
  q.slab_bytes = ws_bytes, q.conv = kind >= 2, q.vec = kind == 2 || kind == 4, q.C1 = K / 9;
  if (kind == 4) q.fold = true, q.C1 = K / 4, q.tile = 0, q.splits = 1;
  return plan_name(plan_gemm(q));
}

// The kernels address A, A2 and the residual through buffer descriptors with 32-bit byte offsets (Fit31): an
// operand whose byte extent passes 2^31 - 1 would read zeros past that point.  Such a call (e.g. the motion modules'
// ff.net.2 at the 64^2 level of an 8-clip CFG batch, A = 1M x 1280 bf16 = 2.7 GB) runs as equal row chunks with
// offset pointers instead.  The kernels' per-row k order does not depend on M, and chunks this large take the same
// kernels (no split-K), so every row gets the bits of one launch (test_kernels_gpu.py::test_gemm_rows_past_2gb).
static size_t row_extent(size_t rows, int ld, int cols) { return ((rows - 1) * (size_t)ld + (size_t)cols) * 2; }
static int row_chunk(int M, size_t row_bytes, int align) {  // balanced rows per chunk (a multiple of align), 0: none
  const size_t fit = (kMaxExtent / row_bytes) / (size_t)align * (size_t)align;
  if (fit == 0) return 0;
  const size_t n = ((size_t)M + fit - 1) / fit;
  const size_t rows = (((size_t)M + n - 1) / n + align - 1) / align * align;
  return rows <= fit ? (int)rows : (int)fit;
}
static int gcd_int(int a, int b) { return b ? gcd_int(b, a % b) : a; }

extern "C" int vst_gemm_ex(const void* A, int lda, const void* A2, int lda2, int K1, const void* W, int ldw, int M,
                           int N, int K, const float* bias, const float* row_bias, int row_bias_div, int ld_row_bias,
                           const void* R, int ldr, void* C, int ldc, int epilogue, int tile, int splits,
                           void* workspace, size_t ws_bytes, void* stream) {
  Fit31 fit;
  if (!A || !W || !C || M <= 0 || N <= 0 || K <= 0) return VST_ERR_ARG;
  if ((K & 7) || (lda & 7) || (ldw & 7) || (ldc & 7)) return VST_ERR_ARG;
  if (A2) {
    if (K1 <= 0 || K1 % BK || K1 >= K || (lda2 & 7)) return VST_ERR_ARG;
  } else {
    K1 = K;
  }
  if (epilogue < 0 || epilogue > 2) return VST_ERR_ARG;
  if (epilogue == 1 && (N % 64)) return VST_ERR_ARG;
  if (epilogue == 2 && (R || row_bias)) return VST_ERR_ARG;  // GELU: bias only
  if (R && (ldr & 7)) return VST_ERR_ARG;
  if (row_bias && row_bias_div <= 0) return VST_ERR_ARG;
  {
    const int nout = epilogue == 1 ? N / 2 : N;
    const size_t lim = kMaxExtent;
    if (row_extent(M, lda, K1) > lim || (A2 && row_extent(M, lda2, K - K1) > lim) ||
        (R && row_extent(M, ldr, nout) > lim) || row_extent(M, ldc, nout) > lim) {
      const int wide = max(max(lda, A2 ? lda2 : 0), max(R ? ldr : 0, ldc));
      const int align = row_bias ? 256 / gcd_int(256, row_bias_div) * row_bias_div : 256;
      const int rows = align > 0 ? row_chunk(M, (size_t)wide * 2, align) : 0;
      if (rows <= 0) return VST_ERR_ARG;
      const int ldrb = ld_row_bias ? ld_row_bias : N;
      for (int m0 = 0; m0 < M; m0 += rows) {
        const int mc = min(rows, M - m0);
        const int st = vst_gemm_ex(
            (const char*)A + (size_t)m0 * lda * 2, lda, A2 ? (const char*)A2 + (size_t)m0 * lda2 * 2 : nullptr, lda2,
            A2 ? K1 : 0, W, ldw, mc, N, K, bias, row_bias ? row_bias + (size_t)(m0 / row_bias_div) * ldrb : nullptr,
            row_bias_div, ld_row_bias, R ? (const char*)R + (size_t)m0 * ldr * 2 : nullptr, ldr,
            (char*)C + (size_t)m0 * ldc * 2, ldc, epilogue, tile, splits, workspace, ws_bytes, stream);
        if (st != VST_OK) return st;
      }
      return VST_OK;
    }
  }
  GemmQuery q{};
  q.M = M, q.N = N, q.K = K, q.K1 = K1, q.two_src = A2 != nullptr, q.epi = epilogue == 2 ? 3 : epilogue;
  q.no_epi = !A2 && !bias && !row_bias && !R && epilogue == 0;
  q.tile = tile, q.splits = splits, q.slab_bytes = workspace ? ws_bytes : 0, q.c_bytes = (size_t)M * ldc * 2;
  const GemmPlan plan = plan_gemm(q);
  if (plan.family == kNone) return VST_ERR_ARG;
  GemmArgs a = dense_args(fit, A, lda, K1, W, ldw, M, N, K, bias, C, ldc);
  a.A2 = (const bf16_t*)A2; a.lda2 = lda2;
  a.a2_bytes = A2 ? fit(((size_t)(M - 1) * lda2 + (K - K1)) * 2) : 0;
  a.rbias = row_bias; a.rbias_div = row_bias_div; a.ldrb = ld_row_bias;
  a.R = (const bf16_t*)R; a.ldr = ldr;
  a.r_bytes = R ? fit(((size_t)(M - 1) * ldr + N) * 2) : 0;
  a.ws = (float*)workspace;
  if (fit.over) return VST_ERR_ARG;  // (A / R / C are chunked above; a weight past 2^31 - 1 bytes is refused)
  a.act = epilogue == 2 ? 1 : 0;
  return launch_plan(a, plan, (hipStream_t)stream);
}

extern "C" int vst_gemm(const void* A, int lda, const void* A2, int lda2, int K1, const void* W, int ldw, int M, int N,
                        int K, const float* bias, const float* row_bias, int row_bias_div, int ld_row_bias,
                        const void* R, int ldr, void* C, int ldc, int epilogue, void* stream) {
  return vst_gemm_ex(A, lda, A2, lda2, K1, W, ldw, M, N, K, bias, row_bias, row_bias_div, ld_row_bias, R, ldr, C, ldc,
                     epilogue, 0, 1, nullptr, 0, stream);
}

// 3x3 conv, padding 1, NHWC.  x1: [nimg,H,W,C1], optional x2: [nimg,H,W,C2] concatenated
// on channels.  Wt: [Cout][3][3][C1+C2].  stride 1 or 2; upsample=1 applies nearest 2x to
// the input first (output 2H x 2W).  Output [nimg, OH, OW, Cout] with row stride ldc.

static int conv3x3_impl(const void* x1, int C1, const void* x2, int C2, int nimg, int H, int W, int stride,
                        int upsample, int pad0, const void* Wt, int Cout, const float* bias, const float* row_bias,
                        int row_bias_div, int ld_row_bias, const void* R, int ldr, void* out, int ldc, int tile,
                        int splits, void* workspace, size_t ws_bytes, void* stream) {
  Fit31 fit;
  if (!x1 || !Wt || !out || nimg <= 0 || H <= 0 || W <= 0 || Cout <= 0) return VST_ERR_ARG;
  if (pad0 && (stride != 2 || H < 2 || W < 2)) return VST_ERR_ARG;
  if (stride != 1 && stride != 2) return VST_ERR_ARG;
  if (upsample && stride != 1) return VST_ERR_ARG;
  const int Ct = C1 + (x2 ? C2 : 0);
  const bool vec = (Ct % BK == 0) && (C1 % 8 == 0);
  if (x2 && !vec) return VST_ERR_ARG;
  GemmArgs a{};
  a.OH = upsample ? 2 * H : pad0 ? (H - 2) / 2 + 1 : (stride == 2 ? (H + 1) / 2 : H);
  a.OW = upsample ? 2 * W : pad0 ? (W - 2) / 2 + 1 : (stride == 2 ? (W + 1) / 2 : W);
  {  // byte extents past the 32-bit buffer offsets (vst_gemm_ex): chunks of whole images (a 3x3 tap never leaves its
     // image), equal in size
    const size_t lim = kMaxExtent, hw = (size_t)H * W, ohw = (size_t)a.OH * a.OW;
    const size_t img_bytes = max(max(hw * C1, x2 ? hw * C2 : 0), max(R ? ohw * ldr : 0, ohw * ldc)) * 2;
    if ((size_t)nimg * img_bytes > lim) {
      if (row_bias && row_bias_div != (int)ohw) return VST_ERR_UNSUPPORTED;
      const int per = (int)(lim / img_bytes);
      if (per <= 0) return VST_ERR_ARG;
      const int nch = (nimg + per - 1) / per, ipc = (nimg + nch - 1) / nch;
      const int ldrb = ld_row_bias ? ld_row_bias : Cout;
      for (int i0 = 0; i0 < nimg; i0 += ipc) {
        const int ni = min(ipc, nimg - i0);
        const int st = conv3x3_impl(
            (const char*)x1 + (size_t)i0 * hw * C1 * 2, C1, x2 ? (const char*)x2 + (size_t)i0 * hw * C2 * 2 : nullptr,
            C2, ni, H, W, stride, upsample, pad0, Wt, Cout, bias, row_bias ? row_bias + (size_t)i0 * ldrb : nullptr,
            row_bias_div, ld_row_bias, R ? (const char*)R + (size_t)i0 * ohw * ldr * 2 : nullptr, ldr,
            (char*)out + (size_t)i0 * ohw * ldc * 2, ldc, tile, splits, workspace, ws_bytes, stream);
        if (st != VST_OK) return st;
      }
      return VST_OK;
    }
  }
  a.pad0 = pad0;
  a.A1 = (const bf16_t*)x1; a.A2 = (const bf16_t*)x2; a.C1 = C1; a.C2 = x2 ? C2 : 0;
  a.H = H; a.W = W; a.stride = stride; a.up = upsample;
  a.K = 9 * Ct; a.K1 = a.K;
  a.M = nimg * a.OH * a.OW; a.N = Cout;
  if (!vec) a.K = (a.K + 7) & ~7;  // scalar gather: pad K to a chunk; weight rows padded too
  a.Wt = (const bf16_t*)Wt; a.ldw = a.K;
  if (row_bias && (row_bias_div <= 0 || (ld_row_bias && ld_row_bias < Cout) || ((ld_row_bias ? ld_row_bias : Cout) & 3)))
    return VST_ERR_ARG;
  a.bias = bias; a.rbias = row_bias; a.rbias_div = row_bias_div; a.ldrb = ld_row_bias ? ld_row_bias : Cout;
  a.R = (const bf16_t*)R; a.ldr = ldr; a.C = (bf16_t*)out; a.ldc = ldc;
  a.ws = (float*)workspace;
  a.a1_bytes = fit((size_t)nimg * H * W * C1 * 2);
  a.a2_bytes = x2 ? fit((size_t)nimg * H * W * C2 * 2) : 0;
  a.w_bytes = fit((size_t)Cout * a.K * 2);
  a.r_bytes = R ? fit(((size_t)(a.M - 1) * ldr + Cout) * 2) : 0;
  if (fit.over) return VST_ERR_ARG;  // (A / R / C are chunked above; a weight past 2^31 - 1 bytes is refused)
  if ((ldc & 7) && Cout >= 8) return VST_ERR_ARG;
  GemmQuery q{};
  q.M = a.M, q.N = a.N, q.K = a.K, q.K1 = a.K1, q.two_src = x2 != nullptr, q.tile = tile, q.splits = splits;
  q.slab_bytes = workspace ? ws_bytes : 0, q.c_bytes = (size_t)a.M * ldc * 2;
  q.conv = true, q.vec = vec, q.C1 = a.C1, q.C2 = a.C2;
  const GemmPlan plan = plan_gemm(q);
  if (plan.family == kNone) return VST_ERR_ARG;
  return launch_plan(a, plan, (hipStream_t)stream);
}

extern "C" int vst_conv3x3_ex(const void* x1, int C1, const void* x2, int C2, int nimg, int H, int W, int stride,
                              int upsample, const void* Wt, int Cout, const float* bias, const float* row_bias,
                              int row_bias_div, int ld_row_bias, const void* R, int ldr, void* out, int ldc, int tile,
                              int splits, void* workspace, size_t ws_bytes, void* stream) {
  return conv3x3_impl(x1, C1, x2, C2, nimg, H, W, stride, upsample, 0, Wt, Cout, bias, row_bias, row_bias_div,
                      ld_row_bias, R, ldr, out, ldc, tile, splits, workspace, ws_bytes, stream);
}

// ---- the nearest-2x upsample conv as four 2x2 convs on folded weights (gemm_common.h conv_row_folded) ----
extern "C" int vst_fold_upsample_weight(const void* Wt, int Cout, int C, void* Wf, void* stream) {
  if (!Wt || !Wf || Cout <= 0 || C <= 0) return VST_ERR_ARG;
  if (C & 7) return VST_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(fold_upsample_weight_kernel, dim3(grid_for((size_t)16 * Cout * (C / 8))), dim3(256), 0,
                     (hipStream_t)stream, (const bf16_t*)Wt, (bf16_t*)Wf, Cout, C);
  return launch_status();
}

extern "C" int vst_conv3x3_up_folded(const void* x1, int ldx, int C1, const void* x2, int C2, int nimg, int H, int W,
                                     const void* Wf, int ldwf, int Cout, const float* bias, const float* row_bias,
                                     const void* R, void* out, int ldc, void* stream) {
  Fit31 fit;
  if (!x1 || !Wf || !out || nimg <= 0 || H <= 0 || W <= 0 || Cout <= 0 || C1 <= 0) return VST_ERR_ARG;
  if (x2 || C2 || row_bias || R || (C1 & 63) || (Cout & 7)) return VST_ERR_UNSUPPORTED;
  if ((ldx & 7) || ldx < C1 || (ldwf & 7) || ldwf < 4 * C1 || (ldc & 7) || ldc < Cout) return VST_ERR_ARG;
  const size_t hw = (size_t)H * W;
  {  // byte extents past the 32-bit buffer offsets: chunks of whole images, as conv3x3_impl (a row's k order, and so its
     // bits, do not depend on nimg)
    const size_t img_bytes = max(hw * ldx, 4 * hw * ldc) * 2;
    if ((size_t)nimg * img_bytes > kMaxExtent) {
      const int per = (int)(kMaxExtent / img_bytes);
      if (per <= 0) return VST_ERR_ARG;
      const int nch = (nimg + per - 1) / per, ipc = (nimg + nch - 1) / nch;
      for (int i0 = 0; i0 < nimg; i0 += ipc) {
        const int st = vst_conv3x3_up_folded((const char*)x1 + (size_t)i0 * hw * ldx * 2, ldx, C1, nullptr, 0,
                                             min(ipc, nimg - i0), H, W, Wf, ldwf, Cout, bias, nullptr, nullptr,
                                             (char*)out + (size_t)i0 * 4 * hw * ldc * 2, ldc, stream);
        if (st != VST_OK) return st;
      }
      return VST_OK;
    }
  }
  GemmArgs a{};
  a.A1 = (const bf16_t*)x1; a.lda1 = ldx; a.C1 = C1;
  a.H = H; a.W = W; a.OH = 2 * H; a.OW = 2 * W; a.stride = 1; a.up = 2;
  a.up_live = nimg * H * W;
  a.up_rows = (a.up_live + kFoldRowAlign - 1) / kFoldRowAlign * kFoldRowAlign;
  a.K = a.K1 = 4 * C1;
  a.M = 4 * a.up_rows; a.N = Cout;
  a.Wt = (const bf16_t*)Wf; a.ldw = ldwf;
  a.bias = bias; a.C = (bf16_t*)out; a.ldc = ldc;
  a.a1_bytes = fit(((size_t)(a.up_live - 1) * ldx + C1) * 2);
  a.w_bytes = fit(((size_t)(4 * Cout - 1) * ldwf + a.K) * 2);
  if (fit.over) return VST_ERR_ARG;  // (x / out are chunked above; a weight past 2^31 - 1 bytes is refused)
  GemmQuery q{};
  q.M = a.M, q.N = a.N, q.K = q.K1 = a.K, q.splits = 1, q.c_bytes = (size_t)4 * a.up_live * ldc * 2;
  q.conv = q.vec = q.fold = true, q.C1 = C1;
  const GemmPlan plan = plan_gemm(q);
  if (plan.family == kNone) return VST_ERR_ARG;
  return launch_plan(a, plan, (hipStream_t)stream);
}

// 3x3 stride-2 conv with padding (0,1,0,1): diffusers Downsample2D(padding=0) = F.pad(x, (0, 1, 0, 1)) + conv(k3, s2,
// p0), the downsampler of the SDXL VAE encoder's DownEncoderBlock2D.  Output [nimg, (H-2)/2+1, (W-2)/2+1, Cout].
extern "C" int vst_conv3x3_down_pad0(const void* x, int C, int nimg, int H, int W, const void* Wt, int Cout,
                                     const float* bias, void* out, int ldc, void* workspace, size_t ws_bytes,
                                     void* stream) {
  return conv3x3_impl(x, C, nullptr, 0, nimg, H, W, 2, 0, 1, Wt, Cout, bias, nullptr, 1, 0, nullptr, 0, out, ldc, 0,
                      0, workspace, ws_bytes, stream);
}

// C[M][N] (fp32, row stride N) = A[M][K] . W[N][K]^T with no rounding of the accumulator: the ring kernel's split-K slab
// epilogue with one split.  For attention scores whose softmax must see fp32 logits (the SDXL VAE mid-block attention,
// head_dim 512, fp32 in the reference: inference_animatediff.py:164-169).
extern "C" int vst_gemm_f32out(const void* A, int lda, const void* W, int ldw, int M, int N, int K, float* C,
                               void* stream) {
  Fit31 fit;
  if (!A || !W || !C || M <= 0 || N <= 0 || K <= 0) return VST_ERR_ARG;
  if ((K & 7) || (lda & 7) || (ldw & 7) || (N & 3)) return VST_ERR_ARG;
  GemmArgs a = dense_args(fit, A, lda, K, W, ldw, M, N, K, nullptr, nullptr, N);
  a.ws = C;  // (no bf16 output: the fp32 slab is the result)
  if (fit.over) return VST_ERR_ARG;  // past the 32-bit buffer offsets (not chunked here): refuse
  GemmQuery q{};
  q.M = M, q.N = N, q.K = q.K1 = K, q.epi = 2, q.splits = 1;  // the slab epilogue: a ring tile, one split
  return launch_plan(a, plan_gemm(q), (hipStream_t)stream);
}

extern "C" int vst_conv3x3(const void* x1, int C1, const void* x2, int C2, int nimg, int H, int W, int stride,
                           int upsample, const void* Wt, int Cout, const float* bias, const float* row_bias,
                           int row_bias_div, const void* R, int ldr, void* out, int ldc, void* stream) {
  return vst_conv3x3_ex(x1, C1, x2, C2, nimg, H, W, stride, upsample, Wt, Cout, bias, row_bias, row_bias_div, 0, R,
                        ldr, out, ldc, 0, 1, nullptr, 0, stream);
}
