// Regional prompts: masked multi-prompt cross-attention of the spatial attn2 layers (no line of the
// reference does this, the definition is this project's).
//
// Per query row m (image b = m / Nq), head h and region r < R
//   o_r = softmax(q_m K_r^T scale) V_r     one softmax per region over that region's Nk keys (sa_tile),
//   O[m] = bf16(sum over r ascending with w_r[m] != 0 of w_r[m] * (o_r_unnormalised * 1/l_r))     (sa_blend),
// with K_r / V_r the rows ((b / kv_div) R + r) Nk + key of Kt / Vt and w the caller's normalised fp32 [nimg Nq][4].
//
// The kernel is a shell over the shared head-dim-64 tile step, shaped as spatial_attn_kernel: a workgroup is 4 waves x
// 32 queries of one (image, head); a wave keeps Q^T, the running softmax state of the current region and a second
// fp32 accumulator for the blend in registers.  A region whose weight is zero on every row of the workgroup's 128-query
// block is dead there: none of its K/V is loaded.  The decision is taken once per workgroup from the weights of all of
// its rows (wave ballots met in LDS), so the cooperative K/V staging never diverges.  Two LDS plans, bit-identical:
//   PRE = 0  the (live region, tile) pairs are one walk, double-buffered through registers as in spatial_attn_kernel<0>:
//            tile 0 of region r + 1 is fetched under the last tile of region r.  32 KiB, any Nk.
//   PRE = n  (Nk <= 64 n, n <= 2) the K/V of every live region is brought in up front by LDS-DMA, one wait, one
//            barrier, as spatial_attn_kernel<PRE> does for one prompt.  R x n x 16 KiB: 128 KiB at R = 4, Nk = 77.
// vst_region_attention picks the plan by measurement (see there); a row's bits depend on its own q row, its weights and the K/V of its
// live regions only.
#include <limits.h>
#include <math.h>

#include <algorithm>

#include "attn_fwd.h"

namespace vst {

constexpr int kRegionMax = 4;

struct RegionArgs {
  const bf16_t* Q;
  const bf16_t* K;
  const bf16_t* V;
  const float* wts;
  bf16_t* O;
  int ldq, ldkv, ldo, nimg, heads, Nq, Nk, R, kv_div;
  float sl2;
  uint32_t q_bytes, kv_bytes;
};

// The whole K/V of PRE tiles (Nk <= 64 PRE keys from token row `row`) into the tile pairs at smem by LDS-DMA, as
// spatial_attn_kernel<PRE> issues it, every load of the workgroup in flight at once: tile t, operand (K, V), 8-row
// piece p; wave w issues p = w and p = w + 4 of every tile and operand.  The DMA writes each piece lane-linearly, so each lane fetches the global chunk that the
// tile's swizzle (k_off / v_off) puts at its LDS slot.  The caller waits (vmcnt) and synchronises.
template <int PRE>
__device__ __forceinline__ void sa_dma_kv(__amdgpu_buffer_rsrc_t rk, __amdgpu_buffer_rsrc_t rv, char* smem, int row,
                                          int Nk, int ldkv, int h, int wid, int lane) {
  const int prow = lane >> 3, pslot = lane & 7;
#pragma unroll
  for (int t = 0; t < PRE; ++t)
#pragma unroll
    for (int pp = 0; pp < 2; ++pp) {
      const int r = (wid + 4 * pp) * 8 + prow;
      const int key = t * SA_KT + r;
      const int ck = pslot ^ ((r >> 1) & 7), cv = pslot ^ (((r >> 1) & 3) << 1);
      const int base = (row + key) * ldkv + h * 64;
      char* dst = smem + t * 2 * SA_TILE + (wid + 4 * pp) * 1024;
      sa_dma16(rk, dst, key < Nk ? (base + ck * 8) * 2 : kOOB);
      sa_dma16(rv, dst + SA_TILE, key < Nk ? (base + cv * 8) * 2 : kOOB);
    }
}

// the lowest live region above r, or -1
__device__ __forceinline__ int region_next(int live, int r) {
  const int rest = (live >> (r + 1)) << (r + 1);  // r = -1: every region
  return rest ? __builtin_ctz(rest) : -1;
}

template <int PRE>
__global__ __launch_bounds__(256, 2) void region_attn_kernel(const RegionArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int live_s[4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, fr = lane & 15;
  const int nqb = (p.Nq + 127) / 128;
  const int wg = xcd_remap(blockIdx.x, nqb * p.heads * p.nimg);
  const int qblk = wg % nqb;
  const int bh = wg / nqb;
  const int h = bh % p.heads, b = bh / p.heads;
  const int Nk = p.Nk;
  const int kvrow0 = (b / p.kv_div) * p.R * Nk;

  const auto rq = make_rsrc(p.Q, p.q_bytes);
  const auto rk = make_rsrc(p.K, p.kv_bytes);
  const auto rv = make_rsrc(p.V, p.kv_bytes);

  bf16x8 qf[2][2];
  const int qbase = qblk * 128 + wid * 32;
  sa_load_q(qf, rq, b * p.Nq, qbase, p.Nq, p.ldq, h, lane);

  // this lane's weights: w[qb][r] of query qbase + 16 qb + fr; columns >= R and rows past Nq count as 0, unread or not
  f32x4 w[2];
  int mine = 0;
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const int q = qbase + qb * 16 + fr;
    w[qb] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (q < p.Nq) w[qb] = *reinterpret_cast<const f32x4*>(p.wts + ((size_t)b * p.Nq + q) * 4);
#pragma unroll
    for (int r = 0; r < kRegionMax; ++r) {
      if (r >= p.R) w[qb][r] = 0.0f;
      mine |= (w[qb][r] != 0.0f) << r;
    }
  }
  // live regions of the workgroup's query block: the same value in every thread, held in an SGPR
  int wave_live = 0;
#pragma unroll
  for (int r = 0; r < kRegionMax; ++r) wave_live |= (__ballot((mine >> r) & 1) != 0) << r;
  if (lane == 0) live_s[wid] = wave_live;
  __syncthreads();
  const int live = __builtin_amdgcn_readfirstlane(live_s[0] | live_s[1] | live_s[2] | live_s[3]);

  SaState st;
  f32x4 acc[4][2];
  sa_blend_init(acc);
  int voff[4];
  sa_voffs(voff, lane);
  const int nt = (Nk + SA_KT - 1) / SA_KT;
  auto weights = [&](int r, float(&wr)[2]) {  // (r is uniform: a register pick, no scratch)
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) wr[qb] = w[qb][r];
  };

  if constexpr (PRE == 0) {
    int r = region_next(live, -1), t = 0, cur = 0;
    if (r >= 0) {
      SaStage stg;
      stg.load(rk, rv, kvrow0 + r * Nk, 0, Nk, p.ldkv, h, tid);
      stg.store(smem, 0, tid);
      __syncthreads();
      sa_init(st);
      for (;;) {
        // the next step of the walk: the region's next tile, or tile 0 of the next live region
        const bool last = t + 1 == nt;
        const int rn = last ? region_next(live, r) : r, tn = last ? 0 : t + 1;
        if (rn >= 0) stg.load(rk, rv, kvrow0 + rn * Nk, tn, Nk, p.ldkv, h, tid);
        const char* Ks = smem + cur * 2 * SA_TILE;
        sa_tile(Ks, Ks + SA_TILE, qf, voff, p.sl2, st, lane, [&](f32x4(&s)[4][2]) {
          if ((t + 1) * SA_KT > Nk) sa_mask(s, t, Nk, lane);
        });
        if (rn >= 0) stg.store(smem, cur ^ 1, tid);
        __syncthreads();
        if (last) {
          float wr[2];
          weights(r, wr);
          sa_blend(st, acc, wr);
          sa_init(st);
        }
        if (rn < 0) break;
        r = rn, t = tn, cur ^= 1;
      }
    }
  } else {
    // slot j holds the j-th live region
    int j = 0;
    for (int r = region_next(live, -1); r >= 0; r = region_next(live, r), ++j)
      sa_dma_kv<PRE>(rk, rv, smem + j * PRE * 2 * SA_TILE, kvrow0 + r * Nk, Nk, p.ldkv, h, wid, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    j = 0;
    for (int r = region_next(live, -1); r >= 0; r = region_next(live, r), ++j) {
      sa_init(st);
      for (int t = 0; t < nt; ++t) {
        const char* Ks = smem + (j * PRE + t) * 2 * SA_TILE;
        sa_tile(Ks, Ks + SA_TILE, qf, voff, p.sl2, st, lane, [&](f32x4(&s)[4][2]) {
          if ((t + 1) * SA_KT > Nk) sa_mask(s, t, Nk, lane);
        });
      }
      float wr[2];
      weights(r, wr);
      sa_blend(st, acc, wr);
    }
  }

#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const int q = qbase + qb * 16 + fr;
    if (q >= p.Nq) continue;
    // a row without any weight is the empty sum: +0, not the accumulator's starting -0
    const bool any = (w[qb][0] != 0.0f) | (w[qb][1] != 0.0f) | (w[qb][2] != 0.0f) | (w[qb][3] != 0.0f);
    if (!any) {
#pragma unroll
      for (int db = 0; db < 4; ++db) acc[db][qb] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    sa_store_row(acc, qb, 1.0f, p.O + ((size_t)b * p.Nq + q) * p.ldo + h * 64, lane);
  }
}

}  // namespace vst

using namespace vst;

// -1: by the LDS the up-front plan needs (default); 0 / 1: that plan where it applies.  VST_REGION_PLAN, or
// vst_region_plan (tests, A/B)
static int g_region_plan = -2;
static int region_plan() {
  if (g_region_plan < -1) g_region_plan = std::max(-1, std::min(1, env_int("VST_REGION_PLAN", -1)));
  return g_region_plan;
}

extern "C" int vst_region_plan(int plan) {
  const int prev = region_plan();
  g_region_plan = std::max(-1, std::min(1, plan));
  return prev;
}

template <int PRE>
static int region_launch(const RegionArgs& a, size_t lds, unsigned grid, hipStream_t st) {
  static const bool attr = hipFuncSetAttribute((const void*)region_attn_kernel<PRE>,
                                               hipFuncAttributeMaxDynamicSharedMemorySize,
                                               PRE ? kRegionMax * PRE * 2 * SA_TILE : SA_LDS) == hipSuccess;
  if (!attr) return VST_ERR_LAUNCH;
  hipLaunchKernelGGL(region_attn_kernel<PRE>, dim3(grid), dim3(256), lds, st, a);
  return launch_status();
}

extern "C" int vst_region_attention(const void* q, int ldq, const void* Kt, const void* Vt, int ldkv, const float* wts,
                                    void* O, int ldo, int nimg, int heads, int Nq, int Nk, int R, int kv_div,
                                    float scale, void* stream) {
  if (!q || !Kt || !Vt || !wts || !O) return VST_ERR_ARG;
  if (nimg <= 0 || heads <= 0 || Nq <= 0 || Nk <= 0 || R <= 0 || kv_div <= 0) return VST_ERR_ARG;
  if (R > kRegionMax || nimg % kv_div) return VST_ERR_ARG;
  const long long inner = 64LL * heads;
  if (ldq < inner || ldkv < inner || ldo < inner || (ldq & 7) || (ldkv & 7) || (ldo & 7)) return VST_ERR_ARG;
  if (((uintptr_t)q | (uintptr_t)Kt | (uintptr_t)Vt | (uintptr_t)O | (uintptr_t)wts) & 15) return VST_ERR_ARG;
  Fit31 fit;
  RegionArgs a;
  const size_t rows = (size_t)nimg * Nq, kvrows = (size_t)(nimg / kv_div) * R * Nk;
  a.q_bytes = fit(((rows - 1) * ldq + inner) * sizeof(bf16_t));
  // Kt and Vt may be column views of one fused buffer; each rsrc is sized from its own base
  a.kv_bytes = fit(((kvrows - 1) * ldkv + inner) * sizeof(bf16_t));
  fit(((rows - 1) * ldo + inner) * sizeof(bf16_t));
  const long long grid = (long long)((Nq + 127) / 128) * heads * nimg;
  if (fit.over || grid > INT_MAX) return VST_ERR_ARG;  // past the kernel's 31-bit offsets: refuse, never read zeros
  a.Q = (const bf16_t*)q; a.K = (const bf16_t*)Kt; a.V = (const bf16_t*)Vt; a.wts = wts; a.O = (bf16_t*)O;
  a.ldq = ldq; a.ldkv = ldkv; a.ldo = ldo; a.nimg = nimg; a.heads = heads; a.Nq = Nq; a.Nk = Nk; a.R = R;
  a.kv_div = kv_div; a.sl2 = scale * kLog2e;
  hipStream_t st = (hipStream_t)stream;
  const int nt = (Nk + SA_KT - 1) / SA_KT;
  // measured (tools/region_attention_bench.py, Nk 77, one process, alternating; 32^2 / 16^2 level, us, walk -> up
  // front): R 1 36.7 -> 31.5 / 21.6 -> 18.3; R 2 soft maps 52.3 -> 50.8 / 29.2 -> 28.8, block-aligned 36.3 -> 36.4 /
  // 21.2 -> 21.3; R 4 soft 87.4 -> 123.5 / 46.8 -> 62.6, block-aligned 36.0 -> 55.1 / 28.5 -> 39.4 (128 KiB of LDS:
  // one workgroup per CU).  So the K/V comes up front while that leaves two workgroups per CU (64 KiB), else the walk.
  const int plan = region_plan();
  const bool fits = nt <= 2 && (size_t)R * nt * 2 * SA_TILE <= 2 * (size_t)SA_LDS;
  const int pre = nt <= 2 && (plan == 1 || (plan < 0 && fits)) ? nt : 0;
  const size_t lds = pre ? (size_t)R * pre * 2 * SA_TILE : SA_LDS;
  switch (pre) {
    case 1: return region_launch<1>(a, lds, (unsigned)grid, st);
    case 2: return region_launch<2>(a, lds, (unsigned)grid, st);
    default: return region_launch<0>(a, lds, (unsigned)grid, st);
  }
}
