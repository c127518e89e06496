// The backward cores that the attention kernels of the training path share (attention.hip), beside the forward ones
// (attn_fwd.h).  As there, the kernels are shells: each does its own index math, chooses what streams through LDS and
// what stays in registers, masks by its own rule and runs its own loop; every step that rounds is one piece here or in
// attn_fwd.h, so a change to the formula or to a fragment convention is made once.
//
// 1) Spatial, head_dim 64 (sa_bwd_dq_kernel, sa_bwd_dkv_kernel).  A wave keeps 32 token rows as B fragments in registers
//    (sa_load_rows: Q / dO in dQ, K / V in dK/dV) and streams 64-row tiles of the other side through LDS (SbStage).
//    Who owns which rounding step:
//      S, dP (bf16 MFMA, fp32 accumulation from zero, k-steps 0 then 1)      sb_scores
//      P = exp2(S sl2 - lse2), dS = P (dP - D) in fp32                      sb_prob, attn_ds
//      P / dS to bf16 B fragments, two 16-row tiles per 32-deep k-step      sa_pack2 (attn_fwd.h; sa_tile's too)
//      acc += T^T . fragment, over the tiles in loop order                  sb_accum (tr_frag)
//      acc (x scale) to bf16 rows                                           sa_store_row (attn_fwd.h; sa_finish's too)
//    The dQ kernel's D = dO . O reduction stays in that kernel.
//
// 2) Frame axis (temporal_attn_bwd_kernel).  The query-column statistics come from the forward's ta_softmax (mask, max,
//    exp2, sum; it also hands back the exp2-domain max), the three B operands from ta_pack_p and the K^T / Q^T / dO^T A
//    fragments from ta_vt_frag; dS = P (dP - D) is attn_ds.  The key-column tiles, which take the statistics by
//    __shfl, stay in the kernel.
#pragma once
#include "attn_fwd.h"

namespace vst {

constexpr int SB_TILE = SA_TILE;  // one 64-row x 64-d bf16 tile, 8 KiB

// P recomputed from the forward's log2-domain logsumexp
__device__ __forceinline__ float sb_prob(float s, float sl2, float lse2) { return fast_exp2(s * sl2 - lse2); }
// dS = P (dP - D)
__device__ __forceinline__ float attn_ds(float p, float dp, float D) { return p * (dp - D); }

// Register staging of one 64-row tile of two operands (rows sr, sr + 32; 16-B chunk sc per thread), each stored as a
// row copy (k_off, the A operand of sb_scores), a transposed-read copy (v_off, tr_frag) or both: LDS tiles in the order
// [R0][T0][R1][T1], present ones only.
template <bool R0, bool T0, bool R1, bool T1>
struct SbStage {
  static constexpr int BYTES = (R0 + T0 + R1 + T1) * SB_TILE;
  u32x4 a[2], b[2];

  // rows t0.. of the N token rows whose first is row0; rows past N read zeros.  Both offsets are formed before the two
  // loads: with the selects written inside the load calls and two row strides, the compiler branched around the first
  // operand's loads and waited for them before the second's (sa_bwd_dkv_kernel up to 13 % slower on the long
  // cross-attention loops, profiles/attn_bwd_2026-10-20.json).
  __device__ __forceinline__ void load(__amdgpu_buffer_rsrc_t ra, int lda, __amdgpu_buffer_rsrc_t rb, int ldb, int row0,
                                       int t0, int N, int h, int tid) {
    const int sc = tid & 7, sr = tid >> 3;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = t0 + sr + 32 * i;
      const int oa = r < N ? ((row0 + r) * lda + h * 64 + sc * 8) * 2 : kOOB;
      const int ob = r < N ? ((row0 + r) * ldb + h * 64 + sc * 8) * 2 : kOOB;
      a[i] = buf_load16(ra, oa);
      b[i] = buf_load16(rb, ob);
    }
  }

  __device__ __forceinline__ void store(char* buf, int tid) const {
    const int sc = tid & 7, sr = tid >> 3;
    constexpr int t0 = R0 * SB_TILE, r1 = t0 + T0 * SB_TILE, t1 = r1 + R1 * SB_TILE;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = sr + 32 * i;
      if (R0) *reinterpret_cast<u32x4*>(buf + k_off(row, sc)) = a[i];
      if (T0) *reinterpret_cast<u32x4*>(buf + t0 + v_off(row, sc)) = a[i];
      if (R1) *reinterpret_cast<u32x4*>(buf + r1 + k_off(row, sc)) = b[i];
      if (T1) *reinterpret_cast<u32x4*>(buf + t1 + v_off(row, sc)) = b[i];
    }
  }
};

// S = A0 . b0^T and dP = A1 . b1^T of the 64 LDS rows at A0 / A1 (k_off layout) against the wave's 32 register rows:
// s[rt][cb], lane col = register row 16 cb + fr, rows = LDS row 16 rt + 4 g + i.  (K / V against Q^T / dO^T in dQ, Q / dO
// against K / V in dK/dV.)
__device__ __forceinline__ void sb_scores(const char* A0, const char* A1, const bf16x8 (&b0)[2][2],
                                          const bf16x8 (&b1)[2][2], f32x4 (&s)[4][2], f32x4 (&dp)[4][2], int lane) {
  const int fr = lane & 15, g = lane >> 4;
#pragma unroll
  for (int rt = 0; rt < 4; ++rt) {
    bf16x8 a0[2], a1[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      a0[kk] = *reinterpret_cast<const bf16x8*>(A0 + k_off(rt * 16 + fr, kk * 4 + g));
      a1[kk] = *reinterpret_cast<const bf16x8*>(A1 + k_off(rt * 16 + fr, kk * 4 + g));
    }
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      f32x4 a{0.f, 0.f, 0.f, 0.f}, c{0.f, 0.f, 0.f, 0.f};
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[0], b0[cb][0], a, 0, 0, 0);
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[1], b0[cb][1], a, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[0], b1[cb][0], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[1], b1[cb][1], c, 0, 0, 0);
      s[rt][cb] = a;
      dp[rt][cb] = c;
    }
  }
}

// one transposed A fragment: T^T[d = 16 db + li][rows 32 st + 4 g + {0..3}, 32 st + 16 + 4 g + {0..3}]
__device__ __forceinline__ bf16x8 tr_frag(const char* T, int st, int db, int lane) {
  const int li = lane & 15, g = lane >> 4;
  const int r0 = st * 32 + g * 4 + (li >> 2);
  const int col = db * 16 + (li & 3) * 4;
  const int ch = col >> 3, within = (col & 7) * 2;
  return cat_tr(ds_read_tr(T + v_off(r0, ch) + within), ds_read_tr(T + v_off(r0 + 16, ch) + within));
}

// acc[db][cb] += T^T . pf[cb] over the 32 rows of k-step st of the v_off tile T
__device__ __forceinline__ void sb_accum(f32x4 (&acc)[4][2], const char* T, int st, int db, const bf16x8 (&pf)[2],
                                         int lane) {
  const bf16x8 tf = tr_frag(T, st, db, lane);
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) acc[db][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tf, pf[cb], acc[db][cb], 0, 0, 0);
}

}  // namespace vst
