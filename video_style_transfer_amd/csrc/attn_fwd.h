// The forward cores that the attention kernels share.
//
// 1) Spatial, head_dim 64 (spatial_attn_kernel<PRE>, sa_self_kernel: attention.hip).  A workgroup is 4 waves x 32
//    queries; a wave keeps its Q^T fragments, the running softmax state and the O^T accumulators in registers and
//    consumes K/V in 64-key tiles from LDS.  The kernels are shells: each does its own index math and decides where a
//    tile's K/V rows come from and which keys are masked; everything that rounds (S^T = K.Q^T, online softmax, P
//    packing, O^T += V^T.P^T, finalize) is sa_tile / sa_finish, so the kernels' outputs are bit-identical wherever
//    their key sets agree (test_sa_self_bitwise_equals_spatial_attn, test_causal_attention).  sa_frames_kernel
//    (attention_frames.hip) still carries a copy of this step; its head comment says why.
//
// 2) Frame axis (temporal_attn_kernel: attention.hip; temporal_attn_windowed_kernel: temporal_window.hip).  One wave per
//    (clip, pixel, head) holds the whole NT x NT score tile; the kernels share the masked one-pass softmax, the P
//    packing and the transposed V fragment read (test_windowed_bit_anchors).  Their Q/K loads (position add) and their
//    output paths (ring blend) differ and stay with the kernels.
//
// The backward kernels (attn_bwd.h) take from here what they round as the forward does: sa_load_rows, sa_zero,
// sa_pack2, sa_store_row, and ta_softmax / ta_pack_p / ta_vt_frag.
#pragma once
#include "attn_common.h"

namespace vst {

// ---------------------------------------------------------------------------------
// Spatial core
// ---------------------------------------------------------------------------------

// Per-wave running state: O^T accumulators [d-block][q-block] (lane col q, rows d = 16db + 4g + i), running max of the
// raw scores, the same max in the exp2 domain, and this lane group's share of the running sum.
struct SaState {
  f32x4 o[4][2];
  float mrun[2], mb[2], lrun[2];
};

// A transposed accumulator [d-block][row-block] (lane col = token row, rows d = 16db + 4g + i) from zero
__device__ __forceinline__ void sa_zero(f32x4 (&acc)[4][2]) {
#pragma unroll
  for (int d = 0; d < 4; ++d)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) acc[d][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
}

__device__ __forceinline__ void sa_init(SaState& st) {
  sa_zero(st.o);
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) st.mrun[qb] = -INFINITY, st.mb[qb] = 0.f, st.lrun[qb] = 0.f;
}

// B fragments of the wave's 32 token rows base..base+31 (of N) of the batch whose first token row is row0: lane (col
// r, group g) holds X[r][32kk + 8g .. +7]; rows past N read zeros.  Q^T for S^T = K.Q^T, and every register operand of
// the backward kernels.
__device__ __forceinline__ void sa_load_rows(bf16x8 (&xf)[2][2], __amdgpu_buffer_rsrc_t rx, int row0, int base, int N,
                                             int ld, int h, int lane) {
  const int fr = lane & 15, g = lane >> 4;
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) {
    const int r = base + cb * 16 + fr;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int off = r < N ? ((row0 + r) * ld + h * 64 + kk * 32 + g * 8) * 2 : kOOB;
      xf[cb][kk] = __builtin_bit_cast(bf16x8, buf_load16(rx, off));
    }
  }
}

// The forward's Q^T fragments
__device__ __forceinline__ void sa_load_q(bf16x8 (&qf)[2][2], __amdgpu_buffer_rsrc_t rq, int row0, int qbase, int Nq,
                                          int ldq, int h, int lane) {
  sa_load_rows(qf, rq, row0, qbase, Nq, ldq, h, lane);
  // The Q loads issue before the first K/V loads.  Sunk behind them, they are still in flight after the first tile's
  // LDS stores, and their s_waitcnt vmcnt lands inside the key loop, where on every later tile it waits for the
  // prefetch of the next one (sa_self_kernel 32x32: 146 -> 149 us).
  __builtin_amdgcn_sched_barrier(0);
}

// K/V register staging of one tile: 64 rows x 8 chunks = 512 16-B chunks per operand, 2 per thread (rows sr, sr + 32)
struct SaStage {
  u32x4 kreg[2], vreg[2];

  // tile t of the Nk keys whose first token row is `row`; keys past Nk read zeros
  __device__ __forceinline__ void load(__amdgpu_buffer_rsrc_t rk, __amdgpu_buffer_rsrc_t rv, int row, int t, int Nk,
                                       int ldkv, int h, int tid) {
    const int sc = tid & 7, sr = tid >> 3;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int key = t * SA_KT + sr + 32 * i;
      const int off = key < Nk ? ((row + key) * ldkv + h * 64 + sc * 8) * 2 : kOOB;
      kreg[i] = buf_load16(rk, off);
      vreg[i] = buf_load16(rv, off);
    }
  }

  // into the K and V tiles of LDS buffer `buf`, swizzled
  __device__ __forceinline__ void store(char* smem, int buf, int tid) const {
    const int sc = tid & 7, sr = tid >> 3;
    char* Ks = smem + buf * 2 * SA_TILE;
    char* Vs = Ks + SA_TILE;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = sr + 32 * i;
      *reinterpret_cast<u32x4*>(Ks + k_off(row, sc)) = kreg[i];
      *reinterpret_cast<u32x4*>(Vs + v_off(row, sc)) = vreg[i];
    }
  }
};

typedef __attribute__((address_space(3))) void sa_lds_void;

// One 1-KiB LDS-DMA piece: 64 lanes x 16 B, lane-linear in LDS at `lds_piece` (wave-uniform).
__device__ __forceinline__ void sa_dma16(__amdgpu_buffer_rsrc_t r, char* lds_piece, int off) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(
      r, (sa_lds_void*)((__attribute__((address_space(3))) char*)(uintptr_t)lds_piece), 16, off, 0, 0, 0);
}

// V^T fragment reads: lane 4q'+p' of group g reads row 4g + q' (+16, +32, +48), cols 16db + 4p'
__device__ __forceinline__ void sa_voffs(int (&voff)[4], int lane) {
  const int li = lane & 15, g = lane >> 4;
#pragma unroll
  for (int db = 0; db < 4; ++db) {
    const int r0 = g * 4 + (li >> 2), col = db * 16 + (li & 3) * 4;
    voff[db] = v_off(r0, col >> 3) + (col & 7) * 2;
  }
}

// Keys of tile t at or past Nk get -inf; with causal_q0 >= 0 (the wave's first query) so do the keys after the query
// (CLIP text self-attention).  Callers that never pass causal_q0 compile no causal compare: in the long self-attention
// kernels it cost 31 SGPR spills (see sa_self_kernel).
__device__ __forceinline__ void sa_mask(f32x4 (&s)[4][2], int t, int Nk, int lane, int causal_q0 = -1) {
  const int fr = lane & 15, g = lane >> 4;
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int key = t * SA_KT + kt * 16 + g * 4 + i;
#pragma unroll
      for (int qb = 0; qb < 2; ++qb)
        if (key >= Nk || (causal_q0 >= 0 && key > causal_q0 + qb * 16 + fr)) s[kt][qb][i] = -INFINITY;
    }
}

// The bf16 B fragment of 32-deep k-step ks from the accumulator tiles t[2ks][cb] (elements 0-3) and t[2ks+1][cb] (4-7):
// P^T in the forward, P / dS in the backward
__device__ __forceinline__ bf16x8 sa_pack2(const f32x4 (&t)[4][2], int ks, int cb) {
  return pack_p8(t[2 * ks][cb][0], t[2 * ks][cb][1], t[2 * ks][cb][2], t[2 * ks][cb][3], t[2 * ks + 1][cb][0],
                 t[2 * ks + 1][cb][1], t[2 * ks + 1][cb][2], t[2 * ks + 1][cb][3]);
}

// Column block cb of a transposed accumulator, times scale, as the 64 bf16 of the lane's token row
__device__ __forceinline__ void sa_store_row(const f32x4 (&acc)[4][2], int cb, float scale, bf16_t* row, int lane) {
  const int g = lane >> 4;
#pragma unroll
  for (int db = 0; db < 4; ++db) {
    const f32x4 v = acc[db][cb] * scale;
    u32x2 w{pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
    *reinterpret_cast<u32x2*>(row + db * 16 + g * 4) = w;
  }
}

// One 64-key tile from the K and V tiles at Ks / Vs: S^T, the caller's mask on it, online softmax, O^T += V^T.P^T.
template <class Mask>
__device__ __forceinline__ void sa_tile(const char* Ks, const char* Vs, const bf16x8 (&qf)[2][2], const int (&voff)[4],
                                        float scale_log2, SaState& st, int lane, Mask&& mask) {
  const int fr = lane & 15, g = lane >> 4;
  // ---- S^T = K Q^T : s[kt][qb], lane col q, rows key = 16kt + 4g + i ----
  f32x4 s[4][2];
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) {
    bf16x8 kf[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) kf[kk] = *reinterpret_cast<const bf16x8*>(Ks + k_off(kt * 16 + fr, kk * 4 + g));
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      f32x4 a{0.f, 0.f, 0.f, 0.f};
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[0], qf[qb][0], a, 0, 0, 0);
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[1], qf[qb][1], a, 0, 0, 0);
      s[kt][qb] = a;
    }
  }
  mask(s);
  // ---- online softmax (lane-local rows; reduce over the 4 g-lanes): max from -inf, P = exp2(s sl2 - mb),
  // l = l alpha + sum P.  One forward arithmetic for inference and training.  (Round 5 wrote P with an explicit fmaf
  // and l as two roundings in one of the then separate copies; that moved outputs by ulps.) ----
  float mx[2], alpha[2];
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int i = 0; i < 4; ++i) m = fmaxf(m, s[kt][qb][i]);
    mx[qb] = group_max(m);
  }
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const float mnew = fmaxf(st.mrun[qb], mx[qb]);
    alpha[qb] = fast_exp2((st.mrun[qb] - mnew) * scale_log2);
    st.mrun[qb] = mnew;
    st.mb[qb] = mnew * scale_log2;
#pragma unroll
    for (int d = 0; d < 4; ++d) st.o[d][qb] *= alpha[qb];
  }
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    float ls = 0.f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float pv = fast_exp2(s[kt][qb][i] * scale_log2 - st.mb[qb]);
        s[kt][qb][i] = pv;
        ls += pv;
      }
    st.lrun[qb] = st.lrun[qb] * alpha[qb] + ls;
  }
  // ---- O^T += V^T P^T: two 32-key k-steps ks (P tiles 2ks -> elements 0-3, 2ks+1 -> 4-7) ----
  bf16x8 pf[2][2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) pf[ks][qb] = sa_pack2(s, ks, qb);
#pragma unroll
  for (int db = 0; db < 4; ++db) {
    const char* vp = Vs + voff[db];  // rows +16 / +32 keep the swizzle: immediate offsets 2048 / 4096
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8 vf = cat_tr(ds_read_tr(vp + ks * 4096), ds_read_tr(vp + ks * 4096 + 2048));
#pragma unroll
      for (int qb = 0; qb < 2; ++qb)
        st.o[db][qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[ks][qb], st.o[db][qb], 0, 0, 0);
    }
  }
}

// Finalize: O[q][d] = O^T[d][q] / l for the batch whose first token row is row0; with lse, the log2-domain logsumexp of
// query q goes to lse[lse0 + q] (training: P = exp2(s sl2 - lse)).
__device__ __forceinline__ void sa_finish(const SaState& st, bf16_t* O, int ldo, int row0, int qbase, int Nq, int h,
                                          float* lse, size_t lse0, float scale_log2, int lane) {
  const int fr = lane & 15, g = lane >> 4;
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    float l = st.lrun[qb];
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    const float inv = 1.0f / l;
    const int q = qbase + qb * 16 + fr;
    if (q >= Nq) continue;
    if (lse && g == 0) lse[lse0 + q] = st.mrun[qb] * scale_log2 + __log2f(l);
    sa_store_row(st.o, qb, inv, O + (size_t)(row0 + q) * ldo + h * 64, lane);
  }
}

// Regional finalize (region_attn_kernel, region_attention.hip): acc^T[d][q] += w[q] * (O^T[d][q] * 1/l) for the lane's
// query columns with w != 0 -- a select, so a column with w == 0 takes nothing from this state, whatever it holds.
// O^T * 1/l is sa_finish's product; the multiply by w and the add are rounded separately.  acc starts from -0.0f
// (sa_blend_init): x + -0 = x for every x, signed zeros included, so a column's first term lands with its own bits.
__device__ __forceinline__ void sa_blend_init(f32x4 (&acc)[4][2]) {
#pragma unroll
  for (int d = 0; d < 4; ++d)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) acc[d][cb] = f32x4{-0.f, -0.f, -0.f, -0.f};
}
__device__ __forceinline__ void sa_blend(const SaState& st, f32x4 (&acc)[4][2], const float (&w)[2]) {
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    float l = st.lrun[qb];
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    const float inv = 1.0f / l;
    if (w[qb] != 0.0f) {
#pragma unroll
      for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          acc[db][qb][i] = __fadd_rn(acc[db][qb][i], __fmul_rn(w[qb], __fmul_rn(st.o[db][qb][i], inv)));
    }
  }
}

// ---------------------------------------------------------------------------------
// Frame-axis core.  NT = number of 16-frame tiles; s[a][c] is the S^T tile of keys 16a.. and queries 16c..
// ---------------------------------------------------------------------------------

// Keys >= n get -inf, then the softmax per query column: s becomes the unnormalised P, inv[c] = 1 / l, mb[c] = the
// column's max in the exp2 domain (the backward recomputes the key-column P from it)
template <int NT>
__device__ __forceinline__ void ta_softmax(f32x4 (&s)[NT][NT], int n, float scale_log2, float (&inv)[NT],
                                           float (&mb)[NT], int lane) {
  const int g = lane >> 4;
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (a * 16 + g * 4 + i >= n) {
#pragma unroll
        for (int c = 0; c < NT; ++c) s[a][c][i] = -INFINITY;
      }
#pragma unroll
  for (int c = 0; c < NT; ++c) {
    float mx = -INFINITY;
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
      for (int i = 0; i < 4; ++i) mx = fmaxf(mx, s[a][c][i]);
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    mb[c] = mx * scale_log2;
    float ls = 0.f;
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float pv = fast_exp2(s[a][c][i] * scale_log2 - mb[c]);
        s[a][c][i] = pv;
        ls += pv;
      }
    ls += __shfl_xor(ls, 16);
    ls += __shfl_xor(ls, 32);
    inv[c] = 1.0f / ls;
  }
}
template <int NT>
__device__ __forceinline__ void ta_softmax(f32x4 (&s)[NT][NT], int n, float scale_log2, float (&inv)[NT], int lane) {
  float mb[NT];
  ta_softmax<NT>(s, n, scale_log2, inv, mb, lane);
}

// P^T B operands of O^T = V^T P^T (one 32-key k-step; for NT = 1 the upper 16 keys are zero)
template <int NT>
__device__ __forceinline__ void ta_pack_p(const f32x4 (&s)[NT][NT], bf16x8 (&pf)[NT]) {
#pragma unroll
  for (int c = 0; c < NT; ++c) {
    if (NT == 2)
      pf[c] = pack_p8(s[0][c][0], s[0][c][1], s[0][c][2], s[0][c][3], s[NT - 1][c][0], s[NT - 1][c][1],
                      s[NT - 1][c][2], s[NT - 1][c][3]);
    else
      pf[c] = pack_p8(s[0][c][0], s[0][c][1], s[0][c][2], s[0][c][3], 0.f, 0.f, 0.f, 0.f);
  }
}

// V^T A fragment of d block db from the wave's row-major V tile (vrow bytes per row)
template <int NT>
__device__ __forceinline__ bf16x8 ta_vt_frag(const char* vs, int vrow, int db, int lane) {
  const int li = lane & 15, g = lane >> 4;
  const int r0 = g * 4 + (li >> 2);
  const int colb = (db * 16 + (li & 3) * 4) * 2;
  const s16x4 lo = ds_read_tr(vs + r0 * vrow + colb);
  s16x4 hi = s16x4{0, 0, 0, 0};
  if (NT == 2) hi = ds_read_tr(vs + (r0 + 16) * vrow + colb);
  return cat_tr(lo, hi);
}

}  // namespace vst
