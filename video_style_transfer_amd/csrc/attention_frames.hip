// Cross-frame (extended) spatial self-attention (DESIGN.md "Cross-frame spatial self-attention").
//
// vst_spatial_attention_frames: the keys and values of query frame f of clip b are the frame's own N tokens followed by
// the tokens of up to two source frames of the same clip (an absolute frame index, or the previous frame):
//   o[b, f] = softmax(q[b, f] . [K[b, f]; K[b, s1(f)]; K[b, s2(f)]]^T * scale) . [V[b, f]; V[b, s1(f)]; V[b, s2(f)]]
// one softmax over the concatenated keys, per head.  A source that resolves to a frame already in the list is dropped
// (frame 0 with source 0 attends to itself only).  No line of the reference does this; the definition is this
// project's.
//
// sa_frames_kernel is sa_self_kernel's loop (attention.hip; its tile step is sa_tile, attn_fwd.h), expression for
// expression: 4 waves x 32 queries, 64-key K/V tiles double-buffered through registers into LDS, S^T = K.Q^T with the
// query on the lane, online softmax from -inf against the running max, P rounded to bf16 unnormalised, O^T = V^T.P^T
// from transposed V reads.  It keeps a copy of that step instead of calling sa_tile: as a shell over attn_fwd.h
// (same registers and occupancy, 150 VGPRs, no spills) it measured 0.7 % / 1.1 % slower at the 32^2 level with one /
// two sources, outside the parent's own 0.3 % run-to-run range (profiles/attn_core_2026-10-19.json); the compiler then
// keeps the load cursor's tile index in a VGPR and forms the K/V addresses in 5 VALU instructions instead of 2.  A
// change to sa_tile's arithmetic must be repeated here; test_frames_bits_equal_plain_kernel fails otherwise.  The only change
// is where a tile's rows come from: the key-tile loop walks the frames of the list one after the other, every frame in
// 64-key tiles of its own (keys are not packed across frames, so with N % 64 != 0 every frame's last tile is masked
// separately), and the running max, sum and O carry across a frame boundary exactly as across two tiles of one frame.
// The tile after the last tile of a frame is tile 0 of the next one, so the register prefetch runs across the boundary
// and a boundary exposes no extra latency.  The list is wave-uniform: it is computed from (f, src1, src2) in scalars.
// K/V are read in place through the same buffer resources (no gather copy, no workspace, no atomics, no lse).
// With N % 64 == 0 the output bits are those of sa_self_kernel on the physically concatenated K/V; with no source
// they are those of sa_self_kernel on the frame itself (tests/test_cross_frame_gpu.py).
#include "attn_common.h"

namespace vst {

// src >= 0: that frame; -2: the previous frame (frame 0: itself); -1: none
__device__ __forceinline__ int sf_source(int src, int f) { return src == -2 ? max(f - 1, 0) : src; }

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void sa_frames_kernel(
    const bf16_t* __restrict__ Q, int ldq, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V, int ldkv,
    bf16_t* __restrict__ O, int ldo, int nclip, int F, int heads, int N, int src1, int src2, float scale_log2,
    uint32_t q_bytes, uint32_t kv_bytes) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int nqb = (N + 127) / 128;
  const int wg = xcd_remap(blockIdx.x, nqb * heads * nclip * F);
  const int qblk = wg % nqb;
  const int bh = wg / nqb;
  const int h = bh % heads, b = bh / heads;  // b = clip * F + f
  const int f = b % F;
  const int fr = lane & 15, g = lane >> 4;

  // key/value frame list [f, s1, s2] without repeats (scalars: every operand is uniform over the workgroup)
  int s1 = sf_source(src1, f), s2 = sf_source(src2, f);
  if (s1 == f) s1 = -1;
  if (s2 == f || s2 == s1) s2 = -1;
  if (s1 < 0) {
    s1 = s2;
    s2 = -1;
  }
  const int nf = 1 + (s1 >= 0) + (s2 >= 0);
  const int row0 = b * N;
  const int row1 = s1 >= 0 ? (b - f + s1) * N : row0;
  const int row2 = s2 >= 0 ? (b - f + s2) * N : row0;

  const auto rq = make_rsrc(Q, q_bytes);
  const auto rk = make_rsrc(K, kv_bytes);
  const auto rv = make_rsrc(V, kv_bytes);

  bf16x8 qf[2][2];
  const int qbase = qblk * 128 + wid * 32;
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const int q = qbase + qb * 16 + fr;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int off = q < N ? ((row0 + q) * ldq + h * 64 + kk * 32 + g * 8) * 2 : kOOB;
      qf[qb][kk] = __builtin_bit_cast(bf16x8, buf_load16(rq, off));
    }
  }

  const int sc = tid & 7, sr = tid >> 3;  // rows sr, sr + 32
  u32x4 kreg[2], vreg[2];
  auto load_kv = [&](int row, int t) {  // tile t of the frame whose first token row is `row`
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int key = t * SA_KT + sr + 32 * i;
      const int off = key < N ? ((row + key) * ldkv + h * 64 + sc * 8) * 2 : kOOB;
      kreg[i] = buf_load16(rk, off);
      vreg[i] = buf_load16(rv, off);
    }
  };
  auto store_kv = [&](int buf) {
    char* Ks = smem + buf * 2 * SA_TILE;
    char* Vs = Ks + SA_TILE;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = sr + 32 * i;
      *reinterpret_cast<u32x4*>(Ks + k_off(row, sc)) = kreg[i];
      *reinterpret_cast<u32x4*>(Vs + v_off(row, sc)) = vreg[i];
    }
  };

  f32x4 o[4][2];
#pragma unroll
  for (int d = 0; d < 4; ++d)
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) o[d][qb] = f32x4{0.f, 0.f, 0.f, 0.f};
  float mrun[2] = {-INFINITY, -INFINITY};
  float mb[2] = {0.f, 0.f};  // mrun * scale_log2
  float lrun[2] = {0.f, 0.f};

  const int ntf = (N + SA_KT - 1) / SA_KT;  // tiles per frame
  const int nt = nf * ntf;
  int voff[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) {
    const int li = lane & 15, r0 = g * 4 + (li >> 2), col = db * 16 + (li & 3) * 4;
    voff[db] = v_off(r0, col >> 3) + (col & 7) * 2;
  }
  // (lrow, lt): frame and tile of the next load; it steps to tile 0 of the next frame after a frame's last tile
  int lrow = row0, lt = 0, lj = 0;
  auto load_next = [&]() {
    load_kv(lrow, lt);
    if (++lt == ntf) {
      lt = 0;
      lrow = ++lj == 1 ? row1 : row2;
    }
  };
  load_next();
  store_kv(0);
  __syncthreads();

  int t = 0;  // tile inside the frame being computed
  for (int tt = 0; tt < nt; ++tt) {
    const int cur = tt & 1;
    if (tt + 1 < nt) load_next();
    const char* Ks = smem + cur * 2 * SA_TILE;
    const char* Vs = Ks + SA_TILE;

    f32x4 s[4][2];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      bf16x8 kf[2];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
        kf[kk] = *reinterpret_cast<const bf16x8*>(Ks + k_off(kt * 16 + fr, kk * 4 + g));
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) {
        f32x4 a{0.f, 0.f, 0.f, 0.f};
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[0], qf[qb][0], a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[1], qf[qb][1], a, 0, 0, 0);
        s[kt][qb] = a;
      }
    }
    if ((t + 1) * SA_KT > N) {  // the last tile of every frame of the list
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool dead = t * SA_KT + kt * 16 + g * 4 + i >= N;
#pragma unroll
          for (int qb = 0; qb < 2; ++qb)
            if (dead) s[kt][qb][i] = -INFINITY;
        }
    }
    // sa_self_kernel's softmax, expression for expression (max from -inf, P = exp2(s sl2 - mb), l = l alpha + sum P)
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
      const float mnew = fmaxf(mrun[qb], mx[qb]);
      alpha[qb] = fast_exp2((mrun[qb] - mnew) * scale_log2);
      mrun[qb] = mnew;
      mb[qb] = mnew * scale_log2;
#pragma unroll
      for (int d = 0; d < 4; ++d) o[d][qb] *= alpha[qb];
    }
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      float ls = 0.f;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float pv = fast_exp2(s[kt][qb][i] * scale_log2 - mb[qb]);
          s[kt][qb][i] = pv;
          ls += pv;
        }
      lrun[qb] = lrun[qb] * alpha[qb] + ls;
    }
    bf16x8 pf[2][2];
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int qb = 0; qb < 2; ++qb)
        pf[st][qb] = pack_p8(s[2 * st][qb][0], s[2 * st][qb][1], s[2 * st][qb][2], s[2 * st][qb][3],
                             s[2 * st + 1][qb][0], s[2 * st + 1][qb][1], s[2 * st + 1][qb][2], s[2 * st + 1][qb][3]);
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      const char* vp = Vs + voff[db];
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        const bf16x8 vf = cat_tr(ds_read_tr(vp + st * 4096), ds_read_tr(vp + st * 4096 + 2048));
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
          o[db][qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[st][qb], o[db][qb], 0, 0, 0);
      }
    }
    if (tt + 1 < nt) store_kv(cur ^ 1);
    __syncthreads();
    if (++t == ntf) t = 0;
  }

#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    float l = lrun[qb];
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    const float inv = 1.0f / l;
    const int q = qbase + qb * 16 + fr;
    if (q >= N) continue;
    bf16_t* orow = O + (size_t)(row0 + q) * ldo + h * 64;
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      const f32x4 v = o[db][qb] * inv;
      u32x2 w{pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
      *reinterpret_cast<u32x2*>(orow + db * 16 + g * 4) = w;
    }
  }
}

}  // namespace vst

using namespace vst;

extern "C" int vst_spatial_attention_frames(const void* q, int ldq, const void* k, const void* v, int ldkv, void* o,
                                            int ldo, int nclip, int F, int heads, int N, int src1, int src2,
                                            int head_dim, float scale, void* stream) {
  Fit31 fit;
  if (head_dim != 64 || !q || !k || !v || !o || nclip <= 0 || F <= 0 || heads <= 0 || N <= 0) return VST_ERR_ARG;
  if ((ldq & 7) || (ldkv & 7) || (ldo & 7)) return VST_ERR_ARG;
  if (src1 < -2 || src2 < -2 || src1 >= F || src2 >= F) return VST_ERR_ARG;
  if ((src1 == -1 && src2 != -1) || (src1 != -1 && src1 == src2)) return VST_ERR_ARG;
  if ((size_t)nclip * F * N > 0x7fffffffULL) return VST_ERR_ARG;
  const int rows = nclip * F * N;
  const uint32_t qb = fit(((size_t)(rows - 1) * ldq + heads * 64) * 2);
  // K and V may be column views of one fused buffer; each rsrc is sized from its own base
  const uint32_t kvb = fit(((size_t)(rows - 1) * ldkv + heads * 64) * 2);
  fit(((size_t)(rows - 1) * ldo + heads * 64) * 2);
  if (fit.over) return VST_ERR_ARG;  // past the 32-bit buffer offsets: refuse, never read zeros
  const size_t nwg = (size_t)((N + 127) / 128) * heads * nclip * F;
  if (nwg > 0x7fffffffULL) return VST_ERR_ARG;
  hipLaunchKernelGGL(sa_frames_kernel, dim3((unsigned)nwg), dim3(256), SA_LDS, (hipStream_t)stream, (const bf16_t*)q,
                     ldq, (const bf16_t*)k, (const bf16_t*)v, ldkv, (bf16_t*)o, ldo, nclip, F, heads, N, src1, src2,
                     scale * kLog2e, qb, kvb);
  return launch_status();
}
