// Sliding-window frame attention for clips longer than the motion modules' trained length (DESIGN.md "Long clips").
//
// vst_temporal_attention_windowed: every (clip, pixel, head) attends inside windows of L frames that start at
// 0, S, 2S, ... (plus one at F - L when the last of those does not end the clip), and the windows' results are blended
// per frame with flat or pyramid weights:  o[f] = sum_s w[f-s] O_s[f-s] / sum_s w[f-s].  q/k/v hold one projection per
// frame WITHOUT the positional term; the kernel adds the fp32 table row of the position INSIDE the window
// (pos_*[j] = pe[j] . W^T) and rounds to bf16, so one q/k/v GEMM serves every window a frame belongs to.
//
// One wave per (clip, pixel, head), as in temporal_attn_kernel, with which it shares the softmax, the P packing and the
// transposed V read (attn_fwd.h), so a window's attention rounds as that kernel's does.
// The wave walks its windows in ascending order.  Its lane layout ties a lane to a position j inside the window, not
// to a frame, so
//   - the table rows a lane adds are the same in every window: they are loaded once into registers;
//   - the running blend of a frame moves between lanes from one window to the next: it lives in an fp32 ring
//     [16 NT][D] in LDS, indexed by frame & (16 NT - 1).  A frame that no later window covers is scaled by
//     1 / sum w and stored as bf16 by the lane that just added to it (every output element is written exactly once);
//     the others go back to the ring.
// The q/k/v rows that consecutive windows share are read again; the same wave touched them one window earlier.
// No workspace, no atomics.
#include "attn_fwd.h"

namespace vst {

template <int NT, int D>
struct TW {
  static constexpr int KS = (D + 31) / 32;  // 32-deep k-steps for S
  static constexpr int DB = (D + 15) / 16;  // 16-wide d blocks for O
  static constexpr int NF = 16 * NT;
  static constexpr int VROW = DB * 32;  // bytes per V row in LDS
  static constexpr int CPR = VROW / 16;
  static constexpr int NV = (NF * CPR + 63) / 64;
  static constexpr int VBYTES = NV * 1024;  // one wave's V tile, whole 1-KiB pieces (every lane stores)
  // ring row stride in floats: DB*16 + 4 is 4 mod 8, so the 8 lanes of a ds_write_b128 group (8 consecutive frames,
  // 16 B each) cover the 32 banks once
  static constexpr int RS = DB * 16 + 4;
  static constexpr int RBYTES = NF * RS * 4;
  static constexpr int WBYTES = VBYTES + RBYTES;  // LDS per wave
  // waves per workgroup: at most 8 (one (clip, pixel)'s heads) inside the 64 KiB a launch gets without opting in
  static constexpr int WAVES = (64 * 1024 / WBYTES) < 8 ? (64 * 1024 / WBYTES) : 8;
  static_assert(WAVES >= 1, "one wave's V tile + ring must fit 64 KiB");
};

__device__ __forceinline__ float tw_weight(int j, int L, int pyramid) {
  return pyramid ? (float)min(j + 1, L - j) : 1.0f;
}

template <int NT, int D>
__global__ __launch_bounds__((64 * TW<NT, D>::WAVES)) void temporal_attn_windowed_kernel(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V, int ldqkv,
    const float* __restrict__ PQ, const float* __restrict__ PK, const float* __restrict__ PV, int ldpos,
    bf16_t* __restrict__ O, int ldo, int nclip, int F, int HW, int heads, int L, int S, int pyramid,
    float scale_log2, uint32_t qkv_bytes) {
  using W = TW<NT, D>;
  constexpr int KS = W::KS, DB = W::DB, NF = W::NF, VROW = W::VROW, CPR = W::CPR, NV = W::NV, RS = W::RS;
  extern __shared__ __attribute__((aligned(16))) char wsm[];  // [waves][V tile | ring]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int unit = blockIdx.x * (blockDim.x >> 6) + wid;
  const int nunits = nclip * HW * heads;
  if (unit >= nunits) return;  // whole wave exits (unit is wave-uniform)
  const int h = unit % heads;
  const int bp = unit / heads;
  const int b = bp / HW, p = bp - b * HW;
  const int fr = lane & 15, g = lane >> 4;
  char* vs = wsm + wid * W::WBYTES;
  float* ring = reinterpret_cast<float*>(vs + W::VBYTES);

  const auto rq = make_rsrc(Q, qkv_bytes);
  const auto rk = make_rsrc(K, qkv_bytes);
  const auto rv = make_rsrc(V, qkv_bytes);
  auto row_of = [&](int f) { return (b * F + f) * HW + p; };

  // ---- the table rows of this lane's window positions (zeros without a table, past L and past D) ----
  float tv[NV][8], tq[KS][NT][8], tk[KS][NT][8];
  auto load_pos = [&](const float* P, int j, int d, bool on, float* t) {
    f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = lo;
    if (P && on) {
      const float* src = P + (size_t)j * ldpos + h * D + d;
      lo = *reinterpret_cast<const f32x4*>(src);
      hi = *reinterpret_cast<const f32x4*>(src + 4);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = lo[i], t[4 + i] = hi[i];
  };
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int idx = lane + 64 * j;
    const int f = idx / CPR, c = idx - f * CPR;
    load_pos(PV, f, c * 8, idx < NF * CPR && f < L && c * 8 < D, tv[j]);
  }
#pragma unroll
  for (int kk = 0; kk < KS; ++kk)
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) {
      const int j = tt * 16 + fr, d0 = kk * 32 + g * 8;
      load_pos(PQ, j, d0, j < L && d0 < D, tq[kk][tt]);
      load_pos(PK, j, d0, j < L && d0 < D, tk[kk][tt]);
    }
  // bf16(float(x) + t) of 8 values: the rounding point of "LayerNorm + PE, then the projection" moved behind the GEMM
  auto add_pos = [&](u32x4 x, const float* t) {
    float f[8];
    unpack8(x, f);
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] += t[i];
    return pack8(f);
  };

  const int nreg = (F - L) / S + 1;           // starts 0, S, ..., (nreg - 1) S
  const int tail = (nreg - 1) * S != F - L;   // one more window at F - L
  const int nwin = nreg + tail;
  auto start_of = [&](int wi) { return wi < nreg ? wi * S : F - L; };
  // 1 / (sum of the weights frame f receives over all windows that hold it)
  auto inv_wsum = [&](int f) {
    const int k0 = f >= L ? (f - L) / S + 1 : 0;
    const int k1 = min(nreg - 1, f / S);
    float ws = 0.f;
    for (int k = k0; k <= k1; ++k) ws += tw_weight(f - k * S, L, pyramid);
    if (tail && f >= F - L) ws += tw_weight(f - (F - L), L, pyramid);
    return 1.0f / ws;
  };

  int live_end = 0;  // frames below it hold a running blend in the ring
  for (int wi = 0; wi < nwin; ++wi) {
    const int s0 = start_of(wi);
    const int done_end = wi + 1 < nwin ? start_of(wi + 1) : s0 + L;  // frames [s0, done_end) see no later window

    // ---- V rows into registers (zero rows >= L and columns >= D); they go to LDS after the S MFMAs ----
    u32x4 vreg[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int idx = lane + 64 * j;
      const int f = idx / CPR, c = idx - f * CPR;
      const int off = (idx < NF * CPR && f < L && c * 8 < D) ? (row_of(s0 + f) * ldqkv + h * D + c * 8) * 2 : kOOB;
      vreg[j] = buf_load16(rv, off);
    }
    __builtin_amdgcn_sched_barrier(0);  // every V load issues before the K / Q loads

    // ---- S^T = K Q^T ----
    f32x4 s[NT][NT];
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
      for (int c = 0; c < NT; ++c) s[a][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      const int d0 = kk * 32 + g * 8;
      bf16x8 kf[NT], qf[NT];
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) {
        const int j = tt * 16 + fr;
        const int off = (j < L && d0 < D) ? (row_of(s0 + j) * ldqkv + h * D + d0) * 2 : kOOB;
        kf[tt] = __builtin_bit_cast(bf16x8, add_pos(buf_load16(rk, off), tk[kk][tt]));
        qf[tt] = __builtin_bit_cast(bf16x8, add_pos(buf_load16(rq, off), tq[kk][tt]));
      }
#pragma unroll
      for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int c = 0; c < NT; ++c)
          s[a][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[a], qf[c], s[a][c], 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < NV; ++j)  // chunk idx = f * CPR + c sits at byte idx * 16; the pad chunks get zeros
      *reinterpret_cast<u32x4*>(vs + (lane + 64 * j) * 16) = add_pos(vreg[j], tv[j]);
    // keys >= L masked; softmax per query column
    float inv[NT];
    ta_softmax<NT>(s, L, scale_log2, inv, lane);
    // the blend weight of this lane's query positions, and 1 / sum w for those that finish in this window
    float wj[NT], rws[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) {
      const int j = c * 16 + fr;
      wj[c] = tw_weight(j, L, pyramid);
      rws[c] = (j < L && s0 + j < done_end) ? inv_wsum(s0 + j) : 0.f;
    }
    // V staging stores (this wave only) complete before the transposed reads
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");

    // ---- O^T = V^T P^T (one 32-key k-step) ----
    bf16x8 pf[NT];
    ta_pack_p<NT>(s, pf);
#pragma unroll
    for (int db = 0; db < DB; ++db) {
      const bf16x8 vf = ta_vt_frag<NT>(vs, VROW, db, lane);
#pragma unroll
      for (int c = 0; c < NT; ++c) {
        f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[c], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        const int j = c * 16 + fr;
        const int f = s0 + j;
        const int d = db * 16 + g * 4;
        if (j < L && d < D) {
          acc *= inv[c];
          f32x4* slot = reinterpret_cast<f32x4*>(ring + (f & (NF - 1)) * RS + d);
          f32x4 run = f32x4{0.f, 0.f, 0.f, 0.f};
          if (f < live_end) run = *slot;  // earlier windows' share, written by another lane of this wave
          run += acc * wj[c];
          if (f < done_end) {
            run *= rws[c];
            u32x2 w{pack2bf(run[0], run[1]), pack2bf(run[2], run[3])};
            *reinterpret_cast<u32x2*>(O + (size_t)row_of(f) * ldo + h * D + d) = w;
          } else {
            *slot = run;
          }
        }
      }
    }
    live_end = s0 + L;
    // the transposed V reads and the ring traffic of this window complete before the next window's V stores
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
}

template <int NT, int D>
static int launch_windowed(const bf16_t* Q, const bf16_t* K, const bf16_t* V, int ld, const float* PQ, const float* PK,
                           const float* PV, int ldpos, bf16_t* O, int ldo, int nclip, int F, int HW, int heads, int L,
                           int S, int pyramid, float sl2, uint32_t bytes, hipStream_t s) {
  using W = TW<NT, D>;
  const int units = nclip * HW * heads;
  // all heads of a (clip, pixel) in one workgroup when their V tiles and rings fit, else 4, 2 or 1 units (8 heads
  // then split into whole workgroups)
  const int wpg = heads <= W::WAVES ? heads : W::WAVES >= 4 ? 4 : W::WAVES >= 2 ? 2 : 1;
  hipLaunchKernelGGL((temporal_attn_windowed_kernel<NT, D>), dim3((units + wpg - 1) / wpg), dim3(64 * wpg),
                     wpg * W::WBYTES, s, Q, K, V, ld, PQ, PK, PV, ldpos, O, ldo, nclip, F, HW, heads, L, S, pyramid,
                     sl2, bytes);
  return launch_status();
}

}  // namespace vst

using namespace vst;

extern "C" int vst_temporal_attention_windowed(const void* q, const void* k, const void* v, int ldqkv,
                                               const float* pos_q, const float* pos_k, const float* pos_v, int ldpos,
                                               void* o, int ldo, int nclip, int F, int HW, int heads, int head_dim,
                                               int L, int S, int weighting, float scale, void* stream) {
  Fit31 fit;
  if (!q || !k || !v || !o || nclip <= 0 || HW <= 0 || heads <= 0) return VST_ERR_ARG;
  if (L < 1 || L > 32 || S < 1 || S > L || F < L || (weighting != 0 && weighting != 1)) return VST_ERR_ARG;
  if ((ldqkv & 7) || (ldo & 7) || (head_dim & 7)) return VST_ERR_ARG;
  // the table rows are read as 16-byte vectors
  if (pos_q || pos_k || pos_v) {
    if ((ldpos & 3) || ldpos < heads * head_dim) return VST_ERR_ARG;
    if ((((uintptr_t)pos_q | (uintptr_t)pos_k | (uintptr_t)pos_v) & 15)) return VST_ERR_ARG;
  }
  if ((size_t)nclip * F * HW > 0x7fffffffULL) return VST_ERR_ARG;
  const uint32_t bytes = fit(((size_t)(nclip * F * HW - 1) * ldqkv + heads * head_dim) * 2);
  if (fit.over) return VST_ERR_ARG;  // past the 32-bit buffer offsets: refuse, never read zeros
  const float sl2 = scale * kLog2e;
  hipStream_t s = (hipStream_t)stream;
  const bf16_t *Q = (const bf16_t*)q, *K = (const bf16_t*)k, *V = (const bf16_t*)v;
  bf16_t* O = (bf16_t*)o;
#define VST_TW(D)                                                                                                 \
  case D:                                                                                                         \
    return L <= 16 ? launch_windowed<1, D>(Q, K, V, ldqkv, pos_q, pos_k, pos_v, ldpos, O, ldo, nclip, F, HW, heads, \
                                           L, S, weighting, sl2, bytes, s)                                        \
                   : launch_windowed<2, D>(Q, K, V, ldqkv, pos_q, pos_k, pos_v, ldpos, O, ldo, nclip, F, HW, heads, \
                                           L, S, weighting, sl2, bytes, s);
  switch (head_dim) {
    VST_TW(8)
    VST_TW(16)
    VST_TW(24)
    VST_TW(32)
    VST_TW(40)
    VST_TW(48)
    VST_TW(56)
    VST_TW(64)
    VST_TW(72)
    VST_TW(80)
    VST_TW(88)
    VST_TW(96)
    VST_TW(104)
    VST_TW(112)
    VST_TW(120)
    VST_TW(128)
    VST_TW(136)
    VST_TW(144)
    VST_TW(152)
    VST_TW(160)
    default:
      return VST_ERR_ARG;
  }
#undef VST_TW
}
