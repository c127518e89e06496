// IP-Adapter image attention added onto the attn2 output, without q (replaces to_k_ip / to_v_ip + the
// second F.scaled_dot_product_attention + the scaled add of IPAdapterAttnProcessor2_0,
// unziplora_unet/unzip_attention_processor.py:1793-1809).
//
// The image keys are constants of a clip, so they fold into the query projection (host side, fp32):
//   s[m,h,t] = scale * (x[m] . G[b,h,t] + c[b,h,t]),  G[b,h,t,:] = k_ip[b,t,64h..] . W_eff[64h.., :],  c = k_ip . bias_q
// and per row m (token batch b = (m / Nq) / kv_div) and head h
//   p = softmax_t<T s[m,h,:],  a = bf16(sum_t bf16(p_t) v_ip[b,t,64h..] / l),
//   O[m, 64h..] = bf16(float(O) + (layer_scale * row_scale[m / Nq]) * float(a)).
//
// One workgroup of 4 waves takes 64 rows and every head, each wave 16 rows; where that gives fewer workgroups than
// CUs (8192 rows, the 16^2 level of a 16-frame CFG pair: 128) it takes 32 rows, and wave w has the 16 rows of block
// w & 1 and the heads of half w >> 1 (SPLIT = 2; the same arithmetic per row and head, so the same bits).  S^T = G x^T
// on v_mfma_f32_16x16x32_bf16: G streams through
// the LDS in 64-deep k-chunks ([head][16 keys][64] bf16, 2 KiB per head, double-buffered, the K-tile swizzle k_off),
// each wave's 16 x rows come straight from global memory as B fragments (lane (q, g) holds x[q][32 kk + 8 g ..]), and
// a lane ends with the 4 keys 4 g .. 4 g + 3 of query q per head: the softmax needs two lane swaps (group_max) and P
// is already the B operand of O^T = V^T P^T (mfma_f32_16x16x16bf16_1k, V through ds_read_tr).  The transposed read
// picks the channels so that lane (q, g) holds channels 16 g .. 16 g + 15 of the head: 32 contiguous bytes of O.
// Rows t >= T of G are not loaded (zeros), their scores are selected to -inf, and their V rows are stored as zeros, so
// nothing they hold reaches the result.  A tile that spans token batches runs once per batch; a row takes the pass of
// its own batch.  No atomics, no workspace; a row's bits depend on its own x row, G, c and V only.
#include <math.h>

#include "attn_common.h"

namespace vst {

constexpr int kIpNT = 256;       // threads: 4 waves = 4 / SPLIT blocks of 16 rows x SPLIT parts of the heads
constexpr int kIpRows = 64;      // rows of a workgroup, over SPLIT
constexpr int kIpCUs = 256;      // fewer 64-row tiles than this: 32-row tiles, the heads split over the wave pairs
constexpr int kIpMaxHeads = 20;  // LDS plan: 3 x 2 KiB per head (two G chunks, V) = 120 KiB at 20 heads
constexpr int kIpHeadLds = 2048;

struct IpArgs {
  const bf16_t* x;
  const bf16_t* G;
  const bf16_t* V;
  const float* gbias;
  const float* row_scale;
  bf16_t* O;
  int ldx, ldg, ldv, ldo, K, M, Nq, heads, T, kv_div;
  float sl2, layer_scale;
  uint32_t x_bytes, g_bytes, v_bytes, o_bytes;
};

template <int NH, int SPLIT>
__global__ __launch_bounds__(kIpNT) void ip_attention_add_kernel(const IpArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int GBUF = NH * kIpHeadLds;              // one G chunk
  constexpr int NPIECE = (NH * 128 + kIpNT - 1) / kIpNT;  // 16-byte pieces of a chunk per thread
  constexpr int HW = (NH + SPLIT - 1) / SPLIT;            // heads of a wave
  constexpr int ROWS = kIpRows / SPLIT, RB = 4 / SPLIT;   // rows of the workgroup, 16-row blocks
  // heads per group of the O read-modify-write (10 heads per wave: groups of 2 keep the 64-row instance at two
  // waves per SIMD)
  constexpr int HG = HW == 10 ? 2 : (HW % 5 ? HW : 5), NG = HW / HG;
  static_assert(NG * HG == HW, "head groups");
  char* const Vs = smem + 2 * GBUF;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, fr = lane & 15, fq = lane >> 4;
  const int m0 = blockIdx.x * ROWS;
  const int mend = min(m0 + ROWS, p.M) - 1;  // last row of the tile
  const int f_lo = m0 / p.Nq, f_hi = mend / p.Nq;

  // a tile whose frames all have scale 0 writes nothing: leave before reading anything else
  if (p.row_scale) {
    int live = 0;
    for (int f = f_lo + tid; f <= f_hi; f += kIpNT) live |= (p.layer_scale * p.row_scale[f] != 0.0f);
    if (!__syncthreads_or(live)) return;
  } else if (p.layer_scale == 0.0f) {
    return;
  }

  const auto rx = make_rsrc(p.x, p.x_bytes), rg = make_rsrc(p.G, p.g_bytes), rv = make_rsrc(p.V, p.v_bytes);
  const auto ro = make_rsrc(p.O, p.o_bytes);
  const int m = m0 + (wave % RB) * 16 + fr;  // this lane's query row (all four lane groups of a column share it)
  const int h0 = (wave / RB) * HW;           // this wave's heads: h0 .. h0 + HW - 1, those below p.heads
  const bool row_ok = m < p.M;
  const int frame = row_ok ? m / p.Nq : 0;
  const int my_b = frame / p.kv_div;
  const float sc = row_ok ? p.layer_scale * (p.row_scale ? p.row_scale[frame] : 1.0f) : 0.0f;
  const int xoff = row_ok ? (m * p.ldx + fq * 8) * 2 : kOOB;  // (byte offsets fit 31 bits: checked by the entry point)
  const int nk = p.K / 64;

  // this thread's pieces of a G chunk: piece = (head, key t, 16-byte chunk c of the 128-byte row)
  int g_src[NPIECE], g_dst[NPIECE];
#pragma unroll
  for (int i = 0; i < NPIECE; ++i) {
    const int pc = tid + i * kIpNT, h = pc >> 7, t = (pc >> 3) & 15, c = pc & 7;
    const bool on = h < p.heads && t < p.T;
    g_src[i] = on ? ((h * 16 + t) * p.ldg + c * 8) * 2 : kOOB;  // + batch and chunk offsets below
    g_dst[i] = h < NH ? h * kIpHeadLds + k_off(t, c) : -1;
  }

  const int b_lo = f_lo / p.kv_div, b_hi = f_hi / p.kv_div;
  for (int b = b_lo; b <= b_hi; ++b) {
    if (b != b_lo) __syncthreads();  // the previous pass has read its last G chunk and V
    const int gb = b * p.heads * 16 * p.ldg * 2;
    // V of the batch: [head][16 t][64] bf16, rows t >= T zero
    for (int pc = tid; pc < p.heads * 128; pc += kIpNT) {
      const int h = pc >> 7, t = (pc >> 3) & 15, c = pc & 7;
      u32x4 v = buf_load16(rv, t < p.T ? ((b * 16 + t) * p.ldv + h * 64 + c * 8) * 2 : kOOB);
      if (t >= p.T) v = u32x4{0u, 0u, 0u, 0u};
      *reinterpret_cast<u32x4*>(Vs + h * kIpHeadLds + t * 128 + c * 16) = v;
    }
    u32x4 gst[NPIECE];
#pragma unroll
    for (int i = 0; i < NPIECE; ++i) gst[i] = buf_load16(rg, g_src[i] == kOOB ? kOOB : g_src[i] + gb);
    u32x4 xn[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) xn[kk] = buf_load16(rx, xoff == kOOB ? kOOB : xoff + kk * 64);
#pragma unroll
    for (int i = 0; i < NPIECE; ++i)
      if (g_dst[i] >= 0) *reinterpret_cast<u32x4*>(smem + g_dst[i]) = gst[i];
    __syncthreads();

    // the rows of O this lane updates, fetched in groups of HG heads: group 0 now, so that the k-loop hides it, group
    // g + 1 while group g is worked on (a load behind the previous head's store would wait for it every time)
    const bool mine = row_ok && my_b == b && sc != 0.0f;
    const int obase = (m * p.ldo + fq * 16) * 2;
    auto o_off = [&](int hl) { return mine && h0 + hl < p.heads ? obase + (h0 + hl) * 128 : kOOB; };
    u32x4 ocur[HG][2];
    auto load_group0 = [&]() {
#pragma unroll
      for (int hh = 0; hh < HG; ++hh) {
        ocur[hh][0] = buf_load16(ro, o_off(hh));
        ocur[hh][1] = buf_load16(ro, o_off(hh) == kOOB ? kOOB : o_off(hh) + 16);
      }
    };
    load_group0();

    f32x4 s[HW];
#pragma unroll
    for (int hl = 0; hl < HW; ++hl) s[hl] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kc = 0; kc < nk; ++kc) {
      const char* Gs = smem + (kc & 1) * GBUF;
      bf16x8 xf[2];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) xf[kk] = __builtin_bit_cast(bf16x8, xn[kk]);
      const bool more = kc + 1 < nk;
      const int knext = (kc + 1) * 128;  // byte offset of the next k-chunk in a row
#pragma unroll
      for (int i = 0; i < NPIECE; ++i)
        gst[i] = buf_load16(rg, (more && g_src[i] != kOOB) ? g_src[i] + gb + knext : kOOB);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
        xn[kk] = buf_load16(rx, (more && xoff != kOOB) ? xoff + knext + kk * 64 : kOOB);
#pragma unroll
      for (int hl = 0; hl < HW; ++hl) {
        if (h0 + hl < p.heads) {
          const char* gh = Gs + (h0 + hl) * kIpHeadLds;
          const bf16x8 g0 = *reinterpret_cast<const bf16x8*>(gh + k_off(fr, fq));
          const bf16x8 g1 = *reinterpret_cast<const bf16x8*>(gh + k_off(fr, 4 + fq));
          s[hl] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(g0, xf[0], s[hl], 0, 0, 0);
          s[hl] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(g1, xf[1], s[hl], 0, 0, 0);
        }
      }
      if (more) {
        char* Gn = smem + ((kc + 1) & 1) * GBUF;  // last read in iteration kc - 1: the barrier below closed that
#pragma unroll
        for (int i = 0; i < NPIECE; ++i)
          if (g_dst[i] >= 0) *reinterpret_cast<u32x4*>(Gn + g_dst[i]) = gst[i];
      }
      __syncthreads();
    }

    // softmax over the T keys and O^T = V^T P^T per head; lane (q = fr, g = fq) holds keys 4 g .. 4 g + 3 of query q
#pragma unroll
    for (int hg = 0; hg < NG; ++hg) {
      u32x4 onext[HG][2];
      if (hg + 1 < NG) {
#pragma unroll
        for (int hh = 0; hh < HG; ++hh) {
          const int off = o_off((hg + 1) * HG + hh);
          onext[hh][0] = buf_load16(ro, off);
          onext[hh][1] = buf_load16(ro, off == kOOB ? kOOB : off + 16);
        }
      }
#pragma unroll
      for (int hh = 0; hh < HG; ++hh) {
        const int hl = hg * HG + hh, h = h0 + hl;
        if (h < p.heads) {  // (wave-uniform: ds_read_tr below runs with every lane on)
          f32x4 sv = s[hl];
          if (p.gbias) sv += *reinterpret_cast<const f32x4*>(p.gbias + ((size_t)b * p.heads + h) * 16 + fq * 4);
          float mx = -INFINITY;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            if (fq * 4 + i >= p.T) sv[i] = -INFINITY;
            mx = fmaxf(mx, sv[i]);
          }
          mx = group_max(mx);
          const float mb = mx * p.sl2;
          float l = 0.f;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            sv[i] = fast_exp2(sv[i] * p.sl2 - mb);
            l += sv[i];
          }
          l += __shfl_xor(l, 16);
          l += __shfl_xor(l, 32);
          const float inv = 1.0f / l;
          const u32x2 pw{pack2bf(sv[0], sv[1]), pack2bf(sv[2], sv[3])};
          const s16x4 p4 = __builtin_bit_cast(s16x4, pw);
          // V^T block db: MFMA row r is channel 16 (r >> 2) + 4 db + (r & 3), so this lane's result registers of
          // the four blocks are channels 16 g + 4 db + i: 16 contiguous channels
          const char* vh = Vs + h * kIpHeadLds + (fq * 4 + (fr >> 2)) * 128 + (fr & 3) * 32;
          f32x4 o[4];
#pragma unroll
          for (int db = 0; db < 4; ++db) {
            const s16x4 vf = ds_read_tr(vh + db * 8);
            o[db] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(vf, p4, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
          }
          const int off = o_off(hl);  // out of range for the rows of another batch, of a frame with scale 0, past M
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            float cur[8], res[8];
            unpack8(ocur[hh][j], cur);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float a = round_bf(o[2 * j + (e >> 2)][e & 3] * inv);  // the reference's bf16 SDPA output
              res[e] = __fadd_rn(cur[e], __fmul_rn(sc, a));
            }
            __builtin_amdgcn_raw_buffer_store_b128(pack8(res), ro, off == kOOB ? kOOB : off + j * 16, 0, 0);
          }
        }
      }
      if (hg + 1 < NG) {
#pragma unroll
        for (int hh = 0; hh < HG; ++hh) {
          ocur[hh][0] = onext[hh][0];
          ocur[hh][1] = onext[hh][1];
        }
      }
    }
  }
}

template <int NH, int SPLIT>
static int ip_launch_split(const IpArgs& a, hipStream_t st) {
  constexpr int lds = 3 * NH * kIpHeadLds, rows = kIpRows / SPLIT;
  static const bool attr = hipFuncSetAttribute((const void*)ip_attention_add_kernel<NH, SPLIT>,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess;
  if (!attr) return VST_ERR_LAUNCH;
  hipLaunchKernelGGL((ip_attention_add_kernel<NH, SPLIT>), dim3((unsigned)((a.M + rows - 1) / rows)), dim3(kIpNT), lds,
                     st, a);
  return launch_status();
}

template <int NH>
static int ip_launch(const IpArgs& a, hipStream_t st) {
  // (a function of M alone, and both forms give a row the same bits; more than 10 heads per wave would park
  // accumulators in AGPR copies, so 20 heads always split)
  if constexpr (NH > 10) return ip_launch_split<NH, 2>(a, st);
  else return (a.M + kIpRows - 1) / kIpRows < kIpCUs ? ip_launch_split<NH, 2>(a, st) : ip_launch_split<NH, 1>(a, st);
}

}  // namespace vst

using namespace vst;

extern "C" int vst_ip_attention_add(const void* x, int ldx, int K, const void* G, int ldg, const float* gbias,
                                    const void* V, int ldv, int nbatch, int M, int Nq, int heads, int T, int kv_div,
                                    float scale, float layer_scale, const float* row_scale, void* O, int ldo,
                                    void* stream) {
  if (!x || !G || !V || !O) return VST_ERR_ARG;
  if (K <= 0 || nbatch <= 0 || M <= 0 || Nq <= 0 || heads <= 0 || T <= 0 || kv_div <= 0) return VST_ERR_ARG;
  if (T > 16 || K % 64 || M % Nq || (M / Nq - 1) / kv_div >= nbatch) return VST_ERR_ARG;
  const long long inner = 64LL * heads;
  if (ldx < K || ldg < K || ldv < inner || ldo < inner || ldx % 8 || ldg % 8 || ldv % 8 || ldo % 8) return VST_ERR_ARG;
  if (((uintptr_t)x | (uintptr_t)G | (uintptr_t)V | (uintptr_t)O | (uintptr_t)gbias) & 15) return VST_ERR_ARG;
  if ((uintptr_t)row_scale & 3) return VST_ERR_ARG;
  Fit31 fit;
  IpArgs a;
  a.x_bytes = fit(((size_t)(M - 1) * ldx + K) * sizeof(bf16_t));
  a.g_bytes = fit((((size_t)nbatch * heads * 16 - 1) * ldg + K) * sizeof(bf16_t));
  a.v_bytes = fit((((size_t)nbatch * 16 - 1) * ldv + inner) * sizeof(bf16_t));
  a.o_bytes = fit(((size_t)(M - 1) * ldo + inner) * sizeof(bf16_t));
  if (fit.over) return VST_ERR_ARG;  // past the kernel's 31-bit offsets
  if (heads > kIpMaxHeads) return VST_ERR_UNSUPPORTED;
  a.x = (const bf16_t*)x; a.G = (const bf16_t*)G; a.V = (const bf16_t*)V; a.gbias = gbias; a.row_scale = row_scale;
  a.O = (bf16_t*)O;
  a.ldx = ldx; a.ldg = ldg; a.ldv = ldv; a.ldo = ldo; a.K = K; a.M = M; a.Nq = Nq; a.heads = heads; a.T = T;
  a.kv_div = kv_div; a.sl2 = scale * kLog2e; a.layer_scale = layer_scale;
  hipStream_t st = (hipStream_t)stream;
  if (heads <= 2) return ip_launch<2>(a, st);
  if (heads <= 5) return ip_launch<5>(a, st);
  if (heads <= 10) return ip_launch<10>(a, st);
  return ip_launch<20>(a, st);
}
