// Shared by every GEMM / 3x3-conv kernel (gemm.hip, gemm_big.hip, gemm_p8.hip through gemm_plan.h and
// gemm_epilogue.h): the argument block, the 128-byte-row LDS swizzle and the implicit-GEMM conv geometry.
//
// Operands.  C[M, N] = epilogue(A[M, K] . W[N, K]^T), bf16 in, fp32 accumulate.  W is nn.Linear layout ([out, in], K
// contiguous), so both operands are K-contiguous and an MFMA fragment is one 16-byte LDS read.
//   dense A: rows of A1 for k < K1 and of A2 after (K1 a multiple of 64).  The split carries channel concatenation
//     without a copy, and the UnZipLoRA low-rank delta as extra K columns: [x | x.Acat^T] . [W | s.(B (.) m)]^T =
//     x W^T + s.Delta(x) (unziplora_linear_layer.py:298-346).
//   conv A: implicit-GEMM 3x3 conv over NHWC activations (per-frame SDXL conv, diffusers ResnetBlock2D /
//     Downsample2D / Upsample2D): K = (ky, kx, ci), zero padding through out-of-range buffer loads, stride 1 / 2,
//     fused nearest-2x upsample, two-source channel concat (up-block skip connections); conv_row / conv_tap_pixel.
//     The upsample conv also as four 2x2 convs on folded weights (K = (a, b, ci), 4/9 of the work): conv_row_folded.
// The epilogues and their rounding points: gemm_epilogue.h.
#pragma once
#include "vst_common.h"

namespace vst {

struct GemmArgs {
  const bf16_t* A1; const bf16_t* A2;
  int lda1, lda2, K1;
  // conv geometry: input NHWC [nimg, H, W, C1 (+C2)] -> output [nimg, OH, OW, N]
  int H, W, C1, C2, OH, OW, stride, up;
  int pad0;  // 1: no top/left padding (F.pad (0,1,0,1) + stride-2 conv of diffusers Downsample2D(padding=0))
  const bf16_t* Wt; int ldw;
  int M, N, K;
  const float* bias;
  const float* rbias; int rbias_div, ldrb;
  const bf16_t* R; int ldr;
  bf16_t* C; int ldc;
  float* ws;  // split-K slabs [splits][M][N] fp32
  int splits;
  int act;     // EPI 0 only: 1 = GELU(erf) after the bias (TemporalTransformerBlock ffn, no residual / row bias)
  int persist;  // > 0: persistent launch over `persist` CUs (VST_GEMM_PERSIST; 0 = one workgroup per tile)
  int group_m;  // grouped tile order: row panels per group (0 = default 8; VST_GEMM_GROUP_M for tuning)
  int ablate;  // diagnostics only (VST_GEMM_ABLATE): bit0 skip loop DMA, bit1 skip MFMA
  // byte extents of A1 / A2 / W / R for the buffer descriptors; 16-byte aligned so that one scalar load fetches the four
  alignas(16) uint32_t a1_bytes;
  uint32_t a2_bytes, w_bytes, r_bytes;
  // in-GEMM LoRA down-projection (gemm_p8.hip LORA, vst_gemm_lora): Acat [la_p][K] bf16 (row stride lda_la); the
  // output columns of group g = n / la_gn use u columns [g la_gr, (g + 1) la_gr), whose up-projection sits in W's
  // columns K + that range (ldw >= K + la_p); wtail_bytes covers those columns
  const bf16_t* la;
  int lda_la, la_p, la_gn, la_gr;
  uint32_t la_bytes, wtail_bytes;
  // row gate on u (gemm_p8.hip GATE, vst_gemm_lora_gated): gate [ceil(M / gate_div)][ld_gate] fp32, ld_gate >= la_p and a
  // multiple of 4, 16-byte aligned; row m's u column c is scaled by gate[m / gate_div][c].  NULL: no gate
  const float* gate;
  int ld_gate, gate_div;
  // cross-attention epilogue (gemm_p8.hip EPI 4, vst_gemm_cross_attention): the GEMM output is the q of a
  // BasicTransformerBlock's attn2; instead of storing it, each tile writes softmax(q K^T scale) V of its heads over
  // the xa_nk text keys of text batch (m / xa_nq) / xa_kvdiv (K/V rows [batch * xa_nk + key], row stride xa_ldkv)
  const bf16_t* xa_k;
  const bf16_t* xa_v;
  int xa_ldkv, xa_nk, xa_nq, xa_kvdiv;
  float xa_scale_log2;
  uint32_t xa_kv_bytes;
  // temporal attention epilogue (gemm_p8.hip EPI 5, vst_gemm_temporal_attention): frames per clip 16, head dim ta_d
  // (40: two heads per 256-column tile, 80: one); ta_hw pixels per frame; the output O [M, ta_heads * ta_d]
  // (p.C / p.ldc) is written in (clip, frame, pixel) rows
  int ta_hw, ta_heads, ta_d;
  float ta_scale_log2;
  // folded upsample conv (up == 2, conv_row_folded below): rows per output-parity class, live (nimg * H * W) and padded
  // to the tallest tile (M = 4 * up_rows); lda1 is then the input's pixel stride.  Last members: no other field moves
  int up_live, up_rows;
};

__device__ __forceinline__ int swz(int row, int chunk) {
  return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4);
}

// 3x3 conv geometry, one copy for every implicit-GEMM A loader.  Output row m -> (img, oy, ox); img = -1 past M.
__device__ __forceinline__ void conv_row(const GemmArgs& p, const int m, int& img, int& oy, int& ox) {
  if (m < p.M) {
    const int hw = p.OH * p.OW;
    img = m / hw;
    const int rem = m - img * hw;
    oy = rem / p.OW;
    ox = rem - oy * p.OW;
  } else {
    img = -1; oy = ox = 0;
  }
}

// px = the input pixel (img * H + iy) * W + ix that tap (ky, kx) of output pixel (img, oy, ox) reads; false where
// the tap falls into the padding or img < 0 (px is then not to be used: the caller loads out of range, i.e. zeros).
// up: nearest-2x upsample first; pad0: no top / left padding.
__device__ __forceinline__ bool conv_tap_pixel(const GemmArgs& p, const int img, const int oy, const int ox,
                                               const int ky, const int kx, int& px, const bool live = true) {
  int iy, ix;
  bool ok = live && img >= 0;
  if (p.up) {
    const int uy = oy + ky - 1, ux = ox + kx - 1;
    ok = ok && uy >= 0 && uy < 2 * p.H && ux >= 0 && ux < 2 * p.W;
    iy = uy >> 1; ix = ux >> 1;
  } else {
    iy = oy * p.stride + ky - 1 + p.pad0; ix = ox * p.stride + kx - 1 + p.pad0;
    ok = ok && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
  }
  px = (img * p.H + iy) * p.W + ix;
  return ok;
}

// Folded nearest-2x upsample conv (up == 2; the loaders and epilogues compile it in by a template flag).  In the
// upsampled image every input pixel appears four times, so the nine taps of an output pixel of parity (py, px) read
// only 2x2 distinct input pixels: the conv is four 2x2 convs, one per parity class c = 2 py + px, on weights summed
// over the coinciding taps (fold_upsample_weight_kernel: Wf [4][Cout][2][2][C]).  K = (tap (a, b), channel) = 4 C.
// GEMM rows are class-major: m = c * up_rows + r, r = (img * H + y) * W + x on the INPUT grid, r < up_live; up_rows is
// up_live rounded up to the tallest tile (kFoldRowAlign), so a tile lies in one class and uses that class's weight
// panel (rows c * N + n of Wf).  Rows of the padding are dead: they load zeros and store nothing.
//   tap (a, b) of class (py, px) reads input pixel (y + py + a - 1, x + px + b - 1), zero outside the image: with
//   uy = 2y + py + ky - 1 the upsampled-image test 0 <= uy < 2H is the same as 0 <= (uy >> 1) < H, and uy >> 1 is
//   y + py + a - 1 for the ky of S(py, a) (S(0,0) = {0}, S(0,1) = {1,2}, S(1,0) = {0,1}, S(1,1) = {2});
//   output row (img * 2H + 2y + py) * 2W + 2x + px.
constexpr int kFoldRowAlign = 256;

// m -> (img, oy, ox) = (img, y + py, x + px): tap (a, b) then reads (oy + a - 1, ox + b - 1); img = -1 for a dead row
__device__ __forceinline__ void conv_row_folded(const GemmArgs& p, const int m, int& img, int& oy, int& ox) {
  const int cls = m / p.up_rows, r = m - cls * p.up_rows;
  const int hw = p.H * p.W;
  const int im = r / hw, rem = r - im * hw;
  const int y = rem / p.W;
  img = (r < p.up_live && m < p.M) ? im : -1;
  oy = y + (cls >> 1);
  ox = rem - y * p.W + (cls & 1);
}

__device__ __forceinline__ bool conv_tap_pixel_folded(const GemmArgs& p, const int img, const int oy, const int ox,
                                                      const int a, const int b, int& px) {
  const int iy = oy + a - 1, ix = ox + b - 1;
  px = (img * p.H + iy) * p.W + ix;
  return img >= 0 && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
}

// GEMM row m -> row of the [nimg, 2H, 2W] output; -1 for a dead row
__device__ __forceinline__ int conv_out_row_folded(const GemmArgs& p, const int m) {
  const int cls = m / p.up_rows, r = m - cls * p.up_rows;
  if (r >= p.up_live) return -1;
  const int hw = p.H * p.W;
  const int img = r / hw, rem = r - img * hw;
  const int y = rem / p.W, x = rem - y * p.W;
  return (img * 2 * p.H + 2 * y + (cls >> 1)) * 2 * p.W + 2 * x + (cls & 1);
}

}  // namespace vst
