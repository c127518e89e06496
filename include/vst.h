/*
 * vst.h — C ABI of libvst_hip.so, the MI355X (gfx950) kernels behind the AnimateDiff-XL +
 * UnZipLoRA denoising path of tanmud/video_style_transfer.
 *
 * The reference is pure Python/PyTorch; its "FFI" for this path is the set of torch ops its
 * plug-in classes call.  Each entry point below replaces one of those call sites (cited as
 * reference file:line).  Conventions:
 *   - all tensors are device pointers (bf16 unless stated), caller-owned; no allocation inside
 *     except none at all — workspaces are caller-provided (see *_workspace_bytes);
 *   - activations are token-major NHWC: row = (frame * H*W + pixel), C contiguous;
 *   - `stream` is a hipStream_t; every call is asynchronous on it and graph-capturable;
 *   - return 0 (VST_OK) on success, 1 for a bad argument, 2 for a launch failure, 3 for a
 *     supported-shape refusal (vst_gemm_lora, vst_gemm_cross_attention).
 *
 * View contract (tests/test_view_contract_gpu.py holds every entry point to it):
 *   - a matrix operand that comes with a row stride (lda, ldw, ldr, ldc, ldq, ldkv, ldo, ldx, ldy, ...) may be
 *     any row-major view: the stride is in ELEMENTS, at least the row width and a multiple of 8 (ld_row_bias and
 *     vst_gemm_tn's ldc: a multiple of 4); the columns between the width and the stride belong to the
 *     caller and are neither read into a result nor written;
 *   - the base pointer of every bf16 operand is 16-byte aligned (the loaders and epilogues move 16-byte chunks),
 *     and so are fp32 vectors read as float4 (bias, row_bias, gamma, beta, pe, lse).  Bases at smaller offsets
 *     are outside the contract; only vst_gemm_tn checks its output pointer (8 bytes) and refuses;
 *   - operands WITHOUT a row stride in their signature are contiguous: conv inputs x1 / x2 ([nimg*H*W][C]) and
 *     conv weights ([Cout][9*(C1+C2)], rows padded to 8), bias / gamma / beta / pe / table, lse and
 *     GroupNorm partials, every workspace, vst_permute_rows / vst_silu / vst_add / vst_quick_gelu operands,
 *     vst_gemm_f32out's C, vst_colsum's y, the dgamma / dbeta vectors, the fp32 NCHW / latent tensors;
 *   - an output is written exactly on [rows) x [cols) of its view and nowhere else: no guard row or column is
 *     touched, and every element of the view is written by every call.
 *
 * This header is the one declaration of the ABI: every csrc/ file sees it through vst_common.h (a definition that
 * disagrees with its prototype does not compile), and _lib.py derives its ctypes signatures from the prototypes
 * below, so keep them plain C: one prototype per statement, scalar types int / unsigned / float / size_t.
 * vst_p8_trace_read exists only in -DVST_P8_TRACE builds; it stays outside this header and tools/p8_trace.py types it.
 */
#ifndef VST_H
#define VST_H
#include <stddef.h>
#include <stdint.h>

#define VST_OK 0
#define VST_ERR_ARG 1
#define VST_ERR_LAUNCH 2
#define VST_ERR_UNSUPPORTED 3

#ifdef __cplusplus
extern "C" {
#endif

/* Dense projection C = A.W^T (+bias) (+row_bias[m/div]) (+R), fp32 accumulate.
 * A2 != NULL splits A along K: columns [0,K1) from A, [K1,K) from A2 (K1 % 64 == 0).
 * With A2 = x.Acat^T and W = [W_base | s.(B (.) merger)] this is the fused base + UnZipLoRA
 * projection: replaces LoRACompatibleLinear.forward (unziplora_unet/lora_linear.py:74-81) +
 * UnZipLoRALinearLayerInfer.forward (unziplora_unet/unziplora_linear_layer.py:298-346), and
 * TemporalLoRALinear.forward (animatediff/temporal_lora.py:29-32).
 * epilogue 0: plain; 1: GEGLU (diffusers GEGLU feed-forward, unziplora_unet/unzip_attention.py
 * ff path) with hidden/gate rows interleaved per 32-column block ([32 h | 32 g] per 64 rows), output width N/2; 2: GELU(erf) after
 * the bias, no residual / row bias (TemporalTransformerBlock.ffn, animatediff/temporal_transformer.py:53-59). */
int vst_gemm(const void* A, int lda, const void* A2, int lda2, int K1, const void* W, int ldw, int M, int N, int K,
             const float* bias, const float* row_bias, int row_bias_div, int ld_row_bias, const void* R, int ldr,
             void* C, int ldc, int epilogue, void* stream);
/* Same, with the tile (0 auto, 1 = 128x128, 2 = 128x64, 3 = 256x256, 4 = 256x128, 5 = skinny N <= 64
 * without epilogue: the UnZipLoRA down-projection) and split-K (0 auto, >= 1 forced) choice and a
 * caller-owned fp32 workspace for split-K slabs (NULL / too small disables split-K).  An A / A2 / R / C
 * whose byte extent passes 2^31 - 1 (the kernels' 32-bit buffer offsets) is run as equal row chunks, each row
 * with the bits of one launch. */
int vst_gemm_ex(const void* A, int lda, const void* A2, int lda2, int K1, const void* W, int ldw, int M, int N, int K,
                const float* bias, const float* row_bias, int row_bias_div, int ld_row_bias, const void* R, int ldr,
                void* C, int ldc, int epilogue, int tile, int splits, void* workspace, size_t ws_bytes,
                void* stream);
size_t vst_gemm_workspace_bytes(int M, int N, int K);

/* Fused base + LoRA projection with the LoRA down-projection computed INSIDE the GEMM:
 *   C = [x | bf16(x.Acat^T)] . W^T (+bias) (+R),  W = [W_base | V] of width ldw >= K + P,
 * where Acat [P][K] (row stride ld_acat, zero rows past the real rank) holds the stacked down
 * factors (UnZipLoRA: [A_c; A_s]) and V's column block [g*group_r, (g+1)*group_r) carries the up
 * factors (s.(B (.) merger)) of the output columns n with n / group_n == g (q/k/v stacked: group_n =
 * C, group_r = 2r).  The 8-phase kernel accumulates u = x.Acat^T from the x tiles it already
 * streams, rounds it to bf16 (the reference's rounding point of the down output) and adds u.V^T
 * as one extra k-step: no separate pass over x (replaces the down half of
 * UnZipLoRALinearLayerInfer.forward, unziplora_unet/unziplora_linear_layer.py:298-346, inside
 * LoRACompatibleLinear.forward, unziplora_unet/lora_linear.py:74-81).  Returns 3
 * (VST_ERR_UNSUPPORTED) when the shape is not on the 8-phase kernel or a tile would need u columns
 * outside one 16-aligned block; vst_gemm_lora_supported answers that without a launch (0, or the
 * tile width 256 / 192 / 320 it uses; 320-wide tiles are 128 rows high). */
int vst_gemm_lora(const void* x, int ldx, const void* Acat, int ld_acat, int P, int group_n, int group_r,
                  const void* W, int ldw, int M, int N, int K, const float* bias, const void* R, int ldr,
                  void* C, int ldc, void* stream);
int vst_gemm_lora_supported(int M, int N, int K, int P, int group_n, int group_r);
/* vst_gemm_lora with a per-row gate on the down-projection (per-frame content / style strength):
 *   C = [x | u'] . W^T (+bias) (+R),  u = bf16(x.Acat^T),  u'[m][c] = bf16(gate[m / gate_div][c] * float(u[m][c])),
 * gate: fp32 [ceil(M / gate_div)][ld_gate], ld_gate >= P and a multiple of 4, base 16-byte aligned; any finite
 * value (1 = identity, 0 removes the column's term exactly).  The gate multiplies the already rounded u (fp32
 * product, round-to-nearest-even), so the result is that of vst_lora_gate on an explicit u followed by the
 * K-augmented GEMM.  Same kernel, tile choice and refusals as vst_gemm_lora (vst_gemm_lora_supported answers for
 * both: the gate does not change the path); returns 1 (VST_ERR_ARG) before any launch for a NULL or misaligned
 * gate, gate_div <= 0, ld_gate < P or ld_gate % 4 != 0. */
int vst_gemm_lora_gated(const void* x, int ldx, const void* Acat, int ld_acat, int P, int group_n, int group_r,
                        const void* W, int ldw, int M, int N, int K, const float* bias, const void* R, int ldr,
                        void* C, int ldc, const float* gate, int ld_gate, int gate_div, void* stream);
/* The row gate on an explicit down-projection (the paths that keep u as a tensor: vst_layernorm_lora's u, the
 * separate x.Acat^T pass before the K-augmented vst_gemm_ex):
 *   y[m][c] = bf16(gate[m / gate_div][c] * float(u[m][c])),  c < P,
 * u, y: bf16 [M][P] views (row strides ldu, ldy >= P, multiples of 8; P % 8 == 0; y == u allowed); gate as in
 * vst_gemm_lora_gated.  All three bases 16-byte aligned. */
int vst_lora_gate(const void* u, int ldu, int M, int P, const float* gate, int ld_gate, int gate_div, void* y,
                  int ldy, void* stream);
/* Test / A-B knob: force the 8-phase kernel's tile width (256, 192 or 320 where legal; 0 = automatic policy) for
 * every later GEMM of this process; returns the previous setting.  Not on the product path. */
int vst_p8_force_bn(int bn);
/* Test / A-B knob: 3x3 convs whose channel sources are multiples of 64 run on the 8-phase kernel (1) or the ring
 * kernel (0) for every later conv of this process (default: VST_P8_CONV, else 1); returns the previous setting. */
int vst_p8_conv(int on);
/* Test / A-B knob: the 8-phase kernel's persistent grid (one workgroup per CU walking the tiles, each tile's last
 * k-tiles streaming the next tile's first ones) for GEMMs of two or more tile rounds (1) or one workgroup per tile
 * (0), for every later GEMM of this process (default: VST_P8_PERSIST, else 1; not the convs); returns the previous
 * setting.  Same bits. */
int vst_p8_persist(int on);

/* The motion-module attention's q/k/v projection and its frame-axis self-attention as ONE launch:
 *   O[(c, f, p), 40h .. 40h+39] = softmax(q_h[c,.,p] k_h[c,.,p]^T * scale) v_h[c,.,p]  over the 16 frames of pixel p,
 *   [q | k | v] = x . W^T (+ bias) rounded to bf16,
 * x: [nclip * 16 * HW, K] rows (clip, frame, pixel); Wt: the q/k/v weight rows laid out per group of 256 / (3 d)
 * heads (two of 40: [q_2t k_2t v_2t q_2t+1 k_2t+1 v_2t+1]; one of 80: [q_t k_t v_t]) + zero rows up to 256, i.e.
 * [heads / hpt * 256, K] (bias alike, fp32 or NULL).  q/k/v never reach HBM.  Replaces to_q/to_k/to_v +
 * F.scaled_dot_product_attention of the motion modules' AttnProcessor2_0 (diffusers AnimateDiffTransformer3D;
 * animatediff/temporal_transformer.py:40-71) for head_dim 40 / 80 and 16 frames (the 64^2 and 32^2 levels of
 * configs[2]); returns 3 (VST_ERR_UNSUPPORTED) otherwise, _supported answers without a launch. */
int vst_gemm_temporal_attention(const void* x, int ldx, const void* Wt, int ldw, const float* bias, int M, int K,
                                int nclip, int F, int HW, int heads, int head_dim, float scale, void* O, int ldo,
                                void* stream);
int vst_gemm_temporal_attention_supported(int M, int K, int nclip, int F, int HW, int heads, int head_dim);

/* attn2 of a BasicTransformerBlock as ONE launch: the q projection (vst_gemm_lora when Acat != NULL, else
 * [x].[W]^T) with the cross-attention over the text tokens as its epilogue,
 *   O[m, 64h .. 64h+63] = softmax(q_h K_h^T * scale) V_h,  q = bf16(x.W^T (+bias) (+LoRA)),
 * K/V rows [(frame / kv_div) * Nk + key] (frame = m / Nq; nkv_rows rows in all, row stride ldkv, head h at
 * columns 64h).  q never reaches HBM.  Replaces to_q (lora_linear.py:74-81) + F.scaled_dot_product_attention
 * (animatediff/attention_processor.py:78-80) of AnimateDiffAttnProcessor2_0 with encoder_hidden_states.
 * Needs Nq % 256 == 0, Nk <= 80, N % 64 == 0 and the 8-phase kernel's 256x192 tiles for (M, N); returns 3
 * (VST_ERR_UNSUPPORTED) otherwise.  _supported answers without a launch (lora: Acat will be non-NULL). */
int vst_gemm_cross_attention(const void* x, int ldx, const void* Acat, int ld_acat, int P, int group_n, int group_r,
                             const void* W, int ldw, const float* bias, int M, int N, int K, const void* Kt,
                             const void* Vt, int ldkv, int nkv_rows, int Nq, int Nk, int kv_div, float scale, void* O,
                             int ldo, void* stream);
int vst_gemm_cross_attention_supported(int M, int N, int K, int lora, int P, int group_n, int group_r, int Nq,
                                       int Nk);
/* vst_gemm_cross_attention with the row gate of vst_gemm_lora_gated on the q projection's u (Acat must be
 * non-NULL: returns 1 otherwise, as for a bad gate).  The text K/V of a gated model differ per frame (to_k / to_v
 * carry the delta too), so callers pass kv_div = 1 with one K/V block per frame; the kernel does not require it.
 * _supported answers for both entries. */
int vst_gemm_cross_attention_gated(const void* x, int ldx, const void* Acat, int ld_acat, int P, int group_n,
                                   int group_r, const void* W, int ldw, const float* bias, int M, int N, int K,
                                   const void* Kt, const void* Vt, int ldkv, int nkv_rows, int Nq, int Nk, int kv_div,
                                   float scale, void* O, int ldo, const float* gate, int ld_gate, int gate_div,
                                   void* stream);

/* Diagnostics: short name of the kernel (tile shape, epilogue, split-K) that a vst_gemm_ex
 * (kind 0 linear, 1 GEGLU) or vst_conv3x3_ex (kind 2, kind 3 = Cin not a multiple of 64) call with
 * these sizes and policy would launch; kind 4: vst_conv3x3_up_folded, M = its GEMM rows (4 classes of nimg*H*W rows,
 * each padded to a multiple of 256), K = 4 C1.  Used by bench.py to attribute per-launch timings. */
const char* vst_gemm_kernel_name(int M, int N, int K, int kind, int tile, int splits, size_t ws_bytes);

/* 3x3 conv, padding 1, NHWC, optional channel-concat second input, stride 1|2, fused nearest-2x
 * upsample; Wt = [Cout][3][3][C1+C2].  Replaces the per-frame torch conv2d calls of diffusers
 * ResnetBlock2D / Downsample2D / Upsample2D inside UNetMotionModel (called from
 * inference_animatediff.py:110-121); temb add fused as row_bias[frame][Cout]. */
int vst_conv3x3(const void* x1, int C1, const void* x2, int C2, int nimg, int H, int W, int stride, int upsample,
                const void* Wt, int Cout, const float* bias, const float* row_bias, int row_bias_div, const void* R,
                int ldr, void* out, int ldc, void* stream);
/* _ex: + tile / split-K policy and workspace (as vst_gemm_ex) and the row stride of row_bias (0 = Cout), so
 * the time-embedding projections of every ResnetBlock2D can come from ONE batched GEMM output.  Inputs /
 * outputs past 2^31 - 1 bytes run as chunks of whole images (row_bias then must be per image: row_bias_div =
 * OH * OW; VST_ERR_UNSUPPORTED otherwise). */
int vst_conv3x3_ex(const void* x1, int C1, const void* x2, int C2, int nimg, int H, int W, int stride, int upsample,
                   const void* Wt, int Cout, const float* bias, const float* row_bias, int row_bias_div,
                   int ld_row_bias, const void* R, int ldr, void* out, int ldc, int tile, int splits, void* workspace,
                   size_t ws_bytes, void* stream);
/* The nearest-2x upsample conv (diffusers Upsample2D: F.interpolate(scale 2, nearest) + conv 3x3) as four 2x2 convs,
 * one per output parity (py, px), on weights summed over the taps that coincide in the upsampled image: 4/9 of the
 * multiply-adds of vst_conv3x3(upsample = 1).
 * vst_fold_upsample_weight: Wt [Cout][3][3][C] -> Wf [4][Cout][2][2][C] (both contiguous, C % 8 == 0),
 *   Wf[2 py + px][co][a][b][ci] = sum of Wt[co][ky][kx][ci] over ky in S(py, a), kx in S(px, b), with S(0, 0) = {0},
 *   S(0, 1) = {1, 2}, S(1, 0) = {0, 1}, S(1, 1) = {2}; fp32 sums in ascending (ky, kx) order, rounded once to bf16.
 *   The weights are constants of a model: fold once, outside the step.
 * vst_conv3x3_up_folded: x1 [nimg*H*W][C1] (row stride ldx) -> out [nimg, 2H, 2W, Cout] (row stride ldc); Wf as
 *   above with row stride ldwf >= 4 C1 per (class, co); bias fp32 [Cout] or NULL.  Output pixel (2y + py, 2x + px)
 *   takes tap (a, b) from input pixel (y + py + a - 1, x + px + b - 1), zero outside the image.  Needs C1 % 64 == 0
 *   and Cout % 8 == 0; a second source (x2 / C2), row_bias and R are not taken: VST_ERR_UNSUPPORTED for any of these.
 *   Inputs / outputs past 2^31 - 1 bytes run as chunks of whole images; a row's bits do not depend on nimg.  The
 *   result differs from vst_conv3x3(upsample = 1) by the one rounding of the folded weights. */
int vst_fold_upsample_weight(const void* Wt, int Cout, int C, void* Wf, void* stream);
int vst_conv3x3_up_folded(const void* x1, int ldx, int C1, const void* x2, int C2, int nimg, int H, int W,
                          const void* Wf, int ldwf, int Cout, const float* bias, const float* row_bias, const void* R,
                          void* out, int ldc, void* stream);

/* Spatial SDPA, head_dim 64: replaces F.scaled_dot_product_attention in
 * AnimateDiffAttnProcessor2_0.__call__ (animatediff/attention_processor.py:78-80).  K/V row
 * batch = q batch / kv_div (replaces the repeat_interleave of text states, :63-66). */
int vst_spatial_attention(const void* q, int ldq, const void* k, const void* v, int ldkv, void* o, int ldo,
                          int nbatch, int heads, int Nq, int Nk, int kv_div, int head_dim, float scale, float* lse,
                          void* stream);  /* lse: NULL, or fp32 [nbatch*heads*Nq] log2-domain logsumexp (training) */
/* Self-attention over 64+ keys (kv_div 1) on sa_self_kernel (1, default: VST_SA_SELF, else 1) or on the general
 * spatial kernel (0), for every later vst_spatial_attention of this process; returns the previous setting.  Same
 * bits either way (tests / A/B). */
int vst_sa_self(int on);

/* Cross-frame (extended) spatial self-attention, head_dim 64 (no line of the reference does this; the definition is
 * this project's, DESIGN.md "Cross-frame spatial self-attention").  Token (clip b, frame f, pixel p) at row
 * (b*F + f)*N + p.  The keys/values of query frame f are the N tokens of the frames [f, s1(f), s2(f)] of the same
 * clip, in that order, under ONE softmax per head; src >= 0 is that frame, -2 the previous frame max(f - 1, 0), -1
 * none; an entry equal to an earlier entry of the list is dropped.  Arithmetic and rounding points are
 * vst_spatial_attention's self-attention (every frame of the list walked in 64-key tiles of its own).  Returns 1
 * before any launch for head_dim != 64, a stride that is no multiple of 8, a NULL pointer, src >= F or < -2,
 * src1 == -1 with src2 != -1, two equal sources, or byte extents past 2^31 - 1.  No workspace, no atomics, no lse. */
int vst_spatial_attention_frames(const void* q, int ldq, const void* k, const void* v, int ldkv, void* o, int ldo,
                                 int nclip, int F, int heads, int N, int src1, int src2, int head_dim, float scale,
                                 void* stream);

/* StyleAligned AdaIN of q/k(/v) to the anchor frame, ahead of vst_spatial_attention_frames (no line of the reference
 * does this; the definition is this project's, DESIGN.md §18, after Hertz et al., "Style Aligned Image Generation via
 * Shared Attention", CVPR 2024).  x: bf16 view, rows (b*F + f)*N + p, columns [0, C), modified in place.  Per clip b,
 * frame f and column c, in fp32 from the bf16 values:
 *   mu[b,f,c] = mean over the N tokens;  sd[b,f,c] = sqrt(sum (x - mu)^2 / (N - 1) + eps)  (unbiased, as torch.var);
 *   x[b,f,p,c] = bf16((x[b,f,p,c] - mu[b,f,c]) * (sd[b,anchor,c] / sd[b,f,c]) + mu[b,anchor,c])  for f != anchor.
 * The rows of frame `anchor` of every clip are not written.  A constant column has sd = sqrt(eps) and becomes
 * mu[b,anchor,c].  stats: caller-owned fp32 [nclip * F][2][C] (per frame its mean row, then its sd row), 16-byte
 * aligned, written for every frame, the anchor included; it is the hand-over between the two launches (statistics,
 * apply; F == 1: statistics only, x untouched).  No atomics, every sum in an order fixed by (N, C): the same bits on
 * every call, and a clip's bits do not depend on nclip.  C % 8 == 0, ldx >= C, ldx % 8 == 0, x 16-byte aligned.
 * Returns 1 before any launch on a NULL pointer, a non-positive size, N < 2, anchor outside [0, F), eps negative or
 * not finite, a stride or alignment as above, or byte extents past 2^31 - 1. */
int vst_frame_adain(void* x, int ldx, int nclip, int F, int N, int C, int anchor, float eps, float* stats,
                    void* stream);

/* IP-Adapter image attention, added in place onto the attn2 output O ahead of to_out: replaces
 * to_k_ip / to_v_ip, the second F.scaled_dot_product_attention and `hidden_states + self.scale * ip_hidden_states` of
 * IPAdapterAttnProcessor2_0 (unziplora_unet/unzip_attention_processor.py:1793-1809) without a q tensor.  The image keys
 * are folded into the query projection on the host: per row m (frame m / Nq, token batch b = frame / kv_div), head h,
 *   s[t] = scale * (x[m] . G[(b*heads + h)*16 + t] + gbias[(b*heads + h)*16 + t]),  t < T,
 *   p = softmax(s),  a = bf16(sum_t bf16(p_t) V[b*16 + t][64h ..] / l)  (P unnormalised in bf16, 1/l at the end),
 *   O[m][64h ..] = bf16(float(O) + (layer_scale * row_scale[m / Nq]) * float(a)).
 * x: bf16 [M, K]; G: bf16, 16 rows of K columns per (b, h), row stride ldg; gbias: fp32 [nbatch*heads*16] or NULL;
 * V: bf16, 16 rows of 64*heads columns per b, row stride ldv; row_scale: fp32 [M / Nq] or NULL (= 1); O: bf16
 * [M, 64*heads].  Head size 64, 1 <= T <= 16.  Rows t >= T of G, gbias and V never reach the result, whatever they
 * hold.  A frame whose scale product is exactly 0 is not written at all.  No atomics, no workspace; every sum runs in
 * an order fixed by (K, heads, T), and a row's bits do not depend on M.  Returns 1 before any launch for a NULL
 * required pointer, a non-positive size, T > 16, K % 64, M % Nq, (M/Nq - 1)/kv_div >= nbatch, a stride that is no
 * multiple of 8 or too short, a base that is not 16-byte aligned (row_scale: 4), or byte extents past 2^31 - 1; 3 for
 * more than 20 heads (the kernel's LDS plan). */
int vst_ip_attention_add(const void* x, int ldx, int K, const void* G, int ldg, const float* gbias, const void* V,
                         int ldv, int nbatch, int M, int Nq, int heads, int T, int kv_div, float scale,
                         float layer_scale, const float* row_scale, void* O, int ldo, void* stream);

/* Regional prompts: attn2 over R <= 4 text prompts, blended per query row (no line of the reference does this; the
 * definition is this project's).  Head size 64.  Per query row m (image b = m / Nq), head h:
 *   o_r = softmax(q[m] K_r^T scale) V_r, one softmax per region r over that region's Nk keys, with
 *         vst_spatial_attention's arithmetic and rounding points;
 *   O[m][64h ..] = bf16(sum over r ascending with wts[m][r] != 0 of wts[m][r] * (o_r_unnormalised * (1 / l_r))),
 * the sum in fp32, each product and each add rounded, the result rounded once to bf16.  A row with wts[m][r] == 0
 * takes nothing from region r, whatever its K/V hold (a select, not a multiply); a region whose weight is 0 on every
 * row of a workgroup's 128-query block is not loaded there.  A row whose weights are one-hot carries exactly the bits
 * vst_spatial_attention gives it for that region's K/V; a row whose weights are all 0 is written as 0.
 * q, O: bf16 [nimg*Nq, 64*heads] views; Kt, Vt: bf16 rows ((b / kv_div)*R + r)*Nk + key, head h at columns 64h,
 * one row stride ldkv; wts: fp32 [nimg*Nq][4], the caller's already normalised weights, columns >= R ignored.  Any
 * Nk >= 1, walked in 64-key tiles.  No workspace, no atomics, no lse; a row's bits do not depend on nimg.  Returns 1
 * before any launch for a NULL pointer, a non-positive size, R > 4, nimg % kv_div, a stride below 64*heads or no
 * multiple of 8, a base that is not 16-byte aligned, or byte extents past 2^31 - 1. */
int vst_region_attention(const void* q, int ldq, const void* Kt, const void* Vt, int ldkv, const float* wts, void* O,
                         int ldo, int nimg, int heads, int Nq, int Nk, int R, int kv_div, float scale, void* stream);
/* The kernel's LDS plan for up to 128 keys per region, for every later vst_region_attention of this process: 0 the
 * (region, tile) walk double-buffered through registers, 1 every live region's K/V up front by LDS-DMA, -1 (default:
 * VST_REGION_PLAN, else -1) plan 1 where it needs at most 64 KiB of LDS (R <= 2 at 65 to 128 keys, R <= 4 below), else
 * plan 0, as measured.  Returns the previous setting.  Same bits either way (tests / A/B). */
int vst_region_plan(int plan);

/* Frame-axis attention (motion module / TemporalTransformerBlock, animatediff/temporal_transformer.py:66-68):
 * token (clip b, frame f, pixel p) at row (b*F + f)*HW + p; F <= 32; head_dim in {8,16,32,40,64,80,160}. */
int vst_temporal_attention(const void* q, const void* k, const void* v, int ldqkv, void* o, int ldo, int nclip,
                           int F, int HW, int heads, int head_dim, float scale, void* stream);

/* Frame-axis attention inside sliding windows, for clips longer than the motion modules' trained length (no line of
 * the reference does this: it stops at 32 frames; the definition is this project's, DESIGN.md "Long clips").  Windows of
 * L frames start at 0, S, 2S, ... while they fit, plus one at F - L when the last of those does not end the clip; window
 * position j of the window at s is frame s + j.  Per (clip, pixel, head) and window, q/k/v row j is
 * bf16(float(q/k/v[s + j]) + pos_q/k/v[j]) and the attention over the window's L frames is vst_temporal_attention's;
 * o[f] = sum_s w[f-s] O_s[f-s] / sum_s w[f-s] with w[j] = 1 (weighting 0, flat) or min(j + 1, L - j) (1, pyramid),
 * accumulated in fp32 in ascending window order and rounded to bf16 once.  Rows (b*F + f)*HW + p and the q/k/v/o
 * alignment rules as vst_temporal_attention; pos_*: fp32 [L][>= heads*head_dim] with row stride ldpos (16-byte aligned,
 * ldpos % 4 == 0), all NULL = zeros; F >= L, 1 <= L <= 32, 1 <= S <= L; head_dim a multiple of 8 up to 160.  No
 * workspace, no atomics; every output element is written exactly once. */
int vst_temporal_attention_windowed(const void* q, const void* k, const void* v, int ldqkv, const float* pos_q,
                                    const float* pos_k, const float* pos_v, int ldpos, void* o, int ldo, int nclip,
                                    int F, int HW, int heads, int head_dim, int L, int S, int weighting, float scale,
                                    void* stream);

/* GroupNorm (+SiLU) over NHWC samples of rows_per_sample rows; optional 2-source channel concat. */
size_t vst_groupnorm_workspace_bytes(int nsamples, int rows_per_sample, int groups, int C);
int vst_groupnorm(const void* x1, int ld1, int C1, const void* x2, int ld2, int C2, int nsamples,
                  int rows_per_sample, int groups, float eps, const float* gamma, const float* beta, int silu_act,
                  void* y, int ldy, void* workspace, void* stream);

/* GroupNorm (+SiLU) over NHWC samples of rows_per_sample rows; a frame's statistics depend only on its own rows
 * (the chunking is a function of rows_per_sample, not of how many samples share the launch). */

/* Motion-module GroupNorm (diffusers AnimateDiffTransformer3D norm, built at animatediff/utils.py:31: statistics
 * over every frame of a clip), frame-sharded or not.  vst_groupnorm_frame_partials writes fp32 (sum, sumsq) chunk
 * partials per frame, [nframes][vst_groupnorm_frame_chunks(rows_per_frame)][groups][2]; a frame's partials depend
 * only on that frame.  vst_groupnorm_apply_partials merges the partials of every frame of each clip in one fixed
 * order (fp64) and normalises this rank's rows: `part` is the rank-major all-gather of every rank's partials,
 * [nranks][nclips][frames_local][chunks][groups][2] (nranks = 1: this process holds the whole clip), so a
 * frame-sharded forward gets bit-identical statistics to the unsharded one.  scale_shift: caller-owned fp32
 * [2 * nclips * C], 16-byte aligned. */
int vst_groupnorm_frame_chunks(int rows_per_frame);
int vst_groupnorm_frame_partials(const void* x1, int ld1, int C1, int nframes, int rows_per_frame, int groups,
                                 float* part, void* stream);
int vst_groupnorm_apply_partials(const void* x1, int ld1, int C1, int nclips, int frames_local, int rows_per_frame,
                                 int groups, const float* part, int nranks, float eps, const float* gamma,
                                 const float* beta, int silu_act, void* y, int ldy, float* scale_shift, void* stream);

/* LayerNorm over C (+ sinusoidal PE row pe[(row/pe_div)%pe_mod], temporal_transformer.py:6-27). */
int vst_layernorm(const void* x, int ldx, int C, int rows, const float* gamma, const float* beta, float eps,
                  const float* pe, int pe_div, int pe_mod, void* y, int ldy, void* stream);

/* LayerNorm fused with the UnZipLoRA down-projection of the projections that consume it: y = LN(x) and
 * u = y . A^T (A: [R, C] bf16, R <= 64, R % 16 == 0; C % 32 == 0, C <= 1280), x read once.  Replaces the
 * BasicTransformerBlock norm1/norm2 LayerNorm (unziplora_unet/unzip_attention.py:113-239) followed by the
 * lora_down half of UnZipLoRALinearLayerInfer.forward (unziplora_linear_layer.py:298-346) on q/k/v. */
int vst_layernorm_lora(const void* x, int ldx, int C, int rows, const float* gamma, const float* beta, float eps,
                       const void* A, int R, void* y, int ldy, void* u, int ldu, void* stream);

/* SDXL text encoders (encode_prompt, inference_animatediff.py:16-35 / train_animatediff.py:29-50; transformers
 * CLIPTextModel / CLIPTextModelWithProjection):
 * vst_embed_tokens: CLIPTextEmbeddings, y[r] = token_embedding[ids[r]] + position_embedding[r % L] (ids int32, in
 *   range: checked by the caller; y fp32, the towers' residual stream);
 * vst_residual_layernorm: the encoder layer's residual add in fp32 (h_out = h + y, y bf16 or NULL) fused with the
 *   next LayerNorm (n = LN(h_out), bf16): the reference's fp32 text towers under bf16 autocast keep the residual
 *   stream fp32 (CLIPEncoderLayer, layer_norm1/2 and final_layer_norm);
 * vst_causal_attention: CLIPAttention's softmax(q k^T * scale + causal mask) v over N tokens, head_dim 64;
 * vst_quick_gelu: the CLIP ViT-L/14 MLP activation x * sigmoid(1.702 x). */
int vst_embed_tokens(const int* ids, int rows, int L, const void* tok, const void* pos, int C, float* y, int ldy,
                     void* stream);
int vst_residual_layernorm(const float* h, int ldh, const void* y, int ldy, int rows, int C, const float* gamma,
                           const float* beta, float eps, float* h_out, int ldho, void* n, int ldn, void* stream);
int vst_causal_attention(const void* q, int ldq, const void* k, const void* v, int ldkv, void* o, int ldo, int nbatch,
                         int heads, int N, int head_dim, float scale, void* stream);
int vst_quick_gelu(const void* x, void* y, size_t n, void* stream);

/* Row-block permutation: rows of C bf16 indexed (i0,i1,i2,i3) over dims (d0..d3) in src; dst
 * axis k is src axis p_k.  Used for the frame-shard <-> pixel-shard exchange around the motion
 * module's frame-axis attention (the reference's (B*F,HW,C) <-> (B*HW,F,C) permutes of
 * AnimateDiffTransformer3D, here across ranks). */
int vst_permute_rows(const void* src, void* dst, int C, int d0, int d1, int d2, int d3, int p0, int p1, int p2,
                     int p3, void* stream);

/* y[row] = x[row] + table[(row / div) % mod] (fp32 table [mod][C]): the reference TemporalTransformer's
 * PositionalEncoding.forward (animatediff/temporal_transformer.py:20-27) on token rows (b*F + f)*HW + p. */
int vst_add_row_table(const void* x, int ldx, int C, int rows, const float* table, int div, int mod, void* y, int ldy,
                      void* stream);
/* bf16 token rows ((b*F + f)*HW + p, C) -> fp32 (B, C, F, HW): the 5-D output layout of
 * TemporalTransformer.forward (temporal_transformer.py:142-144) and UNetMotionModel.forward. */
int vst_unpack_tokens(const void* src, int B, int C, int F, int HW, float* out, void* stream);

/* Denoise-loop glue (inference_animatediff.py:104-131). */
int vst_timestep_embedding(const float* t, const int* step_idx, int n, int dim, int flip_sin_to_cos,
                           float downscale_freq_shift, void* out, int ld, int col0, int per_row, void* stream);
int vst_pack_latents(const float* lat, int B, int Cl, int F, int HW, const float* sigmas, const int* step_idx,
                     float fixed_scale, int ncopy, void* out, void* stream);
/* vst_euler_cfg_step: lat += (sigmas[s+1] - sigmas[s]) * eps_hat in place, eps_hat = u + g (c - u) (ncopy 1: the only
 *   row), s = *step_idx read on the device; lat fp32 (B, Cl, F, HW), noise bf16 rows ((k*B + b)*F + f)*HW + p of Cl
 *   channels, k = 0 uncond, k = 1 cond.  Returns 1 before any launch on a NULL pointer, a non-positive size or an
 *   ncopy other than 1 or 2.  With vst_euler_cfg_step_masked and vst_sampler_step it is one kernel (csrc/sampler.hip);
 *   the keep-mask blend those two add is described once, below. */
int vst_euler_cfg_step(const void* noise, int ncopy, float guidance, float* lat, int B, int Cl, int F, int HW,
                       const float* sigmas, const int* step_idx, void* stream);
int vst_step_advance(int* step_idx, int num_steps, void* stream);  // wraps to 0 at num_steps
int vst_silu(const void* x, void* y, size_t n, void* stream);
int vst_add(const void* a, const void* b, void* y, size_t n, void* stream);
int vst_copy2d(const void* x, int ldx, void* y, int ldy, int rows, int cols, void* stream);
/* bf16 transpose y[c][r] = x[r][c] (x: rows x cols, row stride ldx; y: cols x rows, row stride ldy).  Backward-pass
 * operand layout for dW = dY^T X and the temporal-LoRA factor gradients (no reference counterpart: torch.autograd
 * of train_animatediff.py:265-319 does it implicitly). */
int vst_transpose(const void* x, int ldx, int rows, int cols, void* y, int ldy, void* stream);

/* Training path (torch.autograd of train_animatediff.py:265-319 in the reference).
 * vst_layernorm_bwd: dx and (dgamma, dbeta) of BasicTransformerBlock LayerNorm (x, g = dL/dy: rows x C bf16), stats
 * recomputed; workspace of vst_layernorm_bwd_workspace_bytes(C, rows); dgamma = dbeta = NULL (frozen affine):
 * dx only, no workspace.  vst_geglu_bwd: dp of the GEGLU projection output p (32-interleaved [h | gate] blocks,
 * as the fused GEMM stores them) from g = dL/d(h * gelu(gate)) (M x Nh). */
size_t vst_layernorm_bwd_workspace_bytes(int C, int rows);
int vst_layernorm_bwd(const void* x, int ldx, const void* g, int ldg, int C, int rows, const float* gamma, float eps,
                      void* dx, int lddx, float* dgamma, float* dbeta, void* workspace, void* stream);
/* vst_groupnorm_bwd: dx, dgamma, dbeta of vst_groupnorm (single source, optional fused SiLU; statistics and the
 * affine recomputed); workspace of vst_groupnorm_bwd_workspace_bytes. */
size_t vst_groupnorm_bwd_workspace_bytes(int nsamples, int rows_per_sample, int groups, int C);
int vst_groupnorm_bwd(const void* x, int ldx, const void* g, int ldg, int C, int nsamples, int rows_per_sample,
                      int groups, float eps, const float* gamma, const float* beta, int silu_act, void* dx, int lddx,
                      float* dgamma, float* dbeta, void* workspace, void* stream);
/* vst_spatial_attention_bwd: gradients of vst_spatial_attention (head_dim 64; K/V shared by kv_div consecutive
 * batches, as for the per-clip text states) from dO, the forward output o and the forward's lse output (flash-
 * attention backward on MFMA, deterministic): dq (lddq), dk/dv (lddkv, one row per kv token: the gradient of text
 * K/V summed over the frames sharing it; both NULL when K/V are frozen, which skips that pass).  Replaces the
 * autograd backward of F.scaled_dot_product_attention (animatediff/attention_processor.py:78-80) that
 * accelerator.backward runs (train_animatediff.py:314).  Workspace: vst_spatial_attention_bwd_workspace_bytes. */
size_t vst_spatial_attention_bwd_workspace_bytes(int nbatch, int heads, int Nq, int Nk);
int vst_spatial_attention_bwd(const void* q, int ldq, const void* k, const void* v, int ldkv, const void* o, int ldo,
                              const void* dout, int lddo, const float* lse, void* dq, int lddq, void* dk, void* dv,
                              int lddkv, int nbatch, int heads, int Nq, int Nk, int kv_div, int head_dim, float scale,
                              void* workspace, void* stream);
/* Sampler data gradients (NHWC tokens, C % 8 == 0): vst_zero_insert writes x [nimg, h, w, C] onto the even
 * positions of a caller-zeroed [nimg, 2h, 2w, C] (Downsample2D stride-2 conv dgrad); vst_sumpool2x2 sums 2x2 blocks
 * of x [nimg, 2h, 2w, C] into y [nimg, h, w, C] (adjoint of Upsample2D's nearest-2x). */
int vst_zero_insert(const void* x, int nimg, int h, int w, int C, void* y, void* stream);
int vst_sumpool2x2(const void* x, int nimg, int h, int w, int C, void* y, void* stream);
/* vst_temporal_attention_bwd: gradients of vst_temporal_attention (same token layout and q/k/v views) from dO; dq/dk/dv
 * are written with row stride lddqkv (e.g. column views of one [tokens, 3C] buffer).  F <= 32, head_dim one of
 * 8/16/32/40/64/80/160 (the forward's set; SDXL motion modules: 40/80/160), MFMA tiles as the forward. */
int vst_temporal_attention_bwd(const void* q, const void* k, const void* v, int ldqkv, const void* dout, int lddo,
                               void* dq, void* dk, void* dv, int lddqkv, int nclip, int F, int HW, int heads,
                               int head_dim, float scale, void* stream);
int vst_geglu_bwd(const void* p, int ldp, const void* g, int ldg, int M, int Nh, void* dp, int lddp, void* stream);
/* vst_colsum: y[N] (fp32) = column sums of the bf16 [M, N] view x (the bias gradients db = g^T 1 of the trainable
 * linears / GEGLU projections; torch's g.float().sum(0) in autograd's Linear backward), N % 8 == 0.  Deterministic
 * two-pass reduction through a workspace of vst_colsum_workspace_bytes(M, N) bytes (no atomics, no memset). */
size_t vst_colsum_workspace_bytes(int M, int N);
int vst_colsum(const void* x, int ldx, int M, int N, float* y, void* workspace, void* stream);

/* ---- SDXL VAE (diffusers AutoencoderKL, fp32 in the reference: inference_animatediff.py:164-169) decode of the
 * denoised clip (inference_animatediff.py:137-144) and encode of training frames (train_animatediff.py:219-224),
 * SURVEY §8(f) rank 4.  Convs, GroupNorm(+SiLU) and the 1x1 projections reuse the entries above. */
/* vst_conv3x3_down_pad0: diffusers Downsample2D(padding=0) of DownEncoderBlock2D = F.pad(x, (0,1,0,1)) then a 3x3
 * stride-2 conv without padding.  Output [nimg, (H-2)/2+1, (W-2)/2+1, Cout], row stride ldc. */
int vst_conv3x3_down_pad0(const void* x, int C, int nimg, int H, int W, const void* Wt, int Cout, const float* bias,
                          void* out, int ldc, void* workspace, size_t ws_bytes, void* stream);
/* C[N][K] (bf16, row stride ldc) = A^T B with A [M][N] and B [M][K] row-major over M tokens: the training step's
 * weight gradients (dW = g^T x, dA = s v^T x, dB = s g^T u; autograd.py, the backward of train_animatediff.py:265-319)
 * without transposed copies of either operand.  fp32 accumulation; the token range splits over workgroups and the
 * fp32 partials (workspace of vst_gemm_tn_workspace_bytes, may be 0) are summed in a fixed order.  N, K, lda, ldb
 * multiples of 8. */
size_t vst_gemm_tn_workspace_bytes(int M, int N, int K);
int vst_gemm_tn(const void* A, int lda, const void* B, int ldb, int M, int N, int K, void* C, int ldc,
                void* workspace, size_t ws_bytes, void* stream);
/* vst_gemm_f32out: C[M][N] = A[M][K] . W[N][K]^T left in fp32 (row stride N).  The mid-block attention's scores
 * (one head of dim 512 over the latent's h*w tokens) feed vst_softmax_rows unrounded, as the fp32 reference's do. */
int vst_gemm_f32out(const void* A, int lda, const void* W, int ldw, int M, int N, int K, float* C, void* stream);
/* vst_softmax_rows: P[r][j] = softmax_j(scale * S[r][j]) (fp32 math, bf16 out) -- diffusers Attention.get_attention_scores
 * + softmax of the VAE mid-block (AttnProcessor2_0's SDPA math, scale = head_dim^-0.5). */
int vst_softmax_rows(const float* S, int lds, int rows, int n, float scale, void* P, int ldp, void* stream);
/* Layout at the fp32 NCHW tensor boundary of vae.decode / vae.encode:
 * vst_nchw_to_nhwc: dst[(i*HW+p)*ldd + c] = bf16(src[(i*C+c)*HW+p] * mul), channels C..ldd-1 zero-filled
 *   (decode input: latents / scaling_factor, inference_animatediff.py:137; encode input: frames in [-1, 1]);
 * vst_nhwc_to_nchw: bf16 NHWC (row stride ld) -> fp32 NCHW (DecoderOutput.sample);
 * vst_frames_to_u8: (x / 2 + 0.5).clamp(0, 1) * 255 truncated to uint8, HWC per frame (inference_animatediff.py:141-143);
 * vst_vae_sample: DiagonalGaussianDistribution(moments).sample() * mul (train_animatediff.py:222-223): moments NHWC
 *   [n*HW][ld] bf16 (mean = ch 0-3, logvar = ch 4-7 clamped to [-30, 20]), eps fp32 NCHW (null: the mode), out fp32
 *   NCHW (n, 4, HW). */
int vst_nchw_to_nhwc(const float* src, int n, int C, int HW, float mul, void* dst, int ldd, void* stream);
int vst_nhwc_to_nchw(const void* src, int ld, int n, int C, int HW, float* dst, void* stream);
int vst_frames_to_u8(const void* src, int ld, int n, int C, int HW, void* dst, void* stream);
int vst_vae_sample(const void* moments, int ld, int n, int HW, const float* eps, float mul, float* out, void* stream);

/* ---- Video-to-video: entering the denoise loop part-way from an encoded source clip (SDEdit / img2img strength)
 * with an optional per-pixel keep mask (latent inpainting for a 4-channel UNet).  No reference counterpart (its loop
 * starts from noise, inference_animatediff.py:88-95); the definitions are DESIGN.md §13, after the diffusers img2img /
 * inpaint pipelines.  Every entry returns 1 before any launch on a NULL pointer or a non-positive size; the step is
 * read on the device and must index the sigma table (the caller's counter, kept in range by vst_step_advance).
 * vst_noise_latents: lat[i] = z0[i] + sigmas[*step_idx] * eps[i] over n fp32 elements (the start latents).
 * The keep-mask blend (vst_euler_cfg_step_masked, and vst_sampler_step with a mask), in fp32 after the step's own
 *   update lat': lat = m * lat' + (1 - m) * (z0 + sigmas[s+1] * eps), with z0 / eps fp32 of lat's shape, mask fp32
 *   (mask_clips, F, HW) in [0, 1] broadcast over channels (1 = free, 0 = keep the source), mask_clips 1 or B.
 *   m == 1 stores exactly the unmasked step's bits; m == 0 at sigmas[s+1] == 0 stores z0's.
 * vst_euler_cfg_step_masked: vst_euler_cfg_step's update, then the blend.
 * vst_u8_to_frames: uint8 frames (n, HW, C) -> bf16 rows [n*HW][ldd] = (v / 255 - 0.5) / 0.5 in fp32
 *   (video_dataset.py:117-118), channels C..ldd-1 zero-filled: the encoder's input, the inverse boundary of
 *   vst_frames_to_u8. */
int vst_noise_latents(const float* z0, const float* eps, const float* sigmas, const int* step_idx, float* lat,
                      size_t n, void* stream);
int vst_euler_cfg_step_masked(const void* noise, int ncopy, float guidance, float* lat, int B, int Cl, int F, int HW,
                              const float* sigmas, const int* step_idx, const float* z0, const float* eps,
                              const float* mask, int mask_clips, void* stream);
int vst_u8_to_frames(const void* src, int n, int C, int HW, void* dst, int ldd, void* stream);

/* ---- Few-step sampling: table-driven sampler step and guidance rescale.
 * vst_sampler_step: one fused launch for every sampler that steps on the denoised estimate D = x - sigma * eps_hat:
 *   e = u + g (c - u) (ncopy 1: the only row);  e *= factor[b] (factor non-NULL; needs ncopy 2);
 *   D = lat - sigmas[s] e;  lat' = a lat + b D + c hist;  hist = D;
 *   then the keep-mask blend above (mask non-NULL; here a kept pixel is torch's fp32 z0 + sigmas[s+1] eps bit for bit)
 *   with (a, b, c) = coef[3 s ..], s = *step_idx read on the device.  coef for "dpmpp_2m" is DPM-Solver++(2M) as
 *   k-diffusion's sample_dpmpp_2m steps it (scheduler.sampler_coefficients); for "euler" it restates the update of
 *   vst_euler_cfg_step (EulerDiscreteScheduler.step, inference_animatediff.py:121).  hist (fp32, the shape of lat,
 *   never lat itself) is not read where c == 0.  z0 / eps / mask are all given or all NULL; mask_clips 1 or B.
 * vst_cfg_rescale_factor: factor[b] = phi * std(cond_b) / std(e_b) + (1 - phi), e = u + g (c - u), the factor
 *   rescale_noise_cfg multiplies the guided noise by (animatediff/pipeline_animatediff_xl.py:377-379, :414-425); std
 *   over all Cl * F * HW values of clip b, unbiased.  Two launches (per-block (count, mean, M2) partials, a
 *   finalize), Chan merges in an order fixed by the indices, no atomics: the same bits on every call.  factor = 1
 *   where std(e_b) == 0 (the reference gives NaN).  phi in [0, 1]; workspace of
 *   vst_cfg_rescale_factor_workspace_bytes(B, Cl, F, HW) bytes, B the number of clips (noise holds 2 B of them).
 * Every entry returns 1 before any launch on a NULL pointer, a non-positive size or a value outside its range. */
int vst_sampler_step(const void* noise, int ncopy, float guidance, float* lat, float* hist, int B, int Cl, int F,
                     int HW, const float* sigmas, const float* coef, const int* step_idx, const float* factor,
                     const float* z0, const float* eps, const float* mask, int mask_clips, void* stream);
size_t vst_cfg_rescale_factor_workspace_bytes(int B, int Cl, int F, int HW);
int vst_cfg_rescale_factor(const void* noise, float guidance, float phi, int B, int Cl, int F, int HW, float* factor,
                           void* workspace, void* stream);

/* ---- Stochastic samplers: counter-based noise on the device and the sampler step that adds it.  No
 * reference counterpart (its loop is deterministic Euler); the samplers are k-diffusion's Euler ancestral and
 * DPM-Solver++(2M) SDE and diffusers' LCMScheduler.step, as scheduler.sampler_coefficients restates them.
 * The noise has no state.  For the element (clip b, channel c, local frame f, pixel p) of a tensor (B, Cl, F, HW) that
 * holds frames [f0, f0 + F) of clips of F_total frames, with P = ((uint64)b * F_total + f0 + f) * HW + p and
 * s = *step_idx, seed = *seed both read on the device:
 *   x0..x3 = Philox4x32-10(counter (lo32 P, hi32 P, s, stream_id << 16 | c >> 2), key (lo32 seed, hi32 seed));
 *   u_k = ((x_k >> 9) + 0.5) * 2^-23 (exact in fp32, inside (0, 1));
 *   n0 = r0 cospi(2 u1), n1 = r0 sinpi(2 u1), r0 = sqrt(-2 log u0); n2, n3 likewise from (u2, u3);
 *   channel c takes lane c & 3.  So a frame shard, or a replayed graph, draws what the whole eager clip draws.
 *   stream_id 0 is the sampler step's; 1 .. 65535 are free for callers.
 * vst_noise_bits: out[b][c][f][p] = x[c & 3] (the counter layout, exactly checkable against a host Philox).
 * vst_noise_normal: out[b][c][f][p] = n[c & 3], the bits vst_sampler_step_noise adds.
 * vst_sampler_step_noise: vst_sampler_step on coef4 rows (a, b, c, d), with lat' += d xi before the keep-mask blend,
 *   xi the normal above at stream 0: lat' = a lat + b D + c hist + d xi; hist = D; a kept pixel stays
 *   z0 + sigmas[s+1] eps.  Where d == 0 xi is neither generated nor added and lat' has vst_sampler_step's bits on
 *   (a, b, c).  It is one more rule of the one step kernel (csrc/sampler.hip).
 * Every entry returns 1 before any launch on a NULL pointer, a non-positive size, f0 < 0 or f0 + F > F_total, a
 * stream_id outside [0, 65535] or Cl above 2^18 (the last counter word holds both); vst_sampler_step_noise also on
 * what vst_sampler_step refuses. */
int vst_noise_bits(uint32_t* out, const uint64_t* seed, const int* step_idx, int stream_id, int B, int Cl, int F,
                   int F_total, int f0, int HW, void* stream);
int vst_noise_normal(float* out, const uint64_t* seed, const int* step_idx, int stream_id, int B, int Cl, int F,
                     int F_total, int f0, int HW, void* stream);
int vst_sampler_step_noise(const void* noise, int ncopy, float guidance, float* lat, float* hist, int B, int Cl, int F,
                           int F_total, int f0, int HW, const float* sigmas, const float* coef4, const int* step_idx,
                           const uint64_t* seed, const float* factor, const float* z0, const float* eps,
                           const float* mask, int mask_clips, void* stream);

/* ---- FreeU in the up path: diffusers' apply_freeu, which the reference's up blocks call before each
 * skip concatenation of their first two stages (animatediff/unet_block.py:399-417,
 * unziplora_unet/unet_block.py:853-867), as one launch over NHWC bf16 rows [nimg * H * W, C].
 *   x_out[:, :Cx/2] = bf16(float(x) * b), x_out[:, Cx/2:] = x bit for bit;
 *   skip_out = bf16(fourier_filter(float(skip), threshold 1, scale s)) per (image, channel) map, in closed form: with
 *     th = 2 pi h / H, ph = 2 pi w / W and the seven sums m0 = S x, a = S x cos th, b = S x sin th, c = S x cos ph,
 *     d = S x sin ph, e = S x cos(th + ph), f = S x sin(th + ph) over the map,
 *     y = x + (s - 1) / (H W) (m0 + a cos th + b sin th + c cos ph + d sin ph + e cos(th + ph) + f sin(th + ph)),
 *     sums and correction in fp32, one rounding at the store.  s == 1 stores the skip's bits.
 *   (s, b) = table[2 * stage], table[2 * stage + 1]: fp32 [2][2] read on the device, so new values replay a captured
 *   step.  A map's bits depend on that map and on (H, W) only, never on nimg or on the other maps of the batch.
 * x_out may be x itself (same pointer and row stride: the scale runs in place); skip_out may overlap no operand.  Row
 * strides >= channels; bases and strides 16-byte aligned; nothing outside the views is written.
 * Returns 1 before any launch on a NULL pointer, H < 2 or W < 2 (the mask slice of the definition is empty or wraps),
 * Cs % 8, Cx % 16, a stage outside {0, 1}, a stride or alignment as above, or an overlap; 3 for H + W > 4096. */
int vst_freeu(const void* x, int ldx, int Cx, const void* skip, int lds, int Cs, void* x_out, int ldxo,
              void* skip_out, int ldso, int nimg, int H, int W, const float* table, int stage, void* stream);

/* ---- FreeInit's frequency mix: the re-initialisation of the latents between two passes of the denoise
 * loop, after Wu et al., "FreeInit" (ECCV 2024) and diffusers' FreeInitMixin._apply_free_init.  No reference counterpart
 * (its loop runs once).  x, init, noise, out: fp32 (B, Cl, F, H, W) contiguous, the layout of the latents; per (clip,
 * channel) volume, with DFT3 the transform over (F, H, W):
 *   z   = x + init - r          (init NULL: z = x - r)
 *   out = r + Re IDFT3(filt . DFT3(z))
 *   r   = scale * noise[b][c][f][h][w]                        (noise != NULL; seed and iter NULL), or
 *   r   = scale * n, n the normal of vst_noise_normal at (*seed, *iter, stream_id) with HW = H W, F_total = F, f0 = 0
 *                                                             (noise NULL; seed and iter non-NULL, read on the device).
 *   In the second form r is generated in the first launch and again in the last, never stored, and is bit for bit
 *   scale * vst_noise_normal(...) of the same arguments (one fp32 product).
 * filt: fp32 [F][H][W], the low-pass mask in unshifted DFT order, shared by every clip and channel.  It must be
 *   symmetric under k -> -k on every axis (free_init.dft_order makes it so): the operator is then real, equal to the
 *   real part diffusers keeps, and the kernel reads only the bins kw <= W / 2 of the real transform along W.
 * Every axis is a dense DFT in fp32 on an exact (k n) mod N twiddle table, so any size is taken, not only powers of two.
 * Three launches (plane forward, frame axis with the multiply, plane inverse), no atomics, every sum in an order fixed
 * by (F, H, W): the same bits on every call, and a clip's bits do not depend on B.  filt all zeros stores r's bits.
 * workspace: the spectrum between the launches, B * Cl * F * H * (W / 2 + 1) * 8 bytes, 16-byte aligned; ws_bytes at
 *   least that.  Nothing past that many bytes is read or written.
 * out may be x itself (same pointer: in place); otherwise out overlaps no operand, and the workspace overlaps none.
 * Returns 1 before any launch on a NULL x / out / filt / workspace, both or neither of noise and (seed, iter) (seed and
 * iter go together), a non-positive size, a stream_id outside [0, 65535] or Cl above 2^18 (as vst_noise_normal), B * Cl
 * above 65535, a short workspace, a base that is not aligned to its element (workspace: 16 bytes) or a forbidden
 * overlap; 3 for F, H or W above 128. */
int vst_free_init_mix(const float* x, const float* init, const float* noise, float* out, const float* filt,
                      float scale, const uint64_t* seed, const int* iter, int stream_id,
                      int B, int Cl, int F, int H, int W, void* workspace, size_t ws_bytes, void* stream);

/* ---- Token merging for the spatial transformer blocks: Bolya & Hoffman, "Token Merging for Fast Stable
 * Diffusion" (CVPR-W 2023), tomesd's bipartite_soft_matching_random2d with a row layout that depends on no sort order.
 * No reference counterpart.  Tokens of one image are rows p = y*W + x of a bf16 view [nimg * N, C], N = H * W.
 * Destinations and sources.  The image is cut into hc x wc = (H / sy) x (W / sx) whole cells of sy x sx tokens (leftover
 *   rows and columns belong to no cell).  One token per cell, at in-cell offset o(cell), (oy, ox) = (o / sx, o % sx), is a
 *   destination: Nd = hc * wc of them, numbered j in raster order of the cells.  Every other token is a source:
 *   Ns = N - Nd, numbered i in ascending token index.  seed == NULL: o = 0.  Otherwise, both read on the device,
 *     o(cell) = Philox4x32-10(counter (cell, 0, *step_idx, 2 << 16 | layer), key (lo32, hi32 of *seed))[0] % (sy * sx),
 *   stream 2 of the counters of vst_noise_bits.  The image index is no input: every image of a call, and every frame
 *   shard of a clip, draws one pattern.
 * vst_tome_match, per image, on the metric x: s[i][j] = <a_i, b_j> / (|a_i| |b_j|) (bf16 MFMA products with fp32
 *   accumulation; fp32 norms, lane-strided squares then a butterfly, an order fixed by C; a zero row scores 0, and a
 *   non-finite product 0: never NaN); best[i] = max_j s[i][j], node[i] the lowest j that attains it; the r sources with
 *   the largest best (ties: the lower i) are merged into their node.  Outputs: best, fp32 [nimg][Ns], and the plan,
 *   vst_tome_plan_bytes(nimg, N, r) = nimg * (6 N + 4) * 4 bytes of int32, per image at these offsets:
 *     0       slot[N]: the merged row of token p; destination j has row j, the Ns - r kept sources the rows Nd ..
 *             N - r - 1 in ascending token index, a merged source its node's row;
 *     N       dst_tok[Nd], then src_tok[Ns];
 *     2 N     node[Ns] (of every source, merged or not);
 *     3 N     start[Nd + 1], then list[r]: the tokens of the sources merged into destination j, ascending, are
 *             list[start[j] .. start[j + 1]);
 *     4 N + 4 kept_tok[Ns - r]: the token of merged row Nd + k;
 *     5 N + 4 inv[N]: fp32 bits of 1 / |x_p| (0 for a zero row).
 * vst_tome_merge: y [nimg * (N - r), C]; y[m] = bf16(sum / count) over the members of merged row m (the destination
 *   and list[start[m] .. start[m + 1]) for m < Nd), summed in fp32 in ascending token index; a row with one member is
 *   copied bit for bit.
 * vst_tome_unmerge_add: y[p] = bf16(float(res[p]) + float(o[slot[p]])) over [nimg * N, C], o [nimg * (N - r), C];
 *   res == NULL: y[p] = o[slot[p]] bit for bit; y may be res (same pointer and stride).
 * No atomics; every sum in an order fixed by the shapes: the same bits on every call, and an image's plan and rows do
 * not depend on nimg or on the other images.  Guard columns are neither read into a result nor written.  merge and
 * unmerge_add clamp what they read from a plan to the image.
 * Needs N <= 4096, C % 64 == 0, C <= 1280: 3 (VST_ERR_UNSUPPORTED) otherwise, before any launch.  1 before any launch
 * on a NULL pointer, a non-positive size, sy > H or sx > W, r outside [0, Ns], a layer outside [0, 65535], only one of
 * seed and step_idx, a stride below C or no multiple of 8, a bf16 base or plan that is not 16-byte aligned. */
size_t vst_tome_plan_bytes(int nimg, int N, int r);
int vst_tome_match(const void* x, int ldx, int nimg, int H, int W, int C, int sy, int sx, int r, const uint64_t* seed,
                   const int* step_idx, int layer, int* plan, float* best, void* stream);
int vst_tome_merge(const void* x, int ldx, const int* plan, int nimg, int H, int W, int C, int sy, int sx, int r,
                   void* y, int ldy, void* stream);
int vst_tome_unmerge_add(const void* o, int ldo, const int* plan, int nimg, int N, int r, int C, const void* res,
                         int ldr, void* y, int ldy, void* stream);

/* Ceiling probes (no reference counterpart; bench.py's measured peaks next to the vendor figures,
 * SURVEY §8(d)).  vst_probe_mfma: `grid` workgroups x 8 waves, each wave `iters` x 16 independent
 * 16x16x32 bf16 MFMAs (flops = grid*8*iters*16*16384).  vst_probe_hbm_read: streams `bytes` of `src`
 * with 16-B loads.  `out` receives nothing in practice (anti-dead-code sink, >= grid elements). */
int vst_probe_mfma(int grid, int iters, float* out, void* stream);
int vst_probe_hbm_read(const void* src, size_t bytes, int grid, unsigned* out, void* stream);
/* vst_probe_fetch: the per-CU operand fetch rate from an L2-resident `bytes` region (the GEMM loaders' path): `grid`
 * 512-thread workgroups, each wave moving `iters` 1-KiB pieces, 8 in flight; mode 0 buffer loads into VGPRs, 1 LDS-DMA
 * into an LDS ring (the 8-phase GEMM's loader), 2 buffer loads + ds_write_b128 (a register-staged loader). */
int vst_probe_fetch(int mode, const void* src, int bytes, int grid, int iters, unsigned* out, void* stream);
/* vst_probe_mix: what a loader costs an MFMA stream: `grid` 512-thread workgroups, each wave iterating {issue `pieces`
 * (0, 2, 4, 8) one-KiB pieces, 32 register-operand 16x16x32 bf16 MFMAs, land the pieces}; mode 1 LDS-DMA, 2 buffer
 * loads + ds_write_b128.  Time against pieces = 0 is the loader's cost to the matrix core. */
int vst_probe_mix(int mode, int pieces, const void* src, int bytes, int grid, int iters, float* out, void* stream);
const char* vst_version(void);

#ifdef __cplusplus
}
#endif
#endif /* VST_H */
