// Host only: what one GEMM / 3x3-conv call launches (the plan), the runtime knobs of the GEMM dispatch, and the
// launchers that take a plan.  plan_gemm (gemm.hip) is the one place that builds a plan; the launch, the kernel-name
// query, the workspace size and the fp32-output entry point all read the plan it returns.
#pragma once
#include "gemm_common.h"

namespace vst {

enum GemmFamily {
  kNone = 0,  // the request is not legal (VST_ERR_ARG; VST_ERR_UNSUPPORTED for a column-statistics conv)
  kRows,      // gemm_rows_kernel, M <= 8
  kSkinny,    // gemm_skinny_kernel, N <= 64, no epilogue
  kGather,    // conv_gather_kernel: scalar-gather conv (channels not a multiple of 64)
  kRing,      // gemm_ring_kernel (gemm_big.hip); conv: its implicit-GEMM A loader
  kP8,        // gemm_p8_kernel (gemm_p8.hip)
  kP8Conv,    // gemm_p8_kernel, implicit-GEMM 3x3 conv
};

struct GemmPlan {
  int family;    // GemmFamily
  int bm, bn;    // tile (ring / 8-phase families)
  int splits;    // > 1: ring split-K slabs + gemm_splitk_reduce_kernel
  int epi;       // 0 bias / row bias / residual, 1 GEGLU, 2 fp32 slab (vst_gemm_f32out), 3 bias + GELU
  bool conv;     // 3x3 conv (A loader of the ring / 8-phase kernel)
  bool persist;  // 8-phase: the persistent grid (p8_persist_applies)
  bool fold;     // conv: the folded nearest-2x upsample conv (vst_conv3x3_up_folded; GemmArgs::up == 2)
};

// Every runtime switch of the GEMM dispatch (DESIGN.md §9 lists them), read once per process; vst_p8_force_bn,
// vst_p8_conv and vst_p8_persist write p8_bn, p8_conv and p8_persist.
struct GemmKnobs {
  int p8;               // VST_GEMM_P8: 0 off, unset (-1) / 1 the automatic choice (p8_auto)
  int p8_bn;            // VST_P8_BN: forced 8-phase tile width (256 / 192 / 320), 0 = the policy
  int p8_320;           // VST_P8_320: 1 lets the policy take 128x320 tiles for plain GEMMs
  int p8_conv;          // VST_P8_CONV: 0 keeps the 3x3 convs on the ring kernel
  int p8_persist;       // VST_P8_PERSIST: 0 one workgroup per tile
  int p8_lora_persist;  // VST_P8_LORA_PERSIST: 0 keeps the in-GEMM LoRA kernels off the persistent grid
  int lora_ingemm;      // VST_LORA_INGEMM: 0 runs the LoRA down-projection as a separate pass
  int xattn_fuse;       // VST_XATTN_FUSE: 0 runs attn2's q projection and text attention as two launches
  int ring_persist;     // VST_GEMM_PERSIST: ring kernel's persistent launch, unset (-1) = GEGLU only
  int group_m;          // VST_GEMM_GROUP_M
  int ablate;           // VST_GEMM_ABLATE (reaches the kernels in the -DVST_P8_TRACE diagnostics build only)
};
GemmKnobs& gemm_knobs();

int device_cus();  // CUs of the current device (256 where it cannot be asked)
inline int p8_cus() {  // the 8-phase persistent grid: whole XCD rounds
  const int n = device_cus();
  return (n < 8 ? 256 : n) & ~7;
}

// gemm_big.hip: the plan's tile, its A loader (conv) and epilogue (the fp32 slab one when it splits)
int launch_gemm_ring(const GemmArgs& a, const GemmPlan& p, hipStream_t s);
// gemm_p8.hip: tile width, epilogue and persist come from the plan; the fused entry points pass theirs
int launch_gemm_p8(const GemmArgs& a, const GemmPlan& p, hipStream_t s);
int launch_gemm_p8_conv(const GemmArgs& a, const GemmPlan& p, hipStream_t s);
int launch_gemm_p8_conv_folded(const GemmArgs& a, const GemmPlan& p, hipStream_t s);
int launch_gemm_p8_lora(const GemmArgs& a, int bn, bool persist, hipStream_t s);
int launch_gemm_p8_tattn(const GemmArgs& a, hipStream_t s);
int launch_gemm_p8_xattn(const GemmArgs& a, hipStream_t s);

}  // namespace vst
