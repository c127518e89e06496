// Ceiling probes: the measured counterparts of the vendor peaks bench.py divides by (SURVEY §8(d)
// "use the vendor figures and a measured microbenchmark ceiling; report both").
//
//  * vst_probe_mfma: every wave issues `iters` rounds of 16 independent v_mfma_f32_16x16x32_bf16
//    (16 accumulator chains, so the dependent-issue latency never stalls the pipe), 8 waves per
//    workgroup (2 per SIMD), `grid` workgroups.  flops = grid * 8 * iters * 16 * 16384.
//  * vst_probe_hbm_read: a grid-stride stream of 16-B non-temporal global loads over `bytes` (folded into one
//    word per thread so nothing is dead), 4 loads in flight per thread.
// Neither touches anything outside the caller's buffers; both return 0 / VST_ERR_*.
#include "vst_common.h"

namespace vst {

__global__ __launch_bounds__(512) void probe_mfma_kernel(int iters, float* out) {
  const int lane = threadIdx.x & 63;
  bf16x8 a, b;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    a[i] = (__bf16)(1e-3f * (lane + i));
    b[i] = (__bf16)(1e-3f * (lane - i));
  }
  f32x4 acc[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[j], 0, 0, 0);
  }
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) s += acc[j][0] + acc[j][1] + acc[j][2] + acc[j][3];
  if (s == 1234.5f) out[blockIdx.x] = s;  // never true in practice; keeps the chain alive
}

__global__ __launch_bounds__(256) void probe_hbm_read_kernel(const void* src, size_t bytes, unsigned* out) {
  const size_t nchunk = bytes / 16;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const u32x4* p = reinterpret_cast<const u32x4*>(src);
  u32x4 x = {0u, 0u, 0u, 0u};
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * stride < nchunk; i += 4 * stride) {
    const u32x4 v0 = __builtin_nontemporal_load(p + i);
    const u32x4 v1 = __builtin_nontemporal_load(p + i + stride);
    const u32x4 v2 = __builtin_nontemporal_load(p + i + 2 * stride);
    const u32x4 v3 = __builtin_nontemporal_load(p + i + 3 * stride);
    x ^= v0 ^ v1 ^ v2 ^ v3;
  }
  for (; i < nchunk; i += stride) x ^= p[i];
  const unsigned r = x[0] ^ x[1] ^ x[2] ^ x[3];
  if (r == 0x9e3779b9u) out[blockIdx.x] = r;  // data-dependent, practically never taken
}

// Per-CU operand fetch rate from an L2-resident region (the GEMMs' operand path): one 512-thread
// workgroup per CU, every wave moving 1 KiB pieces (16 B per lane) of a `bytes` region that stays in each XCD's L2,
// `iters` pieces per wave, up to 8 in flight per wave:
//   MODE 0: buffer_load_dwordx4 into VGPRs (folded into one word per lane);
//   MODE 1: LDS-DMA (buffer_load ... lds) into a 64 KiB LDS ring, as the 8-phase GEMM's loader issues them;
//   MODE 2: buffer_load_dwordx4 into VGPRs, then ds_write_b128 into the same ring (register-staged loader).
template <int MODE>
__global__ __launch_bounds__(512) void probe_fetch_kernel(const void* src, int bytes, int iters, unsigned* out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const auto r = make_rsrc(src, (uint32_t)bytes);
  const int npieces = bytes >> 10;
  int piece = (blockIdx.x * 8 + wid) * 97 % npieces;
  u32x4 x = {0u, 0u, 0u, 0u};
  char* ring = smem + wid * 8192;  // 8 KiB (8 pieces) per wave
  for (int it = 0; it < iters; it += 8) {
    if constexpr (MODE == 0) {
      u32x4 v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = buf_load16(r, ((piece + j) % npieces) * 1024 + lane * 16);
#pragma unroll
      for (int j = 0; j < 8; ++j) x ^= v[j];
    } else if constexpr (MODE == 1) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(
            r, (__attribute__((address_space(3))) void*)((__attribute__((address_space(3))) char*)(uintptr_t)(ring + j * 1024)),
            16, ((piece + j) % npieces) * 1024 + lane * 16, 0, 0, 0);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
      u32x4 v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = buf_load16(r, ((piece + j) % npieces) * 1024 + lane * 16);
#pragma unroll
      for (int j = 0; j < 8; ++j) *reinterpret_cast<u32x4*>(ring + j * 1024 + lane * 16) = v[j];
      // read one piece back (another lane's chunk) so the stores are live, as a consumer's fragment read would be
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      x ^= *reinterpret_cast<const u32x4*>(ring + (it & 7) * 1024 + (lane ^ 1) * 16);
    }
    piece = (piece + 8 * 61) % npieces;
  }
  if constexpr (MODE != 0) {
    __syncthreads();
    x = *reinterpret_cast<const u32x4*>(smem + threadIdx.x * 16);
  }
  const unsigned rr = x[0] ^ x[1] ^ x[2] ^ x[3];
  if (rr == 0x9e3779b9u) out[blockIdx.x] = rr;  // data-dependent, practically never taken
}

// What a loader costs an MFMA stream: one 512-thread workgroup per CU (2 waves per SIMD, as the 8-phase
// GEMM), every wave iterating {issue P one-KiB pieces, 32 independent-chain v_mfma_f32_16x16x32_bf16 from registers,
// land the pieces} over an L2-resident region:
//   MODE 1: LDS-DMA (buffer_load ... lds), the pieces of iteration i waited for (counted vmcnt) one iteration later;
//   MODE 2: buffer_load into VGPRs for iteration i + 1, ds_write_b128 of iteration i's (landed) registers.
// P = 0 is the MFMA-only baseline; the difference per iteration is the loader's cost to the matrix core.
template <int MODE, int P>
__global__ __launch_bounds__(512) void probe_mix_kernel(const void* src, int bytes, int iters, float* out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const auto r = make_rsrc(src, (uint32_t)bytes);
  const int npieces = bytes >> 10;
  int piece = (blockIdx.x * 8 + wid) * 97 % npieces;
  char* ring = smem + wid * 16384;  // 16 pieces per wave
  bf16x8 fa, fb;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    fa[i] = (__bf16)(1e-3f * (lane + i));
    fb[i] = (__bf16)(1e-3f * (lane - i));
  }
  f32x4 acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  u32x4 cur[P > 0 ? P : 1], nxt[P > 0 ? P : 1];
  if constexpr (MODE == 2 && P > 0) {
#pragma unroll
    for (int j = 0; j < P; ++j) cur[j] = buf_load16(r, ((piece + j) % npieces) * 1024 + lane * 16);
  }
  for (int it = 0; it < iters; ++it) {
    const int slot = (it & 1) * 8;
    piece = (piece + 8 * 61) % npieces;
    if constexpr (MODE == 1 && P > 0) {
#pragma unroll
      for (int j = 0; j < P; ++j)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(
            r, (__attribute__((address_space(3))) void*)((__attribute__((address_space(3))) char*)(uintptr_t)(ring + (slot + j) * 1024)),
            16, ((piece + j) % npieces) * 1024 + lane * 16, 0, 0, 0);
    }
    if constexpr (MODE == 2 && P > 0) {
#pragma unroll
      for (int j = 0; j < P; ++j) nxt[j] = buf_load16(r, ((piece + j) % npieces) * 1024 + lane * 16);
    }
#pragma unroll
    for (int m = 0; m < 32; ++m) acc[m & 7] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, acc[m & 7], 0, 0, 0);
    if constexpr (MODE == 1 && P > 0) {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(P) : "memory");  // the previous iteration's pieces landed
    }
    if constexpr (MODE == 2 && P > 0) {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(P) : "memory");  // cur (issued one iteration ago) landed
#pragma unroll
      for (int j = 0; j < P; ++j) *reinterpret_cast<u32x4*>(ring + (slot + j) * 1024 + lane * 16) = cur[j];
#pragma unroll
      for (int j = 0; j < P; ++j) cur[j] = nxt[j];
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  float sacc = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) sacc += acc[j][0] + acc[j][1] + acc[j][2] + acc[j][3];
  if (P > 0) sacc += __uint_as_float(*reinterpret_cast<const uint32_t*>(ring + lane * 16) & 0x007fffffu);
  if (sacc == 1234.5f) out[blockIdx.x] = sacc;  // never true in practice; keeps everything live
}

}  // namespace vst

extern "C" int vst_probe_mix(int mode, int pieces, const void* src, int bytes, int grid, int iters, float* out,
                             void* stream) {
  if (!src || bytes < 65536 || (bytes & 1023) || grid <= 0 || iters <= 0 || !out) return VST_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
#define VST_MIX(M, P) \
  hipLaunchKernelGGL((vst::probe_mix_kernel<M, P>), dim3(grid), dim3(512), 131072, s, src, bytes, iters, out)
  if (mode == 0 || pieces == 0) VST_MIX(1, 0);
  else if (mode == 1 && pieces == 2) VST_MIX(1, 2);
  else if (mode == 1 && pieces == 4) VST_MIX(1, 4);
  else if (mode == 1 && pieces == 8) VST_MIX(1, 8);
  else if (mode == 2 && pieces == 2) VST_MIX(2, 2);
  else if (mode == 2 && pieces == 4) VST_MIX(2, 4);
  else if (mode == 2 && pieces == 8) VST_MIX(2, 8);
  else return VST_ERR_ARG;
#undef VST_MIX
  return vst::launch_status();
}

extern "C" int vst_probe_fetch(int mode, const void* src, int bytes, int grid, int iters, unsigned* out, void* stream) {
  if (!src || bytes < 65536 || (bytes & 1023) || grid <= 0 || iters <= 0 || (iters & 7) || !out) return VST_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  switch (mode) {
    case 0: hipLaunchKernelGGL(vst::probe_fetch_kernel<0>, dim3(grid), dim3(512), 65536, s, src, bytes, iters, out); break;
    case 1: hipLaunchKernelGGL(vst::probe_fetch_kernel<1>, dim3(grid), dim3(512), 65536, s, src, bytes, iters, out); break;
    case 2: hipLaunchKernelGGL(vst::probe_fetch_kernel<2>, dim3(grid), dim3(512), 65536, s, src, bytes, iters, out); break;
    default: return VST_ERR_ARG;
  }
  return vst::launch_status();
}

extern "C" int vst_probe_mfma(int grid, int iters, float* out, void* stream) {
  if (grid <= 0 || iters <= 0 || !out) return VST_ERR_ARG;
  hipLaunchKernelGGL(vst::probe_mfma_kernel, dim3(grid), dim3(512), 0, (hipStream_t)stream, iters, out);
  return vst::launch_status();
}

extern "C" int vst_probe_hbm_read(const void* src, size_t bytes, int grid, unsigned* out, void* stream) {
  if (!src || bytes < 16 || grid <= 0 || !out) return VST_ERR_ARG;
  hipLaunchKernelGGL(vst::probe_hbm_read_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, bytes, out);
  return vst::launch_status();
}
