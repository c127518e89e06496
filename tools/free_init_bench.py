"""FreeInit's frequency mix: what one mix costs, next to torch.fft on the same GPU and next to one
denoise step.  Report only: there is no earlier figure to hold these against.

Mix: kernels.free_init_mix as the denoiser calls it between two passes (init given, fresh noise from the Philox
counters, default butterworth mask) on fp32 latents (1, 4, 16, 64, 64) (the bench clip, 16 x 512^2) and
(2, 4, 32, 64, 64).  Yardsticks, eager on the same device, alternating with the kernel in every pass:
  fft_pipeline   diffusers' _apply_free_init in fp32: randn, fftn + fftshift of z_T and of the noise, the mix with M,
                 ifftshift, ifftn, real part;
  fft_restated   r + ifftn(fftn(x + init - r) * M~).real with r = scale * noise_normal(...) (the kernel's own form).
Each record also holds the max error of the kernel and of the fp32 torch.fft pipeline (CPU) against the fp64 pipeline
on explicit noise, the figures tests/test_free_init_gpu.py prints for its small shapes.
Step: AnimateDiffDenoiser at the bench workload with the whole-step HIP graph, replayed.

  python tools/free_init_bench.py [--out profiles/free_init_<date>.json] [--passes 5] [--iters 50] [--steps 4] [--no-step]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_style_transfer_amd import kernels as K  # noqa: E402
from video_style_transfer_amd.free_init import FreeInit, dft_order, freq_filter  # noqa: E402

F32 = torch.float32
FRAMES, SIDE, STEPS = 16, 512, 50
SHAPES = [(1, 4, 16, 64, 64), (2, 4, 32, 64, 64)]
SCALE = 14.6146
DIMS = (-3, -2, -1)


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def fft_pipeline(x, init, noise, M, dtype=torch.complex64):
    """diffusers' _apply_free_init: M in fftshift order."""
    zf = torch.fft.fftshift(torch.fft.fftn((x + init).to(dtype), dim=DIMS), dim=DIMS)
    rf = torch.fft.fftshift(torch.fft.fftn(noise.to(dtype), dim=DIMS), dim=DIMS)
    mixed = zf * M + rf * (1 - M)
    return torch.fft.ifftn(torch.fft.ifftshift(mixed, dim=DIMS), dim=DIMS).real


def mix_records(passes, iters, dev):
    recs = []
    for shape in SHAPES:
        g = torch.Generator().manual_seed(sum(shape))
        x, init, eps = torch.randn(shape, generator=g), SCALE * torch.randn(shape, generator=g), \
            torch.randn(shape, generator=g)
        M64 = freq_filter(*shape[2:], FreeInit())
        Mt = dft_order(M64).to(F32).to(dev)
        M = M64.to(F32).to(dev)
        xd, idev, ed = x.to(dev), init.to(dev), eps.to(dev)
        seed = torch.tensor([42], dtype=torch.int64, device=dev)
        it = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = K.free_init_workspace(shape, dev)
        out = torch.empty_like(xd)
        scale32 = float(torch.tensor(SCALE, dtype=F32))

        # errors on explicit noise against the fp64 pipeline (CPU)
        ref = fft_pipeline(x.double(), init.double(), scale32 * eps.double(), M64, torch.complex128)
        e32 = (fft_pipeline(x, init, torch.tensor(scale32) * eps, M64.to(F32)).double() - ref).abs().max().item()
        got = K.free_init_mix(xd, idev, Mt, scale32, noise=ed)
        err = (got.double().cpu() - ref).abs().max().item()

        def kern():
            K.free_init_mix(xd, idev, Mt, scale32, seed=seed, it=it, out=out, workspace=ws)

        def pipe():
            fft_pipeline(xd, idev, scale32 * torch.randn(shape, device=dev), M)

        def restated():
            r = scale32 * K.noise_normal(seed, it, shape, stream_id=1)
            return r + torch.fft.ifftn(torch.fft.fftn(xd + idev - r, dim=DIMS) * Mt, dim=DIMS).real

        sides = {"mix": kern, "fft_pipeline": pipe, "fft_restated": restated}
        for fn in sides.values():
            for _ in range(3):
                fn()
        t = {k: [] for k in sides}
        for _ in range(passes):
            for k, fn in sides.items():
                t[k].append(timed(fn, iters))
        B, Cl, F, H, W = shape
        rec = {"what": "free_init_mix", "shape": list(shape), "launches": 3, "passes": passes, "iters": iters,
               "workspace_bytes": K.free_init_workspace_bytes(shape),
               "dense_flops": 8.0 * B * Cl * F * H * (W // 2 + 1) * (W / 2 + 2 * H + 2 * F),
               "kernel_max_err_vs_fp64": err, "fp32_torch_fft_max_err_vs_fp64": e32}
        for k, v in t.items():
            rec[f"{k}_us"] = round(statistics.median(v) * 1e3, 2)
            rec[f"{k}_us_range"] = [round(min(v) * 1e3, 2), round(max(v) * 1e3, 2)]
        rec["mix_vs_fft_pipeline"] = round(rec["mix_us"] / rec["fft_pipeline_us"], 3)
        rec["mix_vs_fft_restated"] = round(rec["mix_us"] / rec["fft_restated_us"], 3)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    return recs


def step_record(passes, steps, warmup, dev):
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser
    from video_style_transfer_amd.utils import build_unet
    unet = build_unet(seed=0, lora_rank=8, device=dev)
    cfg = unet.config
    den = AnimateDiffDenoiser(unet, FRAMES, SIDE, SIDE, device=dev, num_inference_steps=STEPS)
    g = torch.Generator().manual_seed(5)
    enc = torch.randn(2, 77, cfg.cross_attention_dim, generator=g)
    pooled = torch.randn(2, cfg.text_embed_dim, generator=g)
    den.set_prompt_embeds(enc[1:2], pooled[1:2], enc[0:1], pooled[0:1])
    den.init_latents(seed=42)
    den.run_steps(warmup)
    t = []
    for _ in range(passes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        den.run_steps(steps)
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3 / steps)
    assert torch.isfinite(den.lat).all()
    rec = {"what": "denoise_step", "passes": passes, "steps_per_pass": steps,
           "shape": f"{FRAMES} x {SIDE}^2, CFG pair, whole-step graph, {STEPS}-step Euler",
           "step_ms": round(statistics.median(t), 3), "step_ms_range": [round(min(t), 3), round(max(t), 3)]}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("free_init_bench: no HIP device (timings need the GPU)")
    dev = torch.device("cuda")
    recs = mix_records(a.passes, a.iters, dev)
    if not a.no_step:
        step = step_record(a.passes, a.steps, a.warmup, dev)
        mix = recs[0]
        step["mix_16x64x64_over_step"] = round(mix["mix_us"] / 1e3 / step["step_ms"], 5)
        recs.append(step)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/free_init_bench.py", "device": torch.cuda.get_device_name(0), "records": recs},
                      f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
