"""Video-to-video: what entering the loop from a source clip, and the keep mask, cost per step.

Step: AnimateDiffDenoiser at the bench workload (16 x 512^2, 50 steps, CFG pair, whole-step HIP graph), three
denoisers over one UNet, all captured up front and replayed alternately, `--steps` replays per pass:
  plain        init_latents (the bench.py path: vst_euler_cfg_step)
  source       set_source(strength 0.5), no mask (the same launches as plain; only the start differs)
  source_mask  set_source(strength 0.5, random binary mask) (vst_euler_cfg_step_masked)
Kernel: the two Euler steps (instances of one kernel) alone at that shape, alternating (device events around `iters` back-to-back calls), and
vst_noise_latents.  Median and min..max over the passes.

  python tools/source_clip_bench.py [--out profiles/source_clip_<date>.json] [--passes 5] [--steps 4] [--no-step]
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

BF = torch.bfloat16
FRAMES, SIDE, STEPS = 16, 512, 50


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def summary(rec, t, unit, scale, digits):
    for s, x in t.items():
        rec[f"{s}_{unit}"] = round(statistics.median(x) * scale, digits)
        rec[f"{s}_{unit}_range"] = [round(min(x) * scale, digits), round(max(x) * scale, digits)]


def kernel_ab(passes, iters, dev):
    from video_style_transfer_amd.scheduler import EulerDiscreteScheduler
    sch = EulerDiscreteScheduler()
    sch.set_timesteps(STEPS)
    sig = sch.sigmas.float().to(dev)
    step = torch.full((1,), 25, dtype=torch.int32, device=dev)
    hw = SIDE // 8
    g = torch.Generator().manual_seed(3)
    shape = (1, 4, FRAMES, hw, hw)
    lat, z0, eps = (torch.randn(shape, generator=g).to(dev) for _ in range(3))
    noise = torch.randn(2 * FRAMES * hw * hw, 4, generator=g).to(BF).to(dev)
    mask = (torch.rand(1, FRAMES, hw, hw, generator=g) < 0.5).float().to(dev)
    sides = {"euler": lambda: K.euler_cfg_step(noise, lat, sig, step, guidance=7.5, ncopy=2),
             "euler_masked": lambda: K.euler_cfg_step_masked(noise, lat, sig, step, z0, eps, mask, guidance=7.5,
                                                             ncopy=2),
             "noise_latents": lambda: K.noise_latents(z0, eps, sig, step, out=lat)}
    for fn in sides.values():
        fn(), fn()
    t = {s: [] for s in sides}
    for _ in range(passes):
        for s, fn in sides.items():
            t[s].append(timed(fn, iters))
    rec = {"what": "kernel_ab", "shape": f"(1, 4, {FRAMES}, {hw}, {hw}) fp32 latents, CFG pair", "passes": passes,
           "iters": iters}
    summary(rec, t, "us", 1e3, 2)
    print(json.dumps(rec), flush=True)
    return rec


def make_denoiser(unet, dev):
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser
    cfg = unet.config
    den = AnimateDiffDenoiser(unet, FRAMES, SIDE, SIDE, num_inference_steps=STEPS, device=dev)
    g = torch.Generator().manual_seed(5)
    enc = torch.randn(2, 77, cfg.cross_attention_dim, generator=g)
    pooled = torch.randn(2, cfg.text_embed_dim, generator=g)
    den.set_prompt_embeds(enc[1:2], pooled[1:2], enc[0:1], pooled[0:1])
    return den


def run_ms(den, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    den.run_steps(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("source_clip_bench: no HIP device (timings need the GPU)")
    dev = torch.device("cuda")
    recs = [kernel_ab(a.passes, a.iters, dev)]
    if not a.no_step:
        from video_style_transfer_amd.utils import build_unet
        unet = build_unet(seed=0, lora_rank=8, device=dev)
        hw = SIDE // 8
        g = torch.Generator().manual_seed(6)
        z0 = torch.randn(1, 4, FRAMES, hw, hw, generator=g)
        mask = (torch.rand(1, FRAMES, hw, hw, generator=g) < 0.5).float()
        dens = {s: make_denoiser(unet, dev) for s in ("plain", "source", "source_mask")}
        dens["plain"].init_latents(seed=42)
        dens["source"].set_source(z0, 0.5, seed=42)
        dens["source_mask"].set_source(z0, 0.5, mask, seed=42)
        for den in dens.values():
            den.run_steps(a.warmup)
        t = {s: [] for s in dens}
        for _ in range(a.passes):
            for s, den in dens.items():
                t[s].append(run_ms(den, a.steps))
        for den in dens.values():
            assert torch.isfinite(den.lat).all()
        rec = {"what": "denoise_step", "shape": f"{FRAMES} x {SIDE}^2, {STEPS} steps, CFG pair, whole-step graph",
               "passes": a.passes, "steps_per_pass": a.steps, "strength": 0.5}
        summary(rec, t, "step_ms", 1.0, 2)
        rec["source_minus_plain_ms"] = round(rec["source_step_ms"] - rec["plain_step_ms"], 2)
        rec["mask_minus_source_ms"] = round(rec["source_mask_step_ms"] - rec["source_step_ms"], 2)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/source_clip_bench.py", "device": torch.cuda.get_device_name(0), "records": recs},
                      f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
