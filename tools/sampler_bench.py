"""Few-step sampling: what the table-driven sampler step and guidance rescale cost.

Kernel: at (1, 4, 16, 64, 64) fp32 latents with a CFG pair, alternating (device events around `iters` back-to-back
calls): vst_sampler_step plain and masked, vst_cfg_rescale_factor (both launches), vst_euler_cfg_step, and the
stochastic samplers' vst_noise_normal and vst_sampler_step_noise (on a d != 0 row of the
DPM-Solver++ 2M SDE table, so the noise is generated).  Median and min..max over the passes.
Step: AnimateDiffDenoiser at the bench workload (16 x 512^2, CFG pair, whole-step HIP graph), three denoisers over one
UNet, all captured up front and replayed alternately, `--steps` replays per pass:
  euler          the default step (the bench.py path: vst_euler_cfg_step), 50-step table
  dpmpp_2m       sampler="dpmpp_2m" on 20 Karras sigmas (vst_sampler_step)
  dpmpp_2m_resc  the same with guidance_rescale 0.7 (vst_cfg_rescale_factor + vst_sampler_step)
  dpmpp_2m_sde   sampler="dpmpp_2m_sde", eta 1, on the same sigmas (vst_sampler_step_noise)
The two stochastic rows are left out when the loaded library does not export their entries (VST_LIB_AB of an older
build, which the other rows are compared against).
A step's time does not depend on the length of its table, so steps/s at 20 against 50 steps follows from it.
Bits (--md5, nothing timed): one JSON line per case with an md5 of lat (and of hist) after one call of each of the
three step entry points on seeded CPU inputs, over shapes x ncopy x step x mask x mask_clips x factor.  Two builds
(VST_LIB_AB, tools/ab_lib.sh) that print the same lines store the same bytes.

  python tools/sampler_bench.py [--out profiles/sampler_<date>.json] [--passes 5] [--steps 4] [--no-step] [--md5]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_style_transfer_amd import _lib, kernels as K  # noqa: E402

BF = torch.bfloat16
FRAMES, SIDE, STEPS, FEW = 16, 512, 50, 20


def has_noise_entries():
    return hasattr(_lib.load(), "vst_sampler_step_noise")


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
    from video_style_transfer_amd.scheduler import EulerDiscreteScheduler, sampler_coefficients
    sch = EulerDiscreteScheduler(sigma_schedule="karras")
    sch.set_timesteps(FEW)
    sig = sch.sigmas.float().to(dev)
    coef = sampler_coefficients(sch.sigmas, "dpmpp_2m").float().to(dev)
    step = torch.full((1,), FEW // 2, dtype=torch.int32, device=dev)  # a second-order row: the history is read
    hw = SIDE // 8
    g = torch.Generator().manual_seed(3)
    shape = (1, 4, FRAMES, hw, hw)
    lat, hist, z0, eps = (torch.randn(shape, generator=g).to(dev) for _ in range(4))
    factor = torch.ones(1, device=dev)
    ws = K.cfg_rescale_workspace(shape, dev)
    noise = torch.randn(2 * FRAMES * hw * hw, 4, generator=g).to(BF).to(dev)
    mask = (torch.rand(1, FRAMES, hw, hw, generator=g) < 0.5).float().to(dev)
    sides = {"euler": lambda: K.euler_cfg_step(noise, lat, sig, step, guidance=7.5, ncopy=2),
             "sampler_step": lambda: K.sampler_step(noise, lat, hist, sig, coef, step, guidance=7.5, ncopy=2),
             "sampler_step_masked": lambda: K.sampler_step(noise, lat, hist, sig, coef, step, guidance=7.5, ncopy=2,
                                                           z0=z0, eps=eps, mask=mask),
             "cfg_rescale_factor": lambda: K.cfg_rescale_factor(noise, shape, guidance=7.5, phi=0.7, out=factor,
                                                                workspace=ws)}
    if has_noise_entries():
        coef4 = sampler_coefficients(sch.sigmas, "dpmpp_2m_sde").float().to(dev)
        seed = torch.full((1,), 42, dtype=torch.int64, device=dev)
        xi = torch.empty(shape, device=dev)
        sides["noise_normal"] = lambda: K.noise_normal(seed, step, shape, out=xi)
        sides["sampler_step_noise"] = lambda: K.sampler_step_noise(noise, lat, hist, sig, coef4, step, seed,
                                                                   guidance=7.5, ncopy=2)
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


MD5_SHAPES = [(2, 4, 3, 5, 7), (2, 5, 3, 5, 7), (1, 4, 16, 64, 64)]


def md5(t):
    return hashlib.md5(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def md5_cases(dev):
    """Every case's inputs come from its own generator, seeded by the case name."""
    from video_style_transfer_amd.scheduler import EulerDiscreteScheduler, sampler_coefficients
    sch = EulerDiscreteScheduler(sigma_schedule="karras")
    sch.set_timesteps(FEW)
    sig = sch.sigmas.float().to(dev)
    coef = sampler_coefficients(sch.sigmas, "dpmpp_2m").float().to(dev)
    for shape in MD5_SHAPES:
        B, Cl, F, H, W = shape
        for ncopy in (1, 2):
            for s in (0, FEW // 2, FEW - 1):
                for kind in (None, "binary", "uniform"):
                    for mc in sorted({1, B}) if kind else (0,):
                        # the plain Euler step takes no mask, the masked one needs one; a factor needs the CFG pair
                        entries = ["euler_masked" if kind else "euler", "sampler"] + ["sampler_factor"] * (ncopy == 2)
                        for entry in entries:
                            name = f"{entry} {shape} ncopy={ncopy} step={s} mask={kind} mask_clips={mc}"
                            g = torch.Generator().manual_seed(int(hashlib.md5(name.encode()).hexdigest()[:8], 16))
                            lat, hist, z0, eps = (torch.randn(shape, generator=g).to(dev) for _ in range(4))
                            noise = torch.randn(ncopy * B * F * H * W, Cl, generator=g).to(BF).to(dev)
                            u = torch.rand(max(mc, 1), F, H, W, generator=g)
                            mask = ((u < 0.5).float() if kind == "binary" else u).to(dev)
                            factor = (0.5 + torch.rand(B, generator=g)).to(dev)
                            step = torch.full((1,), s, dtype=torch.int32, device=dev)
                            kw = dict(guidance=7.5, ncopy=ncopy)
                            mkw = dict(z0=z0, eps=eps, mask=mask) if kind else {}
                            if entry == "euler":
                                K.euler_cfg_step(noise, lat, sig, step, **kw)
                            elif entry == "euler_masked":
                                K.euler_cfg_step_masked(noise, lat, sig, step, z0, eps, mask, **kw)
                            else:
                                K.sampler_step(noise, lat, hist, sig, coef, step, **kw, **mkw,
                                               factor=factor if entry == "sampler_factor" else None)
                            out = {"lat": md5(lat)}
                            if entry.startswith("sampler"):
                                out["hist"] = md5(hist)
                            print(json.dumps({"case": name, "md5": out}), flush=True)


def make_denoiser(unet, dev, **kw):
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser
    from video_style_transfer_amd.scheduler import EulerDiscreteScheduler
    cfg = unet.config
    if kw:
        kw.update(num_inference_steps=FEW, scheduler=EulerDiscreteScheduler(sigma_schedule="karras"))
    else:
        kw = dict(num_inference_steps=STEPS)
    den = AnimateDiffDenoiser(unet, FRAMES, SIDE, SIDE, device=dev, **kw)
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
    ap.add_argument("--md5", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sampler_bench: no HIP device (timings need the GPU)")
    dev = torch.device("cuda")
    if a.md5:
        return md5_cases(dev)
    recs = [kernel_ab(a.passes, a.iters, dev)]
    if not a.no_step:
        from video_style_transfer_amd.utils import build_unet
        unet = build_unet(seed=0, lora_rank=8, device=dev)
        dens = {"euler": make_denoiser(unet, dev), "dpmpp_2m": make_denoiser(unet, dev, sampler="dpmpp_2m"),
                "dpmpp_2m_resc": make_denoiser(unet, dev, sampler="dpmpp_2m", guidance_rescale=0.7)}
        if has_noise_entries():
            dens["dpmpp_2m_sde"] = make_denoiser(unet, dev, sampler="dpmpp_2m_sde")
        for den in dens.values():
            den.init_latents(seed=42)
            den.run_steps(a.warmup)
        t = {s: [] for s in dens}
        for _ in range(a.passes):
            for s, den in dens.items():
                t[s].append(run_ms(den, a.steps))
        for den in dens.values():
            assert torch.isfinite(den.lat).all()
        rec = {"what": "denoise_step", "shape": f"{FRAMES} x {SIDE}^2, CFG pair, whole-step graph; euler on the "
               f"{STEPS}-step table, dpmpp_2m on {FEW} Karras sigmas", "passes": a.passes, "steps_per_pass": a.steps}
        summary(rec, t, "step_ms", 1.0, 2)
        rec["dpmpp_2m_minus_euler_ms"] = round(rec["dpmpp_2m_step_ms"] - rec["euler_step_ms"], 2)
        rec["rescale_minus_dpmpp_2m_ms"] = round(rec["dpmpp_2m_resc_step_ms"] - rec["dpmpp_2m_step_ms"], 2)
        if "dpmpp_2m_sde" in dens:
            rec["sde_minus_dpmpp_2m_ms"] = round(rec["dpmpp_2m_sde_step_ms"] - rec["dpmpp_2m_step_ms"], 2)
        # derived from the step times, not a measured run: frames per second of a whole denoise
        rec["derived_frames_per_s"] = {f"euler_{STEPS}_steps": round(FRAMES / (STEPS * rec["euler_step_ms"] * 1e-3), 3),
                                       f"dpmpp_2m_{FEW}_steps": round(FRAMES / (FEW * rec["dpmpp_2m_step_ms"] * 1e-3), 3)}
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/sampler_bench.py", "device": torch.cuda.get_device_name(0), "records": recs},
                      f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
