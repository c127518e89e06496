"""Per-frame content / style strength: what the row gate on the UnZipLoRA down-projection costs.

Step: AnimateDiffDenoiser at the bench workload (16 x 512^2, 50 steps, CFG pair, whole-step HIP graph), three
denoisers over one UNet, all captured up front and replayed alternately, `--steps` replays per pass:
  plain       no gates (the bench.py path)
  gates_one   set_lora_gates(1, 1): the gated kernels, the plain run's values
  style_ramp  set_lora_gates(style=linspace(0, 1, 16)): unstyled to fully styled over the clip
then one eager step of `plain` and of `style_ramp` under the launch profiler: device-event time per kernel name of the
LoRA projections, the fused cross-attention and vst_lora_gate, i.e. which launches the difference sits in.
Kernel: gated against ungated vst_gemm_lora / vst_gemm_cross_attention at the six fused-LoRA shapes of the step
(bench.py's fused_lora_gemms), alternating (device events around `iters` back-to-back calls), and vst_lora_gate alone.
Median and min..max over the passes.

  python tools/lora_gate_bench.py [--out profiles/lora_gate_<date>.json] [--passes 5] [--steps 4] [--no-step]
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
# (M, N, K, P, group_n, group_r, tokens per frame or 0, name): the step's fused base + UnZipLoRA r=8 projections
SHAPES = [
    (32768, 1920, 640, 64, 640, 16, 0, "32768x1920x704"),        # attn1 q/k/v, 32x32 level
    (32768, 640, 640, 32, 640, 16, 0, "32768x640x672"),          # to_out, 32x32 level (persistent 128x320 grid)
    (32768, 640, 640, 32, 640, 16, 1024, "32768x640x672 xattn"),  # attn2 q + cross-attention
    (8192, 3840, 1280, 64, 1280, 16, 0, "8192x3840x1344"),       # attn1 q/k/v, 16x16 level
    (8192, 1280, 1280, 32, 1280, 16, 0, "8192x1280x1312"),       # to_out, 16x16 level
    (8192, 1280, 1280, 32, 1280, 16, 256, "8192x1280x1312 xattn"),
]


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
    g = torch.Generator().manual_seed(3)
    recs = []
    for M, N, Kd, P, gn, gr, nq, name in SHAPES:
        x = torch.randn(M, Kd, generator=g).to(BF).to(dev)
        a = (torch.randn(P, Kd, generator=g) * Kd ** -0.5).to(BF).to(dev)
        w = (torch.randn(N, Kd + P, generator=g) * Kd ** -0.5).to(BF).to(dev)
        out = torch.empty(M, N, dtype=BF, device=dev)
        div = nq or (1024 if M == 32768 else 256)
        gate = (torch.rand(M // div, P, generator=g) + 0.5).to(dev)
        if nq:
            frames = M // nq
            kv1 = torch.randn(frames * 77, 2 * N, generator=g).to(BF).to(dev)  # gated: one K/V block per frame
            kv2 = kv1[: 2 * 77]                                               # plain: one per CFG branch
            sides = {"plain": lambda: K.linear_cross_attention(x, w, a, gn, gr, None, kv2[:, :N], kv2[:, N:], Nq=nq,
                                                               Nk=77, kv_div=frames // 2, scale=0.125, out=out),
                     "gated": lambda: K.linear_cross_attention(x, w, a, gn, gr, None, kv1[:, :N], kv1[:, N:], Nq=nq,
                                                               Nk=77, kv_div=1, scale=0.125, out=out, gate=gate,
                                                               gate_div=div)}
        else:
            sides = {"plain": lambda: K.linear_lora(x, w, a, gn, gr, out=out),
                     "gated": lambda: K.linear_lora(x, w, a, gn, gr, out=out, gate=gate, gate_div=div)}
        for fn in sides.values():
            fn(), fn()
        t = {s: [] for s in sides}
        for _ in range(passes):
            for s, fn in sides.items():
                t[s].append(timed(fn, iters))
        # (tile: the width vst_gemm_lora takes for the shape; the xattn launches always run 256x192 tiles)
        rec = {"what": "gemm_lora_gate_ab", "shape": name, "tile": K.gemm_lora_tile(M, N, Kd, P, gn, gr),
               "passes": passes, "iters": iters}
        summary(rec, t, "us", 1e3, 2)
        rec["gated_minus_plain_us"] = round(rec["gated_us"] - rec["plain_us"], 2)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    for M, P, div in ((32768, 64, 1024), (32 * 77, 32, 77)):
        u = torch.randn(M, P, generator=g).to(BF).to(dev)
        gate = (torch.rand(M // div, P, generator=g) + 0.5).to(dev)
        fn = lambda: K.lora_gate(u, gate, div, out=u)  # noqa: E731
        fn(), fn()
        rec = {"what": "lora_gate", "shape": f"{M}x{P}, gate_div {div}", "passes": passes, "iters": iters}
        summary(rec, {"lora_gate": [timed(fn, iters) for _ in range(passes)]}, "us", 1e3, 2)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    return recs


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


def lora_launches(den):
    """One eager step under the launch profiler: {kernel name: [launches, total ms]} of the LoRA projections, the
    fused cross-attention and vst_lora_gate."""
    K.profile_launches(True)
    den._step()
    rec = K.collect_launches()
    K.profile_launches(False)
    out = {}
    for kind, sym, _f, _b, ms, _shape in rec:
        if kind in ("gemm_lora", "gemm_xattn", "lora_gate", "gemm_lora_down"):
            e = out.setdefault(sym or kind, [0, 0.0])
            e[0] += 1
            e[1] += ms
    return {k: [n, round(ms, 3)] for k, (n, ms) in sorted(out.items())}


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
        raise SystemExit("lora_gate_bench: no HIP device (timings need the GPU)")
    dev = torch.device("cuda")
    recs = kernel_ab(a.passes, a.iters, dev)
    if not a.no_step:
        from video_style_transfer_amd.utils import build_unet
        unet = build_unet(seed=0, lora_rank=8, device=dev)
        dens = {s: make_denoiser(unet, dev) for s in ("plain", "gates_one", "style_ramp")}
        dens["gates_one"].set_lora_gates(1.0, 1.0)
        dens["style_ramp"].set_lora_gates(style=torch.linspace(0.0, 1.0, FRAMES))
        for den in dens.values():
            den.init_latents(seed=42)
            den.run_steps(a.warmup)
        t = {s: [] for s in dens}
        for _ in range(a.passes):
            for s, den in dens.items():
                t[s].append(run_ms(den, a.steps))
        for den in dens.values():
            assert torch.isfinite(den.lat).all()
        rec = {"what": "denoise_step", "shape": f"{FRAMES} x {SIDE}^2, {STEPS} steps, CFG pair, whole-step graph",
               "passes": a.passes, "steps_per_pass": a.steps}
        summary(rec, t, "step_ms", 1.0, 2)
        rec["gates_one_minus_plain_ms"] = round(rec["gates_one_step_ms"] - rec["plain_step_ms"], 2)
        rec["style_ramp_minus_plain_ms"] = round(rec["style_ramp_step_ms"] - rec["plain_step_ms"], 2)
        rec["plain_spread_ms"] = round(rec["plain_step_ms_range"][1] - rec["plain_step_ms_range"][0], 2)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
        lr = {"what": "lora_launches_eager_step", "note": "device events around each launch of one eager step",
              "plain": lora_launches(dens["plain"]), "style_ramp": lora_launches(dens["style_ramp"])}
        for s in ("plain", "style_ramp"):
            lr[f"{s}_total_ms"] = round(sum(ms for _, ms in lr[s].values()), 3)
        print(json.dumps(lr), flush=True)
        recs.append(lr)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/lora_gate_bench.py", "device": torch.cuda.get_device_name(0), "records": recs},
                      f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
