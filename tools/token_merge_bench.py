"""Token merging: what the three kernels cost, next to a LayerNorm launch over the same rows, and what
the option does to the captured denoise step.  Report only: whichever way the step figure comes out, it is written down.

Kernels: kernels.tome_match / tome_merge / tome_unmerge_add at ratio 0.5 on the two levels of the bench workload's
CFG batch (16 x 512^2: 32 images of 32 x 32 tokens x 640 channels and of 16 x 16 x 1280), random destinations, with
kernels.layer_norm over the same [nimg * N, C] rows as the yardstick; the four alternate in every pass.
Step: AnimateDiffDenoiser at the bench workload with the whole-step HIP graph, one model, one process; the plain step and
ratio 0.5 attn-only / attn + mlp at max_downsample 2 and 4 alternate in every pass.  Each record also holds the relative
L2 distance of the latents after the timed steps from the plain run's: the option changes the result (image quality is
not evaluated here).

  python tools/token_merge_bench.py [--out profiles/token_merge_<date>.json] [--passes 5] [--iters 50] [--steps 4] [--no-step]
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
from video_style_transfer_amd.token_merge import TokenMerging  # noqa: E402

BF16 = torch.bfloat16
FRAMES, SIDE, STEPS = 16, 512, 50
LEVELS = [(32, 32, 32, 640), (32, 16, 16, 1280)]  # (images of the CFG batch, H, W, C)
CONFIGS = [("off", None),
           ("attn_md2", dict(ratio=0.5, max_downsample=2)),
           ("attn_mlp_md2", dict(ratio=0.5, max_downsample=2, merge_mlp=True)),
           ("attn_md4", dict(ratio=0.5, max_downsample=4)),
           ("attn_mlp_md4", dict(ratio=0.5, max_downsample=4, merge_mlp=True))]


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def kernel_records(passes, iters, dev):
    recs = []
    for nimg, H, W, C in LEVELS:
        N, Nd, Ns, r = K.tome_sizes(H, W, 2, 2, 0.5)
        g = torch.Generator().manual_seed(H + C)
        x = torch.randn(nimg * N, C, generator=g).to(BF16).to(dev)
        o = torch.randn(nimg * (N - r), C, generator=g).to(BF16).to(dev)
        gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        plan = K.tome_plan(nimg, N, dev)
        best = torch.empty(nimg, Ns, dtype=torch.float32, device=dev)
        seed = torch.tensor([42], dtype=torch.int64, device=dev)
        step = torch.zeros(1, dtype=torch.int32, device=dev)
        merged, full, normed = torch.empty_like(o), torch.empty_like(x), torch.empty_like(x)
        sides = {
            "match": lambda: K.tome_match(x, nimg, H, W, r, plan, seed=seed, step_idx=step, layer=3, best=best),
            "merge": lambda: K.tome_merge(x, nimg, H, W, r, plan, out=merged),
            "unmerge_add": lambda: K.tome_unmerge_add(o, nimg, N, r, plan, residual=x, out=full),
            "layer_norm": lambda: K.layer_norm(x, gamma, beta, out=normed),
        }
        for fn in sides.values():
            for _ in range(3):
                fn()
        t = {k: [] for k in sides}
        for _ in range(passes):
            for k, fn in sides.items():
                t[k].append(timed(fn, iters))
        rec = {"what": "token_merge_kernels", "images": nimg, "H": H, "W": W, "C": C, "ratio": 0.5, "r": r,
               "destinations": Nd, "sources": Ns, "passes": passes, "iters": iters,
               "match_launches": 4, "score_flops": 2.0 * nimg * Ns * Nd * C}
        for k, v in t.items():
            rec[f"{k}_us"] = round(statistics.median(v) * 1e3, 2)
            rec[f"{k}_us_range"] = [round(min(v) * 1e3, 2), round(max(v) * 1e3, 2)]
        for k in ("match", "merge", "unmerge_add"):
            rec[f"{k}_vs_layer_norm"] = round(rec[f"{k}_us"] / rec["layer_norm_us"], 3)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    return recs


def step_records(passes, steps, warmup, dev):
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser
    from video_style_transfer_amd.utils import build_unet
    unet = build_unet(seed=0, lora_rank=8, device=dev)
    cfg = unet.config
    g = torch.Generator().manual_seed(5)
    enc = torch.randn(2, 77, cfg.cross_attention_dim, generator=g)
    pooled = torch.randn(2, cfg.text_embed_dim, generator=g)
    dens = {}
    for name, kw in CONFIGS:
        den = AnimateDiffDenoiser(unet, FRAMES, SIDE, SIDE, device=dev, num_inference_steps=STEPS,
                                  token_merging=None if kw is None else TokenMerging(**kw))
        den.set_prompt_embeds(enc[1:2], pooled[1:2], enc[0:1], pooled[0:1])
        den.init_latents(seed=42)
        den.run_steps(warmup)
        dens[name] = den
    t = {name: [] for name in dens}
    for _ in range(passes):
        for name, den in dens.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            den.run_steps(steps)
            torch.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) * 1e3 / steps)
    recs = []
    base = dens["off"].lat
    for name, kw in CONFIGS:
        den = dens[name]
        assert torch.isfinite(den.lat).all()
        tm = den.token_merging
        rec = {"what": "denoise_step", "config": name, "token_merging": kw, "passes": passes, "steps_per_pass": steps,
               "shape": f"{FRAMES} x {SIDE}^2, CFG pair, whole-step graph, {STEPS}-step Euler",
               "merged_layers": 0 if tm is None else len(tm.layers),
               "step_ms": round(statistics.median(t[name]), 3),
               "step_ms_range": [round(min(t[name]), 3), round(max(t[name]), 3)],
               "latents_rel_l2_vs_off": round(((den.lat - base).norm() / base.norm()).item(), 5)}
        rec["step_ms_vs_off"] = round(rec["step_ms"] - statistics.median(t["off"]), 3)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    return recs


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
        raise SystemExit("token_merge_bench: no HIP device (timings need the GPU)")
    dev = torch.device("cuda")
    recs = kernel_records(a.passes, a.iters, dev)
    if not a.no_step:
        recs += step_records(a.passes, a.steps, a.warmup, dev)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/token_merge_bench.py", "device": torch.cuda.get_device_name(0), "records": recs},
                      f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
