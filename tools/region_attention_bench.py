"""Regional prompts: vst_region_attention per launch, its two LDS plans, the attn2 layer with regions
against the plain layer, and one captured denoise step with two disjoint regions against none.

One process, every side alternating round by round (each side captured as a HIP graph of 10 back-to-back calls,
device events around `iters` calls in all; median and min..max over the rounds), at the two attn2 shapes of a
16 x 512^2 CFG-pair step (32 images; Nq 1024, 10 heads, C 640; Nq 256, 20 heads, C 1280), Nk 77, kv_div 16:

  kernel   K.region_attention alone (q given) for R in {1, 2, 4}, with maps "blocks" (R bands of rows aligned to the
           128-query blocks, one-hot: every block has one live region) and "soft" (non-zero everywhere: every region
           live in every block), under LDS plan 0 (the walk, double-buffered through registers) and plan 1 (every live
           region up front by LDS-DMA); next to K.spatial_attention over one prompt's 77 keys on the same q.
  layer    the attn2 layer (AnimateDiffAttnProcessor2_0 on an Attention with UnZipLoRA r = 8, to_out included) as the
           plain fused launch (vst_gemm_cross_attention + to_out), as the plain two-launch path (q GEMM +
           vst_spatial_attention + to_out) and with regions (q GEMM + vst_region_attention + to_out) at R in {1, 2, 4},
           both maps, the default plan.  The plain kernels are the parent commit's: this change does not touch them.

Step: AnimateDiffDenoiser at 16 x 512^2, CFG pair, whole-step HIP graph: no regions, two regions split top / bottom
(aligned to the query blocks at both levels) and two regions split left / right (both live in every block of the
cond clip), captured up front and replayed alternately.

  python tools/region_attention_bench.py [--out profiles/region_attention_<date>.json] [--no-step] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_style_transfer_amd import _lib, kernels as K  # noqa: E402

BF = torch.bfloat16
NIMG, NK, KV_DIV = 32, 77, 16
# name, Nq, C, heads
SHAPES = [("32^2 level", 1024, 640, 10), ("16^2 level", 256, 1280, 20)]
REGIONS = (1, 2, 4)


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


GRAPH_CALLS = 10  # calls per captured graph: the timings are the device's, not the host's launch rate


def graphed(fn):
    fn(), fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(GRAPH_CALLS):
            fn()
    return g.replay


def alternate(sides, rounds, iters):
    sides = {s: graphed(fn) for s, fn in sides.items()}
    t = {s: [] for s in sides}
    for _ in range(rounds):
        for s, fn in sides.items():
            t[s].append(timed(fn, max(iters // GRAPH_CALLS, 1)) / GRAPH_CALLS)
    return {s: (round(statistics.median(v) * 1e3, 1), [round(min(v) * 1e3, 1), round(max(v) * 1e3, 1)])
            for s, v in t.items()}


def maps(kind, Nq, R, dev, g):
    """fp32 [NIMG*Nq, 4] normalised weights: "blocks" = R one-hot bands of Nq / R rows; "soft" = non-zero everywhere."""
    w = torch.zeros(NIMG, Nq, 4)
    if kind == "blocks":
        w[:, :, :R] = torch.nn.functional.one_hot(torch.arange(Nq) * R // Nq, R).float()
    else:
        raw = torch.rand(NIMG, Nq, R, generator=g) + 0.1
        w[:, :, :R] = raw / raw.sum(-1, keepdim=True)
    return w.view(-1, 4).to(dev)


def kernel_ab(name, Nq, C, heads, rounds, iters, dev):
    g = torch.Generator().manual_seed(Nq + C)
    q = torch.randn(NIMG * Nq, C, generator=g).to(BF).to(dev)
    nkv = NIMG // KV_DIV
    kv = {R: torch.randn(nkv * R * NK, 2 * C, generator=g).to(BF).to(dev) for R in REGIONS}
    out = torch.empty_like(q)
    lib = _lib.load()
    sides = {"spatial_attention": lambda: K.spatial_attention(q, kv[1][:, :C], kv[1][:, C:], NIMG, heads, Nq, NK,
                                                              KV_DIV, out=out)}

    def region(R, w, plan):
        def run():
            lib.vst_region_plan(plan)
            K.region_attention(q, kv[R][:, :C], kv[R][:, C:], w, nimg=NIMG, heads=heads, Nq=Nq, Nk=NK, R=R,
                               kv_div=KV_DIV, out=out)
        return run
    prev = lib.vst_region_plan(0)
    try:
        for R in REGIONS:
            for kind in ("blocks", "soft"):
                w = maps(kind, Nq, R, dev, g)
                for plan in (0, 1):
                    sides[f"R{R}_{kind}_plan{plan}"] = region(R, w, plan)
        res = alternate(sides, rounds, iters)
    finally:
        lib.vst_region_plan(prev)
    rec = {"what": "kernel", "shape": name, "nimg": NIMG, "Nq": Nq, "heads": heads, "Nk": NK, "kv_div": KV_DIV,
           "rounds": rounds, "iters": iters}
    for s, (med, rng) in res.items():
        rec[f"{s}_us"], rec[f"{s}_us_range"] = med, rng
    print(json.dumps(rec), flush=True)
    return rec


def layer_ab(name, Nq, C, heads, rounds, iters, dev):
    from video_style_transfer_amd import attention_processor as AP
    from video_style_transfer_amd.attention_processor import AttnCall, Attention
    from video_style_transfer_amd.region_prompts import RegionPrompts
    from video_style_transfer_amd.utils import attach_unziplora_layers
    torch.manual_seed(Nq)
    attn = Attention(C, 2048, heads, 64).to(dev)
    holder = torch.nn.Module()
    holder.blk = torch.nn.Module()
    holder.blk.attn2 = attn
    attach_unziplora_layers(holder, 8)
    holder.to(dev).requires_grad_(False)
    proc = attn.processor
    g = torch.Generator().manual_seed(Nq + 1)
    x = (torch.randn(NIMG, Nq, C, generator=g) * 0.5).to(BF).to(dev)
    res_in = torch.zeros_like(x)
    enc = torch.randn(NIMG // KV_DIV, NK, 2048, generator=g).to(BF).to(dev)
    side = int(Nq ** 0.5)

    def plain():
        proc(attn, x, encoder_hidden_states=enc, _vst=AttnCall(residual=res_in))

    orig = AP._cross_fusable

    def two_launch():
        AP._cross_fusable = lambda *a, **k: False
        try:
            proc(attn, x, encoder_hidden_states=enc, _vst=AttnCall(residual=res_in))
        finally:
            AP._cross_fusable = orig
    sides = {"plain_fused": plain, "plain_two_launch": two_launch}
    for R in REGIONS:
        states = torch.randn(NIMG // KV_DIV, R, NK, 2048, generator=g)
        for kind in ("blocks", "soft"):
            rp = RegionPrompts(states, torch.ones(NIMG, R, side, side), KV_DIV, [(side, side)], dev)
            rp.tables[(side, side)].copy_(maps(kind, Nq, R, dev, g))
            call = AttnCall(residual=res_in, regions=(rp, rp.tables[(side, side)]))
            sides[f"regions_R{R}_{kind}"] = (lambda c: lambda: proc(attn, x, encoder_hidden_states=enc, _vst=c))(call)
    K.profile_launches(True)
    plain()
    fused = "gemm_xattn" in [r[0] for r in K.collect_launches()]
    K.profile_launches(False)
    res = alternate(sides, rounds, iters)
    rec = {"what": "attn2_layer", "shape": name, "nimg": NIMG, "Nq": Nq, "C": C, "heads": heads, "Nk": NK,
           "lora_rank": 8, "plain_runs_fused": fused, "rounds": rounds, "iters": iters}
    for s, (med, rng) in res.items():
        rec[f"{s}_us"], rec[f"{s}_us_range"] = med, rng
    print(json.dumps(rec), flush=True)
    return rec


def make_denoiser(unet, dev, split):
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser
    cfg = unet.config
    den = AnimateDiffDenoiser(unet, 16, 512, 512, num_inference_steps=50, device=dev)
    g = torch.Generator().manual_seed(5)
    enc = torch.randn(2, 77, cfg.cross_attention_dim, generator=g)
    pooled = torch.randn(2, cfg.text_embed_dim, generator=g)
    den.set_prompt_embeds(enc[1:2], pooled[1:2], enc[0:1], pooled[0:1])
    if split is not None:
        m = torch.zeros(1, 1, 64, 64)
        if split == "top_bottom":
            m[..., 32:, :] = 1.0
        else:
            m[..., :, 32:] = 1.0
        den.set_region_prompts(torch.randn(1, 77, cfg.cross_attention_dim, generator=g), m)
    den.init_latents(seed=42)
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("region_attention_bench: no HIP device (timings need the GPU)")
    dev = torch.device("cuda")
    recs = [kernel_ab(*shape, a.rounds, a.iters, dev) for shape in SHAPES]
    recs += [layer_ab(*shape, a.rounds, a.iters, dev) for shape in SHAPES]
    if not a.no_step:
        from video_style_transfer_amd.utils import build_unet
        unet = build_unet(seed=0, lora_rank=8, device=dev)
        dens = {s: make_denoiser(unet, dev, split) for s, split in
                (("plain", None), ("top_bottom", "top_bottom"), ("left_right", "left_right"))}
        for den in dens.values():
            den.run_steps(a.warmup)
        t = {s: [] for s in dens}
        for _ in range(a.rounds):
            for s, den in dens.items():
                t[s].append(run_ms(den, a.steps))
        for den in dens.values():
            assert torch.isfinite(den.lat).all()
        med = {s: statistics.median(v) for s, v in t.items()}
        rec = {"what": "denoise_step", "shape": "16 x 512^2, CFG pair, whole-step graph, two regions", "rounds": a.rounds,
               "steps_per_round": a.steps}
        for s in dens:
            rec[f"{s}_step_ms"] = round(med[s], 2)
            rec[f"{s}_step_ms_range"] = [round(min(t[s]), 2), round(max(t[s]), 2)]
            if s != "plain":
                rec[f"{s}_delta_ms"] = round(med[s] - med["plain"], 2)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/region_attention_bench.py", "device": torch.cuda.get_device_name(0),
                       "records": recs}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
