"""Long clips (DESIGN.md "Long clips"): the windowed frame-attention kernel against the same work done window by
window, and one captured denoise step of a 64-frame 512^2 clip next to four 16-frame clips.

Kernel A/B, one process, the two sides alternating round by round (device events around `iters` back-to-back calls;
median and min..max over the rounds):
  windowed   K.temporal_attention_windowed on the [T, 3C] projection and the fp32 [L, 3C] positional table
  gathered   per window (13 at F 64, L 16, S 4): gather the window's q/k/v rows, add the table and round to bf16
             (torch), K.temporal_attention, fp32 weighted accumulate (torch); then the division and the bf16 rounding
Both compute the same thing; their outputs are compared first (rel-L2 printed; fp32 accumulation order differs).
Bytes: the windowed kernel's algorithmic traffic is q, k, v read once + o written once (2 * 4 * T * C).

Step: AnimateDiffDenoiser at 64 x 512^2 with context (16, 4), whole-step HIP graph, `--steps` replays after
`--warmup`; and the 16-frame step without a context in the same run, times four (four separate clips).

  python tools/long_clip_bench.py [--out profiles/long_clip_<date>.json] [--no-step] [--steps 5] [--warmup 2]
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
SHAPES = [("64^2 level", 2, 64, 4096, 40, 16, 4), ("16^2 level", 2, 64, 256, 160, 16, 4)]  # nclip F HW D L S
HEADS = 8


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def kernel_ab(name, nclip, Fr, HW, D, L, S, rounds, iters, dev):
    C = HEADS * D
    T = nclip * Fr * HW
    g = torch.Generator(device="cpu").manual_seed(Fr + HW + D)
    qkv = torch.randn(T, 3 * C, generator=g).to(BF).to(dev)
    table = (torch.randn(L, 3 * C, generator=g) * 0.5).to(dev)
    starts = K.context_windows(Fr, L, S)
    w = torch.tensor(K.context_weights(L, "pyramid"), device=dev)
    den = torch.zeros(Fr, device=dev)
    for s in starts:
        den[s:s + L] += w
    out_w = torch.empty(T, C, dtype=BF, device=dev)
    acc = torch.empty(nclip, Fr, HW, C, device=dev)
    o_win = torch.empty(nclip * L * HW, C, dtype=BF, device=dev)
    q5 = qkv.view(nclip, Fr, HW, 3 * C)

    def windowed():
        K.temporal_attention_windowed(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], table, nclip, Fr, HW, HEADS, D, L, S,
                                      "pyramid", out=out_w)
        return out_w

    def gathered():
        acc.zero_()
        for s in starts:
            x = (q5[:, s:s + L].float() + table.view(1, L, 1, 3 * C)).to(BF).view(nclip * L * HW, 3 * C)
            K.temporal_attention(x[:, :C], x[:, C:2 * C], x[:, 2 * C:], nclip, L, HW, HEADS, D, out=o_win)
            acc[:, s:s + L] += o_win.view(nclip, L, HW, C).float() * w.view(1, L, 1, 1)
        return (acc / den.view(1, Fr, 1, 1)).to(BF).view(T, C)

    a, b = windowed().float(), gathered().float()
    torch.cuda.synchronize()
    diff = ((a - b).norm() / b.norm()).item()
    for _ in range(2):
        windowed(), gathered()
    tw, tg = [], []
    for _ in range(rounds):
        tw.append(timed(windowed, iters))
        tg.append(timed(gathered, max(1, iters // 4)))
    mw, mg = statistics.median(tw), statistics.median(tg)
    rec = {"what": "kernel_ab", "shape": name, "nclip": nclip, "F": Fr, "HW": HW, "head_dim": D, "L": L, "S": S,
           "windows": len(starts), "rounds": rounds,
           "windowed_us": round(mw * 1e3, 1), "windowed_us_range": [round(min(tw) * 1e3, 1), round(max(tw) * 1e3, 1)],
           "gathered_us": round(mg * 1e3, 1), "gathered_us_range": [round(min(tg) * 1e3, 1), round(max(tg) * 1e3, 1)],
           "gathered_over_windowed": round(mg / mw, 2),
           "windowed_algorithmic_gbs": round(2.0 * 4 * T * C / mw / 1e6, 1),
           "outputs_rel_l2": float(f"{diff:.3e}")}
    print(json.dumps(rec), flush=True)
    return rec


def step_ms(unet, frames, context, steps, warmup, dev):
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser
    cfg = unet.config
    den = AnimateDiffDenoiser(unet, frames, 512, 512, num_inference_steps=50, device=dev,
                              **({"context_length": context[0], "context_stride": context[1]} if context else {}))
    g = torch.Generator().manual_seed(5)
    enc = torch.randn(2, 77, cfg.cross_attention_dim, generator=g)
    pooled = torch.randn(2, cfg.text_embed_dim, generator=g)
    den.set_prompt_embeds(enc[1:2], pooled[1:2], enc[0:1], pooled[0:1])
    den.init_latents(seed=42)
    den.run_steps(warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    den.run_steps(steps)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    assert torch.isfinite(den.lat).all()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("long_clip_bench: no HIP device (timings need the GPU)")
    dev = torch.device("cuda")
    recs = [kernel_ab(*shape, a.rounds, a.iters, dev) for shape in SHAPES]
    if not a.no_step:
        from video_style_transfer_amd.utils import build_unet
        unet = build_unet(seed=0, lora_rank=8, device=dev)
        ms16 = step_ms(unet, 16, None, a.steps, a.warmup, dev)
        ms64 = step_ms(unet, 64, (16, 4), a.steps, a.warmup, dev)
        rec = {"what": "denoise_step", "shape": "512^2, CFG pair, whole-step graph", "steps": a.steps,
               "step_ms_16_frames": round(ms16, 2), "four_16_frame_clips_ms": round(4 * ms16, 2),
               "step_ms_64_frames_context_16_4": round(ms64, 2), "ratio_64_over_4x16": round(ms64 / (4 * ms16), 3)}
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/long_clip_bench.py", "device": torch.cuda.get_device_name(0), "records": recs}, f,
                      indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
