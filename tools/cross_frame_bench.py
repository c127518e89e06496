"""Cross-frame spatial self-attention (DESIGN.md "Cross-frame spatial self-attention"): the kernel against the plain
self-attention launch and against the same attention done by gathering K/V in torch, and one captured denoise step
with and without the option.

Kernel A/B, one process, all sides alternating round by round (device events around `iters` back-to-back calls;
median and min..max over the rounds), on the q/k/v column views of one [rows, 3C] projection:
  plain      K.spatial_attention (every frame attends to itself)
  frames1/2  K.spatial_attention_frames with ("first",) / ("first", "prev")
  gather1/2  torch.cat of every frame's own K/V rows with frame 0's (and the previous frame's) into [nclip*F, 2N / 3N]
             keys, then K.spatial_attention(Nq = N, Nk = 2N / 3N); the copies are part of the timed work
The gathered keys have one length for every frame, so a source that repeats an earlier entry stays in them while the
kernel drops it: the same softmax where all entries are one frame (frame 0), another where only two of three are
(frame 1 of ("first", "prev"): frame 0 counted twice).  The outputs are compared first on the frames where both compute
the same thing (rel-L2 printed); the timed work is the same number of keys either way.

Step: AnimateDiffDenoiser at 16 x 512^2, CFG pair, whole-step HIP graph, with and without cross_frame=("first",),
both captured up front and replayed alternately, `--steps` replays per round.

  python tools/cross_frame_bench.py [--out profiles/cross_frame_<date>.json] [--no-step] [--rounds 7]
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
SHAPES = [("16^2 level", 2, 16, 20, 256), ("32^2 level", 2, 16, 10, 1024)]  # nclip F heads N (16 x 512^2, CFG pair)
SOURCES = {1: ("first",), 2: ("first", "prev")}


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def kernel_ab(name, nclip, Fr, heads, N, rounds, iters, dev):
    C, rows = heads * 64, nclip * Fr * N
    g = torch.Generator(device="cpu").manual_seed(Fr + N + heads)
    qkv = torch.randn(rows, 3 * C, generator=g).to(BF).to(dev)
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    out = torch.empty(rows, C, dtype=BF, device=dev)
    prev = torch.tensor([max(f - 1, 0) for f in range(Fr)], device=dev)

    def gathered(t, n):
        t5 = t.view(nclip, Fr, N, C)
        parts = [t5, t5[:, :1].expand(-1, Fr, -1, -1)] + ([t5[:, prev]] if n == 2 else [])
        return torch.cat(parts, 2).view(nclip * Fr * (n + 1) * N, C)

    sides = {"plain": lambda: K.spatial_attention(q, k, v, nclip * Fr, heads, N, N, out=out)}
    for n in (1, 2):
        sides[f"frames{n}"] = lambda n=n: K.spatial_attention_frames(q, k, v, nclip, Fr, heads, N, SOURCES[n], out=out)
        sides[f"gather{n}"] = lambda n=n: K.spatial_attention(q, gathered(k, n), gathered(v, n), nclip * Fr, heads, N,
                                                               (n + 1) * N, out=out)
    diff = {}
    for n in (1, 2):
        same = [f for f in range(Fr) if len(K.frame_list(f, Fr, SOURCES[n])) in (1, n + 1)]
        a = sides[f"frames{n}"]().float().view(nclip, Fr, N, C)[:, same].clone()
        b = sides[f"gather{n}"]().float().view(nclip, Fr, N, C)[:, same]
        diff[n] = ((a - b).norm() / b.norm()).item()
    for fn in sides.values():
        fn(), fn()
    t = {s: [] for s in sides}
    for _ in range(rounds):
        for s, fn in sides.items():
            t[s].append(timed(fn, iters))
    med = {s: statistics.median(x) for s, x in t.items()}
    avg_len = {n: sum(len(K.frame_list(f, Fr, SOURCES[n])) for f in range(Fr)) / Fr for n in (1, 2)}
    rec = {"what": "kernel_ab", "shape": name, "nclip": nclip, "F": Fr, "heads": heads, "N": N, "rounds": rounds,
           "iters": iters}
    for s in sides:
        rec[f"{s}_us"] = round(med[s] * 1e3, 1)
        rec[f"{s}_us_range"] = [round(min(t[s]) * 1e3, 1), round(max(t[s]) * 1e3, 1)]
    for n in (1, 2):
        rec[f"avg_list_length_{n}"] = round(avg_len[n], 4)
        rec[f"frames{n}_over_plain"] = round(med[f"frames{n}"] / med["plain"], 3)
        rec[f"gather{n}_over_frames{n}"] = round(med[f"gather{n}"] / med[f"frames{n}"], 3)
        rec[f"outputs_rel_l2_{n}"] = float(f"{diff[n]:.3e}")
    print(json.dumps(rec), flush=True)
    return rec


def make_denoiser(unet, cross_frame, dev):
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser
    cfg = unet.config
    den = AnimateDiffDenoiser(unet, 16, 512, 512, num_inference_steps=50, device=dev, cross_frame=cross_frame)
    g = torch.Generator().manual_seed(5)
    enc = torch.randn(2, 77, cfg.cross_attention_dim, generator=g)
    pooled = torch.randn(2, cfg.text_embed_dim, generator=g)
    den.set_prompt_embeds(enc[1:2], pooled[1:2], enc[0:1], pooled[0:1])
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
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cross_frame_bench: no HIP device (timings need the GPU)")
    dev = torch.device("cuda")
    recs = [kernel_ab(*shape, a.rounds, a.iters, dev) for shape in SHAPES]
    if not a.no_step:
        from video_style_transfer_amd.utils import build_unet
        unet = build_unet(seed=0, lora_rank=8, device=dev)
        dens = {"plain": make_denoiser(unet, None, dev), "cross_frame": make_denoiser(unet, ("first",), dev)}
        for den in dens.values():
            den.run_steps(a.warmup)
        t = {s: [] for s in dens}
        for _ in range(a.rounds):
            for s, den in dens.items():
                t[s].append(run_ms(den, a.steps))
        for den in dens.values():
            assert torch.isfinite(den.lat).all()
        med = {s: statistics.median(x) for s, x in t.items()}
        rec = {"what": "denoise_step", "shape": "16 x 512^2, CFG pair, whole-step graph", "rounds": a.rounds,
               "steps_per_round": a.steps, "cross_frame": ["first"]}
        for s in dens:
            rec[f"{s}_step_ms"] = round(med[s], 2)
            rec[f"{s}_step_ms_range"] = [round(min(t[s]), 2), round(max(t[s]), 2)]
        rec["delta_ms"] = round(med["cross_frame"] - med["plain"], 2)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/cross_frame_bench.py", "device": torch.cuda.get_device_name(0), "records": recs},
                      f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
