"""StyleAligned AdaIN of q/k/v to the anchor frame: the kernel against the same arithmetic in torch, and
one captured denoise step with cross_frame=("first",) against the same with adain="qk".

Kernel A/B, one process, all sides alternating round by round (device events around `iters` back-to-back calls; median
and min..max over the rounds), on the first 2 C ("qk") or 3 C ("qkv") columns of one [rows, 3C] bf16 projection:
  kernel_qk / kernel_qkv  K.frame_adain (two launches: statistics, apply), stats buffer given
  torch_qk / torch_qkv    torch.var_mean over the tokens of every frame (fp32), the broadcast affine
                          (x - mu_f) * (sd_a / sd_f) + mu_a on the non-anchor frames and the write-back into the bf16
                          buffer; the conversions and copies are part of the timed work
Each side is timed hot (one buffer, called back to back: 42-126 MB, which the 256 MiB last-level cache holds) and
cold (`*_cold`: every call takes the next of a ring of copies of more than 640 MB in all, as a step's q/k/v arrive).
The AdaIN runs in place, so after a few calls every frame has the anchor's statistics and the arithmetic goes on
unchanged (the ratio is 1): the traffic and the work per call stay what they were.  The two sides' outputs are compared
on a fresh copy first (rel-L2 printed).

Step: AnimateDiffDenoiser at 16 x 512^2, CFG pair, whole-step HIP graph, cross_frame=("first",) without and with
adain="qk", both captured up front and replayed alternately, `--steps` replays per round.

  python tools/frame_adain_bench.py [--out profiles/frame_adain_<date>.json] [--no-step] [--rounds 7]
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
SHAPES = [("16^2 level", 2, 16, 256, 1280), ("32^2 level", 2, 16, 1024, 640)]  # nclip F N inner (16 x 512^2, CFG pair)
BLOCKS = {"qk": 2, "qkv": 3}
EPS = 1e-5
COLD_BYTES = 640 << 20  # more than twice the 256 MiB last-level cache


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def torch_adain(x, nclip, Fr, N):
    """The kernel's arithmetic (anchor = frame 0) as torch ops on the device, in place on the bf16 view x."""
    x4 = x.unflatten(0, (nclip, Fr, N))  # a view: the rows of a column slice keep one stride
    var, mu = torch.var_mean(x4.float(), 2, unbiased=True, keepdim=True)
    sd = (var + EPS).sqrt()
    y = (x4[:, 1:].float() - mu[:, 1:]) * (sd[:, :1] / sd[:, 1:]) + mu[:, :1]
    x4[:, 1:] = y.to(BF)


def kernel_ab(name, nclip, Fr, N, inner, rounds, iters, dev):
    rows = nclip * Fr * N
    g = torch.Generator(device="cpu").manual_seed(Fr + N + inner)
    gain = 0.5 + torch.rand(nclip * Fr, 1, 3 * inner, generator=g)
    shift = torch.randn(nclip * Fr, 1, 3 * inner, generator=g)
    src = (torch.randn(nclip * Fr, N, 3 * inner, generator=g) * gain + shift).view(rows, 3 * inner).to(BF).to(dev)
    stats = {m: torch.empty(nclip * Fr, 2, b * inner, dtype=torch.float32, device=dev) for m, b in BLOCKS.items()}
    # hot: one buffer per side, called back to back; cold: every call takes the next of a ring of copies that is
    # larger than COLD_BYTES in all, so no call finds its operand in the last-level cache
    ring = [src.clone() for _ in range(COLD_BYTES // (src.numel() * 2) + 1)]
    turn = [0]

    def nxt():
        turn[0] = (turn[0] + 1) % len(ring)
        return ring[turn[0]]

    bufs = {f"{k}_{m}": src.clone() for k in ("kernel", "torch") for m in BLOCKS}
    sides = {}
    for m, b in BLOCKS.items():
        for temp, pick in (("", lambda s: bufs[s]), ("_cold", lambda s: nxt())):
            sides[f"kernel_{m}{temp}"] = lambda m=m, b=b, pick=pick: K.frame_adain(
                pick(f"kernel_{m}")[:, :b * inner], nclip, Fr, N, 0, eps=EPS, stats=stats[m])
            sides[f"torch_{m}{temp}"] = lambda m=m, b=b, pick=pick: torch_adain(
                pick(f"torch_{m}")[:, :b * inner], nclip, Fr, N)
    diff = {}
    for m in BLOCKS:
        sides[f"kernel_{m}"](), sides[f"torch_{m}"]()
        a, b = bufs[f"kernel_{m}"].float(), bufs[f"torch_{m}"].float()
        diff[m] = ((a - b).norm() / b.norm()).item()
        del a, b
    for fn in sides.values():
        fn(), fn()
    t = {s: [] for s in sides}
    for _ in range(rounds):
        for s, fn in sides.items():
            t[s].append(timed(fn, iters))
    med = {s: statistics.median(x) for s, x in t.items()}
    rec = {"what": "kernel_ab", "shape": name, "nclip": nclip, "F": Fr, "N": N, "inner": inner, "rounds": rounds,
           "iters": iters, "cold_ring_MB": round(len(ring) * src.numel() * 2 / 1e6, 1)}
    for s in sides:
        rec[f"{s}_us"] = round(med[s] * 1e3, 1)
        rec[f"{s}_us_range"] = [round(min(t[s]) * 1e3, 1), round(max(t[s]) * 1e3, 1)]
    for m, b in BLOCKS.items():
        x_bytes = 2.0 * rows * b * inner
        moved = x_bytes * (1 + 2 * (Fr - 1) / Fr)  # one read for the statistics, the non-anchor frames read and written
        rec[f"x_MB_{m}"] = round(x_bytes / 1e6, 1)
        rec[f"needed_MB_{m}"] = round(moved / 1e6, 1)
        for temp in ("", "_cold"):
            rec[f"kernel_{m}{temp}_TBps"] = round(moved / (med[f"kernel_{m}{temp}"] * 1e-3) / 1e12, 2)
            rec[f"torch_over_kernel_{m}{temp}"] = round(med[f"torch_{m}{temp}"] / med[f"kernel_{m}{temp}"], 2)
        rec[f"outputs_rel_l2_{m}"] = float(f"{diff[m]:.3e}")
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
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frame_adain_bench: no HIP device (timings need the GPU)")
    dev = torch.device("cuda")
    recs = [kernel_ab(*shape, a.rounds, a.iters, dev) for shape in SHAPES]
    if not a.no_step:
        from video_style_transfer_amd.unet_motion import CrossFrameAttention
        from video_style_transfer_amd.utils import build_unet
        unet = build_unet(seed=0, lora_rank=8, device=dev)
        dens = {"cross_frame": make_denoiser(unet, CrossFrameAttention(("first",)), dev),
                "adain_qk": make_denoiser(unet, CrossFrameAttention(("first",), adain="qk"), dev)}
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
               "steps_per_round": a.steps, "cross_frame": ["first"], "adain": "qk"}
        for s in dens:
            rec[f"{s}_step_ms"] = round(med[s], 2)
            rec[f"{s}_step_ms_range"] = [round(min(t[s]), 2), round(max(t[s]), 2)]
        rec["delta_ms"] = round(med["adain_qk"] - med["cross_frame"], 2)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/frame_adain_bench.py", "device": torch.cuda.get_device_name(0), "records": recs},
                      f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
