"""FreeU: what the six launches of a step cost, against a copy of the same bytes, and what they add to
the denoise step.

Kernel: the six vst_freeu launches of one step at the bench workload (16 x 512^2, CFG pair: 32 images), as the up
blocks issue them (x scaled in place, the skip filtered into a new tensor):
  stage 0, 16 x 16: (Cx, Cs) = (1280, 1280), (1280, 1280), (1280, 640)
  stage 1, 32 x 32: (Cx, Cs) = (1280, 640), (640, 640), (640, 320)
Each launch rotates over enough operand sets to exceed the 256 MiB last-level cache ("cold": the skip was written a
whole down path earlier), and is also timed on one set ("hot").  Bytes the algorithm needs: the skip read once and
written once (4 rows Cs) plus half of x read and written (2 rows Cx).  The yardstick is measured here, not assumed:
torch's device-to-device copy (tools/copy_roofline.py's method) of the launch's skip, rotating over the same sets, in
the same passes, alternating with the kernel; `vs_copy` is kernel bytes/s over copy bytes/s.
Step: AnimateDiffDenoiser at the bench workload with the whole-step HIP graph, FreeU off and on (SDXL values) over one
UNet, captured up front and replayed alternately.

  python tools/freeu_bench.py [--out profiles/freeu_<date>.json] [--passes 5] [--iters 40] [--steps 4] [--no-step]
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
from video_style_transfer_amd.freeu import SDXL, FreeU  # noqa: E402

BF = torch.bfloat16
FRAMES, SIDE, STEPS, NIMG = 16, 512, 50, 32
LAUNCHES = [(0, 16, 1280, 1280), (0, 16, 1280, 1280), (0, 16, 1280, 640),
            (1, 32, 1280, 640), (1, 32, 640, 640), (1, 32, 640, 320)]   # (stage, H = W, Cx, Cs)
COLD_BYTES = 640 << 20


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(iters):
        fn(i)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def kernel_records(passes, iters, dev):
    fu = FreeU(**SDXL, device=dev)
    recs = []
    for stage, side, Cx, Cs in sorted(set(LAUNCHES)):
        rows = NIMG * side * side
        need = 4.0 * rows * Cs + 2.0 * rows * Cx
        per_set = 2 * rows * (Cx + 2 * Cs)
        nset = max(2, -(-COLD_BYTES // per_set))
        g = torch.Generator().manual_seed(Cs + side)
        sets = [(torch.randn(rows, Cx, generator=g).to(BF).to(dev), torch.randn(rows, Cs, generator=g).to(BF).to(dev),
                 torch.empty(rows, Cs, dtype=BF, device=dev)) for _ in range(nset)]

        def kern(i, n):
            x, s, o = sets[i % n]
            K.freeu(x, s, NIMG, side, side, fu.table, stage, x_out=x, skip_out=o)

        def copy(i, n):
            _, s, o = sets[i % n]
            o.copy_(s)

        sides = {"freeu_cold": lambda i: kern(i, nset), "copy_cold": lambda i: copy(i, nset),
                 "freeu_hot": lambda i: kern(i, 1), "copy_hot": lambda i: copy(i, 1)}
        for fn in sides.values():
            for i in range(nset):
                fn(i)
        t = {k: [] for k in sides}
        for _ in range(passes):
            for k, fn in sides.items():
                t[k].append(timed(fn, iters))
        rec = {"what": "freeu_launch", "stage": stage, "HxW": f"{side}x{side}", "nimg": NIMG, "Cx": Cx, "Cs": Cs,
               "per_step": LAUNCHES.count((stage, side, Cx, Cs)), "operand_sets": nset, "passes": passes,
               "iters": iters, "bytes_needed": int(need), "copy_bytes": int(4.0 * rows * Cs)}
        for k, x in t.items():
            nb = need if k.startswith("freeu") else 4.0 * rows * Cs
            med = statistics.median(x)
            rec[f"{k}_us"] = round(med * 1e3, 2)
            rec[f"{k}_us_range"] = [round(min(x) * 1e3, 2), round(max(x) * 1e3, 2)]
            rec[f"{k}_TBs"] = round(nb / med / 1e9, 3)
        for temp in ("cold", "hot"):
            rec[f"vs_copy_{temp}"] = round(rec[f"freeu_{temp}_TBs"] / rec[f"copy_{temp}_TBs"], 3)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
        del sets
        torch.cuda.empty_cache()
    total = {"what": "freeu_launches_per_step",
             "cold_us": round(sum(r["freeu_cold_us"] * r["per_step"] for r in recs), 1),
             "hot_us": round(sum(r["freeu_hot_us"] * r["per_step"] for r in recs), 1)}
    print(json.dumps(total), flush=True)
    return recs + [total]


def make_denoiser(unet, dev, **kw):
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser
    cfg = unet.config
    den = AnimateDiffDenoiser(unet, FRAMES, SIDE, SIDE, device=dev, num_inference_steps=STEPS, **kw)
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


def step_record(passes, steps, warmup, dev):
    from video_style_transfer_amd.utils import build_unet
    unet = build_unet(seed=0, lora_rank=8, device=dev)
    dens = {"plain": make_denoiser(unet, dev), "freeu": make_denoiser(unet, dev, freeu=tuple(SDXL[k] for k in
                                                                                            ("s1", "s2", "b1", "b2")))}
    for den in dens.values():
        den.init_latents(seed=42)
        den.run_steps(warmup)
    t = {s: [] for s in dens}
    for _ in range(passes):
        for s, den in dens.items():
            t[s].append(run_ms(den, steps))
    for den in dens.values():
        assert torch.isfinite(den.lat).all()
    rec = {"what": "denoise_step", "passes": passes, "steps_per_pass": steps,
           "shape": f"{FRAMES} x {SIDE}^2, CFG pair, whole-step graph, {STEPS}-step Euler table"}
    for s, x in t.items():
        rec[f"{s}_step_ms"] = round(statistics.median(x), 3)
        rec[f"{s}_step_ms_range"] = [round(min(x), 3), round(max(x), 3)]
    rec["freeu_minus_plain_ms"] = round(rec["freeu_step_ms"] - rec["plain_step_ms"], 3)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("freeu_bench: no HIP device (timings need the GPU)")
    dev = torch.device("cuda")
    recs = kernel_records(a.passes, a.iters, dev)
    if not a.no_step:
        recs.append(step_record(a.passes, a.steps, a.warmup, dev))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/freeu_bench.py", "device": torch.cuda.get_device_name(0), "records": recs},
                      f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
