"""IP-Adapter image attention: vst_ip_attention_add against the same result composed from the kernels
the project had before it, and one captured denoise step without and with an image prompt.

Kernel A/B, one process, both sides alternating round by round (device events around `iters` back-to-back calls;
median and min..max over the rounds), at the two attn2 shapes of a 16 x 512^2 CFG-pair step (M = 8192, C = 1280, 20
heads; M = 32768, C = 640, 10 heads), each with T = 4 and T = 16 image tokens:
  kernel     K.ip_attention_add on the attention output O (x read once, O read and written, no q)
  composed   q = K.linear_lora(x, W | V_up, A_cat) to HBM, K.spatial_attention(q, k_ip, v_ip) over the T keys into a
             buffer, O += scale * that buffer in torch: strictly more bytes
Each side is timed hot (one operand set, called back to back) and cold (`*_cold`: every call takes the next of a ring
of operand sets of more than 640 MB in all, as a step's activations arrive).  Bytes per second are the kernel's needed
bytes (x, O twice, the live rows of G and V) over its time, next to vst_probe_hbm_read's streaming rate measured in the
same process.  The two sides' outputs are compared first (rel-L2 printed).

Step: AnimateDiffDenoiser at 16 x 512^2, CFG pair, whole-step HIP graph, the plain model and the same model with an
IP-Adapter of 4 tokens loaded and an image prompt set, both captured up front and replayed alternately.

  python tools/ip_attention_bench.py [--out profiles/ip_adapter_<date>.json] [--no-step] [--rounds 7]
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
# name, frames (CFG pair of 16), Nq, C, heads
SHAPES = [("16^2 level", 32, 256, 1280, 20), ("32^2 level", 32, 1024, 640, 10)]
TOKENS = (4, 16)
COLD_BYTES = 640 << 20  # more than twice the 256 MiB last-level cache
RANK_PAD, RANK = 32, 16  # UnZipLoRA r = 8 on to_q: [content | style] columns, padded to 32


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def kernel_ab(name, frames, Nq, C, heads, T, rounds, iters, dev, hbm_gbs):
    from video_style_transfer_amd.ip_adapter import fold_image_keys
    M, nb, kv_div = frames * Nq, 2, frames // 2
    g = torch.Generator(device="cpu").manual_seed(frames + Nq + C + T)
    W = torch.zeros(C, C + RANK_PAD)
    W[:, :C] = torch.randn(C, C, generator=g) * C ** -0.5
    W[:, C:C + RANK] = torch.randn(C, RANK, generator=g) * 0.25
    A = torch.zeros(RANK_PAD, C)
    A[:RANK] = torch.randn(RANK, C, generator=g) * C ** -0.5
    W, A = W.to(BF), A.to(BF)
    kv = torch.randn(nb * T, 2 * C, generator=g).to(BF)
    w_eff = W[:, :C].float() + W[:, C:].float() @ A.float()
    Gf, _ = fold_image_keys(kv[:, :C].float().view(nb, T, C), w_eff, None, heads)
    G = torch.zeros(nb, heads, 16, C)
    G[:, :, :T] = Gf
    V = torch.zeros(nb, 16, C)
    V[:, :T] = kv[:, C:].float().view(nb, T, C)
    G, V = G.view(-1, C).to(BF).to(dev), V.view(-1, C).to(BF).to(dev)
    W, A, kv = W.to(dev), A.to(dev), kv.to(dev)
    x0 = torch.randn(M, C, generator=g).to(BF).to(dev)
    o0 = torch.randn(M, C, generator=g).to(BF).to(dev)
    ring = [(x0.clone(), o0.clone()) for _ in range(COLD_BYTES // (4 * M * C) + 1)]
    turn = [0]

    def nxt():
        turn[0] = (turn[0] + 1) % len(ring)
        return ring[turn[0]]

    q = torch.empty(M, C, dtype=BF, device=dev)
    a = torch.empty(M, C, dtype=BF, device=dev)

    def kernel(x, o):
        K.ip_attention_add(x, G, None, V, o, Nq=Nq, heads=heads, T=T, kv_div=kv_div, scale=0.125)

    in_gemm = K.gemm_lora_tile(M, C, C, RANK_PAD, C, RANK) > 0

    def composed(x, o):
        if in_gemm:
            K.linear_lora(x, W, A, C, RANK, out=q)
        else:
            K.linear(x, W, x2=K.linear(x, A), out=q)
        K.spatial_attention(q, kv[:, :C], kv[:, C:], frames, heads, Nq, T, kv_div, out=a, scale=0.125)
        o.add_(a)

    oa, ob = o0.clone(), o0.clone()
    kernel(x0, oa)
    composed(x0, ob)
    diff = ((oa.float() - ob.float()).norm() / (ob.float() - o0.float()).norm()).item()  # on the added term
    hot = {"kernel": (x0.clone(), o0.clone()), "composed": (x0.clone(), o0.clone())}
    sides = {"kernel": lambda: kernel(*hot["kernel"]), "composed": lambda: composed(*hot["composed"]),
             "kernel_cold": lambda: kernel(*nxt()), "composed_cold": lambda: composed(*nxt())}
    for fn in sides.values():
        fn(), fn()
    t = {s: [] for s in sides}
    for _ in range(rounds):
        for s, fn in sides.items():
            t[s].append(timed(fn, iters))
    med = {s: statistics.median(v) for s, v in t.items()}
    needed = 2.0 * (3 * M * C + nb * heads * T * C + nb * T * C)
    rec = {"what": "kernel_ab", "shape": name, "M": M, "C": C, "heads": heads, "T": T, "rounds": rounds, "iters": iters,
           "cold_ring_MB": round(len(ring) * 4 * M * C / 1e6, 1), "needed_MB": round(needed / 1e6, 1),
           "composed_needed_MB": round(2.0 * (7 * M * C) / 1e6, 1), "hbm_probe_TBps": round(hbm_gbs / 1e3, 2),
           "outputs_rel_l2_of_added_term": float(f"{diff:.3e}")}
    for s in sides:
        rec[f"{s}_us"] = round(med[s] * 1e3, 1)
        rec[f"{s}_us_range"] = [round(min(t[s]) * 1e3, 1), round(max(t[s]) * 1e3, 1)]
    for temp in ("", "_cold"):
        rec[f"kernel{temp}_TBps"] = round(needed / (med[f"kernel{temp}"] * 1e-3) / 1e12, 2)
        rec[f"composed_over_kernel{temp}"] = round(med[f"composed{temp}"] / med[f"kernel{temp}"], 2)
    print(json.dumps(rec), flush=True)
    return rec


def make_denoiser(unet, dev, image):
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser
    cfg = unet.config
    den = AnimateDiffDenoiser(unet, 16, 512, 512, num_inference_steps=50, device=dev)
    g = torch.Generator().manual_seed(5)
    enc = torch.randn(2, 77, cfg.cross_attention_dim, generator=g)
    pooled = torch.randn(2, cfg.text_embed_dim, generator=g)
    den.set_prompt_embeds(enc[1:2], pooled[1:2], enc[0:1], pooled[0:1])
    if image:
        den.set_image_prompt(torch.randn(1, 1280, generator=g))
    den.init_latents(seed=42)
    return den


def synthetic_adapter(unet, tokens=4, embed=1280):
    from video_style_transfer_amd.ip_adapter import ip_adapter_layers
    g = torch.Generator().manual_seed(9)
    D = unet.config.cross_attention_dim
    ipa = {}
    for i, (_, m) in enumerate(ip_adapter_layers(unet)):
        for w in ("to_k_ip", "to_v_ip"):
            ipa[f"{2 * i + 1}.{w}.weight"] = torch.randn(m.inner_dim, D, generator=g) * D ** -0.5
    proj = {"proj.weight": torch.randn(tokens * D, embed, generator=g) * embed ** -0.5,
            "proj.bias": torch.zeros(tokens * D), "norm.weight": torch.ones(D), "norm.bias": torch.zeros(D)}
    return {"image_proj": proj, "ip_adapter": ipa}


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
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ip_attention_bench: no HIP device (timings need the GPU)")
    dev = torch.device("cuda")
    hbm = K.probe_hbm_read_gbs(dev)
    recs = [kernel_ab(*shape, T, a.rounds, a.iters, dev, hbm) for shape in SHAPES for T in TOKENS]
    if not a.no_step:
        from video_style_transfer_amd.ip_adapter import load_ip_adapter
        from video_style_transfer_amd.utils import build_unet
        # two models with the same seeded weights: a captured step holds its model's processors
        dens = {"plain": make_denoiser(build_unet(seed=0, lora_rank=8, device=dev), dev, False)}
        unet = build_unet(seed=0, lora_rank=8, device=dev)
        layers = load_ip_adapter(unet, synthetic_adapter(unet))
        dens["image_prompt"] = make_denoiser(unet, dev, True)
        for den in dens.values():
            den.run_steps(a.warmup)
        t = {s: [] for s in dens}
        for _ in range(a.rounds):
            for s, den in dens.items():
                t[s].append(run_ms(den, a.steps))
        for den in dens.values():
            assert torch.isfinite(den.lat).all()
        med = {s: statistics.median(v) for s, v in t.items()}
        rec = {"what": "denoise_step", "shape": "16 x 512^2, CFG pair, whole-step graph", "rounds": a.rounds,
               "steps_per_round": a.steps, "ip_layers": layers, "image_tokens": 4}
        for s in dens:
            rec[f"{s}_step_ms"] = round(med[s], 2)
            rec[f"{s}_step_ms_range"] = [round(min(t[s]), 2), round(max(t[s]), 2)]
        rec["delta_ms"] = round(med["image_prompt"] - med["plain"], 2)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/ip_attention_bench.py", "device": torch.cuda.get_device_name(0),
                       "records": recs}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
