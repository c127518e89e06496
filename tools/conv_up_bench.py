"""Isolated A/B of the nearest-2x upsample conv: the folded path (four 2x2 convs on folded weights,
K.conv3x3_up_folded) against the 3x3 kernel path (K.conv3x3(upsample=True)) at the two UNet upsampler shapes of the
16x512^2 CFG-pair step and the three of the VAE decoder's 4-frame chunks.  One JSON line per shape: kernel names, device
time per call of both (graph-timed), their ratio against the ideal 4/9, and rel_l2 / rel_max of the folded output
against the 3x3 path's.  Inputs come from a seeded CPU generator.

    python tools/conv_up_bench.py            # all shapes; arguments: substrings of the case names"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_style_transfer_amd import kernels as K  # noqa: E402

BF16 = torch.bfloat16
DEV = "cuda"

# (name, nimg, C, Cout, H, W) of the input grid
SHAPES = [("unet_up0_16to32", 32, 1280, 1280, 16, 16), ("unet_up1_32to64", 32, 640, 640, 32, 32),
          ("vae_up0_64to128", 4, 512, 512, 64, 64), ("vae_up1_128to256", 4, 512, 512, 128, 128),
          ("vae_up2_256to512", 4, 256, 256, 256, 256)]


def timeit(fn, reps=10):
    """Device time per call in us: `reps` calls captured in one HIP graph."""
    fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        fn()  # warm the caching allocator on the capture stream
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(reps):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    graph.replay()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def main():
    only = sys.argv[1:]
    for name, n, C, Co, H, W in SHAPES:
        if only and not any(o in name for o in only):
            continue
        g = torch.Generator(device="cpu").manual_seed(C + Co + H)
        x = torch.randn(n * H * W, C, generator=g).to(BF16).to(DEV)
        w = (torch.randn(Co, 9 * C, generator=g) * (9 * C) ** -0.5).to(BF16).to(DEV)
        b = (torch.randn(Co, generator=g) * 0.1).to(DEV)
        wf = K.fold_upsample_weight(w)
        out = torch.empty(n * 4 * H * W, Co, dtype=BF16, device=DEV)
        M = n * 4 * H * W
        rows = 4 * ((n * H * W + K.FOLD_ROW_ALIGN - 1) // K.FOLD_ROW_ALIGN * K.FOLD_ROW_ALIGN)
        us3 = timeit(lambda: K.conv3x3(x, n, H, W, w, b, upsample=True, out=out))
        y3 = out.clone()
        usf = timeit(lambda: K.conv3x3_up_folded(x, n, H, W, wf, b, out=out))
        d = out.float() - y3.float()
        print(json.dumps({
            "case": name, "M": M, "N": Co, "C": C,
            "kernel_3x3": K.gemm_kernel_name(M, Co, 9 * C, 2), "kernel_folded": K.gemm_kernel_name(rows, Co, 4 * C, 4),
            "us_3x3": round(us3, 1), "us_folded": round(usf, 1), "ratio": round(usf / us3, 3), "ideal": round(4 / 9, 3),
            "tflops_3x3": round(2.0 * M * Co * 9 * C / us3 / 1e6, 1),
            "tflops_folded": round(2.0 * M * Co * 4 * C / usf / 1e6, 1),
            "rel_l2": float(d.norm() / y3.float().norm()), "rel_max": float(d.abs().max() / y3.float().abs().max()),
        }), flush=True)
        del x, w, wf, out, y3, d
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
