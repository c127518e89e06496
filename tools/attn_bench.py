"""Spatial / temporal attention kernel timings, forward and backward, at the UNet's shapes (16x512^2, CFG batch 2), and
the A/B tool for csrc/attention.hip:

    bash tools/ab_lib.sh                                   # the committed sources -> abx/libvst_old.so
    VST_LIB_AB=abx/libvst_old.so python tools/attn_bench.py --md5 > old.jsonl; python tools/attn_bench.py --md5 > new.jsonl

Timing (default): one JSON line per shape and pass: forward, `<shape>_bwd_dq` (spatial backward with frozen K/V: the dQ
kernel alone), `<shape>_bwd` (dQ + dK/dV; temporal: the one backward kernel).
Bits (--md5, nothing timed): inputs from a seeded CPU generator per case, one JSON line per case with an md5 of every
output's bytes (spatial: o, lse, dq, dkv; temporal: out, grad) at the timed shapes, the edge shapes of
tests/test_training_gpu.py and temporal F in {1, 16, 17, 32} x head_dim in {8, 40, 64, 160}.  A refactor of the
attention kernels keeps every md5 equal.
Arguments: shape names to run (default: all)."""
import argparse
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_style_transfer_amd import kernels as K  # noqa: E402

BF = torch.bfloat16
SPATIAL = [("self32", 32, 10, 1024, 1024, 1), ("self16", 32, 20, 256, 256, 1), ("cross32", 32, 10, 1024, 77, 16),
           ("cross16", 32, 20, 256, 77, 16)]
TEMPORAL = [("temp64", 2, 16, 4096, 320), ("temp32", 2, 16, 1024, 640), ("temp16", 2, 16, 256, 1280)]
# --md5 only: tile-boundary shapes (nb, heads, Nq, Nk, kv_div) / (nclip, F, HW, C)
SPATIAL_EDGE = [(1, 1, 1, 65, 1), (1, 1, 129, 63, 1), (2, 1, 128, 64, 2), (4, 2, 33, 129, 4), (3, 1, 17, 300, 3)]
TEMPORAL_EDGE = [(1, 17, 3, 64), (2, 2, 5, 320), (1, 31, 1, 1280)] + \
    [(1, Fr, 3, 8 * hd) for Fr in (1, 16, 17, 32) for hd in (8, 40, 64, 160)]


def timeit(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def md5(t):
    return hashlib.md5(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


class Randn:
    """randn on the device (timing), or from a CPU generator seeded by the case name (--md5: the same bits for every
    build, whichever other cases ran)."""

    def __init__(self, name, dev, seeded):
        self.dev = dev
        self.g = torch.Generator().manual_seed(int(hashlib.md5(name.encode()).hexdigest()[:8], 16)) if seeded else None

    def __call__(self, *shape):
        if self.g is None:
            return torch.randn(*shape, device=self.dev).to(BF)
        return torch.randn(*shape, generator=self.g).to(BF).to(self.dev)


def spatial(name, nb, heads, Nq, Nk, kv_div, dev, bits):
    rn = Randn(name, dev, bits)
    C = heads * 64
    q = rn(nb * Nq, 3 * C)
    kv = rn(nb // kv_div * Nk, 2 * C)
    dout = rn(nb * Nq, C)
    if kv_div == 1 and Nq == Nk:
        qq, kk, vv = q[:, :C], q[:, C:2 * C], q[:, 2 * C:]
    else:
        qq, kk, vv = q[:, :C], kv[:, :C], kv[:, C:]
    out = torch.empty(nb * Nq, C, device=dev, dtype=BF)
    lse = torch.empty(nb * heads * Nq, device=dev, dtype=torch.float32)
    dq = torch.empty(nb * Nq, C, device=dev, dtype=BF)
    dkv = torch.empty(nb // kv_div * Nk, 2 * C, device=dev, dtype=BF)
    fwd = lambda: K.spatial_attention(qq, kk, vv, nb, heads, Nq, Nk, kv_div, out=out)  # noqa: E731
    bwd = lambda need: K.spatial_attention_bwd(qq, kk, vv, out, dout, lse, nb, heads, Nq, Nk, kv_div, dq=dq,  # noqa: E731
                                               dkv=dkv if need else None, need_dkv=need)
    K.spatial_attention(qq, kk, vv, nb, heads, Nq, Nk, kv_div, out=out, lse=lse)
    if bits:
        bwd(False)
        dq_only = md5(dq)
        bwd(True)
        torch.cuda.synchronize()
        print(json.dumps({"case": name, "md5": {"o": md5(out), "lse": md5(lse), "dq_only": dq_only, "dq": md5(dq),
                                                "dkv": md5(dkv)}}), flush=True)
        return
    unit = 2.0 * nb * heads * Nq * Nk * 64  # one MFMA product over the score tile
    for tag, fn, prods in (("", fwd, 2), ("_bwd_dq", lambda: bwd(False), 3), ("_bwd", lambda: bwd(True), 7)):
        ms = timeit(fn)
        print(json.dumps({"shape": name + tag, "us": round(ms * 1e3, 1), "tflops": round(prods * unit / ms / 1e9, 1)}),
              flush=True)


def temporal(name, nclip, Fr, HW, C, dev, bits):
    rn = Randn(name, dev, bits)
    rows = nclip * Fr * HW
    qkv = rn(rows, 3 * C)
    dout = rn(rows, C)
    out = torch.empty(rows, C, device=dev, dtype=BF)
    grad = torch.empty(rows, 3 * C, device=dev, dtype=BF)
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    fwd = lambda: K.temporal_attention(q, k, v, nclip, Fr, HW, 8, C // 8, out=out)  # noqa: E731
    bwd = lambda: K.temporal_attention_bwd(q, k, v, dout, nclip, Fr, HW, 8, C // 8, out=grad)  # noqa: E731
    if bits:
        fwd()
        bwd()
        torch.cuda.synchronize()
        print(json.dumps({"case": name, "md5": {"out": md5(out), "grad": md5(grad)}}), flush=True)
        return
    for tag, fn, passes in (("", fwd, 4), ("_bwd", bwd, 7)):
        ms = timeit(fn)
        print(json.dumps({"shape": name + tag, "us": round(ms * 1e3, 1),
                          "gbs": round(2.0 * passes * rows * C / ms / 1e6, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--md5", action="store_true")
    ap.add_argument("only", nargs="*")  # optional shape names (profiling passes)
    a = ap.parse_args()
    dev = torch.device("cuda")
    sp, tp = list(SPATIAL), list(TEMPORAL)
    if a.md5:
        sp += [("sa_%dx%dx%dx%d_div%d" % s, *s) for s in SPATIAL_EDGE]
        tp += [("ta_%dx%dx%dx%d" % t, *t) for t in TEMPORAL_EDGE]
    for name, *shape in sp:
        if not a.only or name in a.only:
            spatial(name, *shape, dev, a.md5)
    for name, *shape in tp:
        if not a.only or name in a.only:
            temporal(name, *shape, dev, a.md5)


if __name__ == "__main__":
    main()
