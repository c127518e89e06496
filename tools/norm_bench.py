"""The A/B tool for csrc/norm.hip: every norm entry point at the 16x512^2 CFG-pair step shapes and at edge shapes
(odd row counts, channel concats, every LayerNorm kernel choice), one JSON line per case with the device time and an
md5 of every output's bytes.  Inputs come from a seeded CPU generator, so two builds see the same bits:

    bash tools/ab_lib.sh                                   # the committed sources -> abx/libvst_old.so
    VST_LIB_AB=abx/libvst_old.so python tools/norm_bench.py > old.jsonl; python tools/norm_bench.py > new.jsonl

A refactor of norm.hip keeps every md5 equal.  Arguments: substrings of the case names to run (default: all).  The
LayerNorm cases under VST_LN_GENERIC=1 (read once per process) run in a child process."""
import hashlib
import json
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_style_transfer_amd import kernels as K  # noqa: E402

BF16 = torch.bfloat16
DEV = "cuda"

# (ns, rps, C1, C2, silu): the step's GroupNorms, then the edge shapes
GN = [(32, 4096, 320, 0, 1), (32, 4096, 320, 320, 1), (32, 4096, 640, 320, 1), (32, 1024, 640, 0, 1),
      (32, 1024, 640, 640, 1), (32, 256, 1280, 0, 1), (32, 256, 1280, 1280, 1), (32, 1024, 640, 0, 0),
      (32, 256, 1280, 0, 0),
      (2, 9, 64, 0, 0), (5, 77, 640, 320, 1), (3, 700, 4096, 0, 0)]
# (P, nclip, F, HW, C): motion-module GroupNorm as frame partials + apply (P ranks' partials, rank 0's rows applied)
GN_PARTS = [(1, 2, 16, 4096, 320), (1, 2, 16, 1024, 640), (1, 2, 16, 256, 1280), (2, 3, 4, 100, 64), (8, 1, 32, 576, 640)]
GN_BWD = [(3, 77, 64, 1), (4, 256, 640, 1)]   # (ns, rps, C, silu)
# (rows, C, pe): the step's LayerNorms, then the edge shapes (C = 64 / 768 / 2048: generic kernel, 1 / 2 / 4 chunks)
LN = [(131072, 320, 0), (32768, 640, 0), (8192, 1280, 0),
      (300, 320, 0), (513, 640, 1), (64, 1280, 1), (10, 64, 0), (9, 768, 1), (9, 2048, 0)]
LN_GENERIC = [(300, 320, 0), (513, 640, 1), (64, 1280, 1)]  # again under VST_LN_GENERIC=1
LN_LORA = [(rows, C, R) for rows, C in ((131072, 320), (32768, 640), (8192, 1280)) for R in (16, 64)] + \
    [(77, 640, 48), (33, 1280, 64)]  # (rows, C, R)
LN_BWD = [(300, 640), (64, 64), (1024, 1280)]  # each with and without the affine gradients


def timeit(fn, reps=20):
    """Device time per call: `reps` calls captured in one HIP graph (eager launches of these 10-50 us
    kernels are bounded by the Python launch path, not the GPU)."""
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


def md5(t):
    return hashlib.md5(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


class Case:
    """Inputs of one case from its own seeded CPU generator (a case's bits do not depend on which others ran)."""

    def __init__(self, name):
        self.name = name
        self.g = torch.Generator(device="cpu").manual_seed(int(hashlib.md5(name.encode()).hexdigest()[:8], 16))

    def bf(self, *shape, shift=0.0):
        return (torch.randn(*shape, generator=self.g) + shift).to(BF16).to(DEV)

    def affine(self, C):
        return ((torch.rand(C, generator=self.g) + 0.5).to(DEV), (torch.randn(C, generator=self.g) * 0.1).to(DEV))

    def report(self, fn, nbytes):
        """fn() -> dict of named output tensors; timed, then hashed from a fresh call."""
        us = timeit(fn)
        outs = fn()
        torch.cuda.synchronize()
        print(json.dumps({"case": self.name, "us": round(us, 2), "gbs": round(nbytes / us / 1e3, 1),
                          "md5": {k: md5(v) for k, v in outs.items()}}), flush=True)


def cases(generic):
    """(name, runner) for every case; `generic`: only the cases that run under VST_LN_GENERIC=1."""
    tag = "ln_generic" if generic else "ln"

    def ln(rows, C, pe):
        def run(c):
            x, (gam, bet) = c.bf(rows, C), c.affine(C)
            tab = torch.randn(32, C, generator=c.g).to(DEV) if pe else None
            out = torch.empty_like(x)
            c.report(lambda: {"y": K.layer_norm(x, gam, bet, 1e-5, pe=tab, pe_div=4, pe_mod=8, out=out)},
                     2 * 2.0 * rows * C)
        return f"{tag}_{rows}x{C}" + ("_pe" if pe else ""), run

    if generic:
        return [ln(*a) for a in LN_GENERIC]

    def gn(ns, rps, C1, C2, act):
        def run(c):
            x1, x2 = c.bf(ns * rps, C1, shift=0.5), (c.bf(ns * rps, C2) if C2 else None)
            gam, bet = c.affine(C1 + C2)
            out = torch.empty(ns * rps, C1 + C2, dtype=BF16, device=DEV)
            c.report(lambda: {"y": K.group_norm(x1, ns, rps, 32, 1e-5, gam, bet, silu=bool(act), x2=x2, out=out)},
                     3 * 2.0 * ns * rps * (C1 + C2))
        return f"gn_{ns}x{rps}x{C1}+{C2}" + ("_silu" if act else ""), run

    def gn_parts(P, nclip, Fr, HW, C):
        def run(c):
            Fl = Fr // P
            shards = [c.bf(nclip * Fl * HW, C, shift=0.3) for _ in range(P)]
            gam, bet = c.affine(C)
            out = torch.empty_like(shards[0])
            part = torch.empty(P, nclip * Fl, int(K._lib.load().vst_groupnorm_frame_chunks(HW)), 32, 2,
                               dtype=torch.float32, device=DEV)

            def fn():
                for r in range(P):
                    K.group_norm_frame_partials(shards[r], nclip * Fl, HW, 32, out=part[r])
                return {"part": part, "y": K.group_norm_apply_partials(shards[0], nclip, Fl, HW, 32, 1e-6, gam, bet,
                                                                       part, P, out=out)}
            c.report(fn, (P + 2) * 2.0 * nclip * Fl * HW * C)
        return f"gn_parts_P{P}_{nclip}x{Fr}x{HW}x{C}", run

    def gn_bwd(ns, rps, C, act):
        def run(c):
            x, g = c.bf(ns * rps, C, shift=0.5), c.bf(ns * rps, C)
            gam, bet = c.affine(C)
            c.report(lambda: dict(zip(("dx", "dgamma", "dbeta"),
                                      K.group_norm_bwd(x, g, ns, rps, 32, 1e-5, gam, bet, silu=bool(act)))),
                     5 * 2.0 * ns * rps * C)
        return f"gn_bwd_{ns}x{rps}x{C}" + ("_silu" if act else ""), run

    def ln_lora(rows, C, R):
        def run(c):
            x, (gam, bet) = c.bf(rows, C), c.affine(C)
            A = (torch.randn(R, C, generator=c.g) * C ** -0.5).to(BF16).to(DEV)
            out, u = torch.empty_like(x), torch.empty(rows, R, dtype=BF16, device=DEV)
            c.report(lambda: dict(zip(("y", "u"), K.layer_norm_lora(x, gam, bet, 1e-5, A, out=out, u=u))),
                     2 * 2.0 * rows * C + 2.0 * rows * R)
        return f"ln_lora_{rows}x{C}_R{R}", run

    def ln_bwd(rows, C, affine):
        def run(c):
            x, g = c.bf(rows, C), c.bf(rows, C)
            gam, _ = c.affine(C)
            keys = ("dx", "dgamma", "dbeta") if affine else ("dx",)
            c.report(lambda: dict(zip(keys, K.layer_norm_bwd(x, g, gam, 1e-5, need_affine=affine))),
                     3 * 2.0 * rows * C)
        return f"ln_bwd_{rows}x{C}" + ("_affine" if affine else ""), run

    return ([gn(*a) for a in GN] + [gn_parts(*a) for a in GN_PARTS] + [gn_bwd(*a) for a in GN_BWD] +
            [ln(*a) for a in LN] + [ln_lora(*a) for a in LN_LORA] +
            [ln_bwd(r, C, aff) for r, C in LN_BWD for aff in (True, False)])


def main():
    generic = "VST_LN_GENERIC" in os.environ
    only = sys.argv[1:]
    for name, run in cases(generic):
        if not only or any(o in name for o in only):
            run(Case(name))
    if not generic:  # the switch is read once per process: a fresh child for the cases under it
        sys.stdout.flush()
        sys.exit(subprocess.run([sys.executable, os.path.abspath(__file__)] + only,
                                env=dict(os.environ, VST_LN_GENERIC="1")).returncode)


if __name__ == "__main__":
    main()
