"""Sliding-window frame attention for clips longer than the motion modules' trained length (DESIGN.md "Long clips"):
the kernel against fp32 and against the unwindowed kernel's bits, its view contract, and the windowed motion module,
UNet, denoiser and frame-sharded forward.

References are fp32 torch written here (kernel level) or tests/test_temporal_context.py's windowed_motion_module,
which is tied to the golden-pinned oracle there.  Model-level bars compare the windowed error with the error the
UNWINDOWED path (existing code) makes against the oracle on the same weights: e_win <= 1.25 e_unwindowed + 2e-3, the
form tests/test_frame_shard.py uses.
"""
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def K():
    from video_style_transfer_amd import kernels
    return kernels


def rnd(*shape, scale=1.0, gen=None):
    return (torch.randn(*shape, generator=gen) * scale).to(BF16)


def errs(out, ref):
    out, ref = out.float().cpu(), ref.float().cpu()
    assert out.shape == ref.shape, (out.shape, ref.shape)
    assert torch.isfinite(out).all()
    err = out - ref
    return ((err.norm() / ref.norm().clamp_min(1e-12)).item(),
            (err.abs().max() / ref.abs().max().clamp_min(1e-12)).item())


def check(out, ref, rel_l2=5e-3, rel_max=1e-2, name=""):
    l2, mx = errs(out, ref)
    print(f"[context] {name}: rel_l2={l2:.3e} rel_max={mx:.3e}")
    assert l2 <= rel_l2 and mx <= rel_max, f"{name}: rel_l2={l2:.3e} rel_max={mx:.3e}"


def windowed_ref(K, qkv, table, nclip, Fr, HW, heads, d, L, S, weighting):
    """fp32 reference on the CPU: per window, q/k/v = bf16(float(qkv[s + j]) + table[j]) (the kernel's defined
    rounding point), softmax attention over the window's frames, weighted blend."""
    C = heads * d
    x = qkv.float().view(nclip, Fr, HW, 3 * C)
    w = torch.tensor(K.context_weights(L, weighting))
    num = torch.zeros(nclip, Fr, HW, C)
    den = torch.zeros(Fr)
    for s in K.context_windows(Fr, L, S):
        xw = x[:, s:s + L]
        if table is not None:
            xw = (xw + table.float().view(1, L, 1, 3 * C)).to(BF16).float()
        q, k, v = (xw[..., i * C:(i + 1) * C].reshape(nclip, L, HW, heads, d).permute(0, 2, 3, 1, 4) for i in range(3))
        o = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(d), -1) @ v       # [nclip, HW, heads, L, d]
        o = o.permute(0, 3, 1, 2, 4).reshape(nclip, L, HW, C)
        num[:, s:s + L] += o * w.view(1, L, 1, 1)
        den[s:s + L] += w
    return (num / den.view(1, Fr, 1, 1)).reshape(nclip * Fr * HW, C)


# ------------------------------------------------------------------ 1. kernel vs fp32
@pytest.mark.parametrize("nclip,Fr,HW,C,L,S,weighting,qs", [
    (2, 20, 5, 320, 16, 4, "pyramid", 1.0),
    (1, 23, 3, 640, 16, 4, "pyramid", 3.0),     # a tail window at 7
    (1, 40, 2, 1280, 16, 16, "flat", 3.0),      # heads of 160, tail at 24
    (1, 33, 4, 320, 32, 8, "pyramid", 3.0),     # two 16-frame tiles, windows 0 and 1
    (3, 19, 7, 64, 8, 3, "flat", 1.0),          # heads of 8, L below a tile
    (2, 24, 1, 128, 16, 4, "pyramid", 1.0),
])
def test_windowed_kernel_vs_fp32(cuda, K, nclip, Fr, HW, C, L, S, weighting, qs):
    """qs scales q: logit std 1 and 3 (peaked softmax).  Bars: test_kernels_gpu.test_temporal_attention's."""
    g = torch.Generator().manual_seed(nclip * Fr + C + L)
    heads, d = 8, C // 8
    qkv = rnd(nclip * Fr * HW, 3 * C, gen=g)
    qkv[:, :C] = (qkv[:, :C].float() * qs).to(BF16)
    table = torch.randn(L, 3 * C, generator=g) * 0.5
    qd, td = qkv.to(cuda), table.to(cuda)
    out = K.temporal_attention_windowed(qd[:, :C], qd[:, C:2 * C], qd[:, 2 * C:], td, nclip, Fr, HW, heads, d, L, S,
                                        weighting)
    ref = windowed_ref(K, qkv, table, nclip, Fr, HW, heads, d, L, S, weighting)
    check(out, ref, name=f"windowed {nclip}x{Fr}x{HW}x{C} L{L} S{S} {weighting}")


# ------------------------------------------------------------------ 2. bit anchors to the unwindowed kernel
@pytest.mark.parametrize("nclip,L,HW,C", [(2, 16, 8, 320), (1, 32, 4, 640)])
def test_windowed_bit_anchors(cuda, K, nclip, L, HW, C):
    g = torch.Generator().manual_seed(L + C)
    heads, d = 8, C // 8

    def cols(t):
        return t[:, :C], t[:, C:2 * C], t[:, 2 * C:]

    # one window, no table: the unwindowed kernel
    qkv = rnd(nclip * L * HW, 3 * C, gen=g).to(cuda)
    base = K.temporal_attention(*cols(qkv), nclip, L, HW, heads, d)
    one = K.temporal_attention_windowed(*cols(qkv), None, nclip, L, HW, heads, d, L, L, "flat")
    assert torch.equal(one, base)
    # one window, random table: the unwindowed kernel on bf16(qkv + T) formed in torch
    table = (torch.randn(L, 3 * C, generator=g) * 0.5).to(cuda)
    added = (qkv.float().view(nclip, L, HW, 3 * C) + table.view(1, L, 1, 3 * C)).to(BF16).view(nclip * L * HW, 3 * C)
    base_t = K.temporal_attention(*cols(added), nclip, L, HW, heads, d)
    one_t = K.temporal_attention_windowed(*cols(qkv), table, nclip, L, HW, heads, d, L, L, "flat")
    assert torch.equal(one_t, base_t)
    # F = 2L, S = L: two disjoint windows = twice the clips of L frames on the same buffer
    qkv2 = rnd(nclip * 2 * L * HW, 3 * C, gen=g).to(cuda)
    base2 = K.temporal_attention(*cols(qkv2), 2 * nclip, L, HW, heads, d)
    two = K.temporal_attention_windowed(*cols(qkv2), None, nclip, 2 * L, HW, heads, d, L, L, "flat")
    assert torch.equal(two, base2)


# ------------------------------------------------------------------ 3. view contract
def test_windowed_view_contract(cuda, K):
    """q/k/v column views of a NaN-padded [T, 3C] arena, out inside a sentinel arena, pos a slice of a NaN-filled
    buffer (tests/test_view_contract_gpu.py's harness, copied in small)."""
    nclip, Fr, HW, heads, d, L, S = 1, 20, 8, 2, 40, 16, 4
    C, T = heads * d, nclip * Fr * HW
    GT, GB, GC, SENT = 8, 320, 8, 0x7FA5
    g = torch.Generator().manual_seed(7)
    qkv = rnd(T, 3 * C, gen=g)
    table = torch.randn(L, 3 * C, generator=g) * 0.5

    dense_qkv, dense_t = qkv.to(cuda), table.to(cuda)
    dense_out = K.temporal_attention_windowed(dense_qkv[:, :C], dense_qkv[:, C:2 * C], dense_qkv[:, 2 * C:], dense_t,
                                              nclip, Fr, HW, heads, d, L, S, "pyramid")

    ld_in = GC + 3 * C + GC
    a_in = torch.full((GT + T + GB, ld_in), float("nan"), dtype=BF16, device=cuda)
    a_in[GT:GT + T, GC:GC + 3 * C] = dense_qkv
    v_in = a_in[GT:GT + T, GC:GC + 3 * C]
    pad = 3 * C                                           # one table row of NaN on each side
    pbuf = torch.full((pad + L * 3 * C + pad,), float("nan"), dtype=F32, device=cuda)
    pbuf[pad:pad + L * 3 * C] = dense_t.reshape(-1)
    v_pos = pbuf[pad:pad + L * 3 * C].view(L, 3 * C)
    ld_out = GC + C + GC
    a_out = torch.empty((GT + T + GB, ld_out), dtype=BF16, device=cuda)
    a_out.view(torch.int16).fill_(SENT)
    v_out = a_out[GT:GT + T, GC:GC + C]

    ret = K.temporal_attention_windowed(v_in[:, :C], v_in[:, C:2 * C], v_in[:, 2 * C:], v_pos, nclip, Fr, HW, heads, d,
                                        L, S, "pyramid", out=v_out)
    assert ret.data_ptr() == v_out.data_ptr()
    same = a_out.view(torch.int16) == SENT
    outside = ~same
    outside[GT:GT + T, GC:GC + C] = False
    assert not outside.any(), "guard band written"
    inner = a_out[GT:GT + T, GC:GC + C]
    assert not (same[GT:GT + T, GC:GC + C] | ~torch.isfinite(inner.float())).any(), "view unwritten or non-finite"
    assert torch.equal(inner.contiguous().view(torch.int16), dense_out.view(torch.int16))
    check(inner, windowed_ref(K, qkv, table, nclip, Fr, HW, heads, d, L, S, "pyramid"), name="windowed view")

    VstError = K._lib.VstError
    args = (v_in[:, :C], v_in[:, C:2 * C], v_in[:, 2 * C:], v_pos, nclip, Fr, HW, heads, d, L, S, "pyramid")
    before = a_out.clone()
    with pytest.raises(VstError):
        K.temporal_attention_windowed(*args, out=torch.empty((T, C), dtype=F32, device=cuda))       # dtype
    with pytest.raises(VstError):
        K.temporal_attention_windowed(*args, out=a_out[GT:GT + T + 1, GC:GC + C])                   # shape
    with pytest.raises(VstError):
        K.temporal_attention_windowed(*args, out=torch.empty((T, 2 * C), dtype=BF16, device=cuda)[:, ::2])  # stride
    torch.cuda.synchronize()
    assert torch.equal(a_out.view(torch.int16), before.view(torch.int16))


# ------------------------------------------------------------------ 4. the motion module
def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm()).item()


def _device_motion_module(P, C, cuda):
    from video_style_transfer_amd.unet_motion import MotionModule
    mm = MotionModule(C)
    mm.load_state_dict({k[len("mm."):]: v for k, v in P.items()})
    mm.to(cuda)
    for p in mm.parameters():  # bf16 weights, fp32 PE buffer: as utils.build_unet leaves them
        p.data = p.data.to(BF16)
    return mm.requires_grad_(False)


def _tokens(x):  # (B*F, C, H, W) -> rows (b*F + f)*HW + p
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


@pytest.mark.parametrize("C", [64, 320])
def test_windowed_motion_module_vs_fp32(cuda, K, C):
    """MotionModule.run with TemporalContext(16, 4) at F = 20 against the fp32 windowed reference.  Yardstick: the
    UNWINDOWED module's error against oracle.unet.motion_module at F = 16 on the same weights (existing code)."""
    from oracle import unet as OU
    from test_temporal_context import motion_params, windowed_motion_module
    from video_style_transfer_amd.unet_motion import ForwardOptions, FwdCtx, TemporalContext
    B, Fr, H, W = 2, 20, 4, 4
    P = motion_params(C, seed=C)
    mm = _device_motion_module(P, C, cuda)
    x = torch.randn(B * Fr, C, H, W, generator=torch.Generator().manual_seed(C + 1)).to(BF16).float()
    x16 = x.view(B, Fr, C, H, W)[:, :16].reshape(B * 16, C, H, W)
    tc = TemporalContext(16, 4)

    out16 = mm.run(_tokens(x16).to(cuda, BF16), B * 16, H, W, FwdCtx(B, 16, None, None, {}))
    e16 = rel(out16, _tokens(OU.motion_module(P, "mm", x16, 16)))
    windowed = ForwardOptions(temporal_context=tc)
    out = mm.run(_tokens(x).to(cuda, BF16), B * Fr, H, W, FwdCtx(B, Fr, None, None, {}, opts=windowed))
    e_win = rel(out, _tokens(windowed_motion_module(P, "mm", x, Fr, 16, 4, "pyramid")))
    print(f"[context] motion module C={C}: windowed F=20 rel_l2={e_win:.3e}, unwindowed F=16 rel_l2={e16:.3e}")
    assert e_win <= 1.25 * e16 + 2e-3, (e_win, e16)
    # an inactive context (F <= length) launches exactly what no context launches
    same = mm.run(_tokens(x16).to(cuda, BF16), B * 16, H, W, FwdCtx(B, 16, None, None, {}, opts=windowed))
    assert torch.equal(same, out16)


# ------------------------------------------------------------------ 5. the UNet
@pytest.fixture(scope="module")
def tiny(cuda):
    from test_parity_gpu import _setup
    from video_style_transfer_amd.utils import build_unet
    cfg, sd, lat, enc, pooled, tids = _setup("tiny", 20, 16)
    unet = build_unet(cfg, state_dict=sd, device=cuda)
    kw = dict(added_cond_kwargs={"text_embeds": pooled.to(cuda), "time_ids": tids.to(cuda)})
    return dict(cfg=cfg, sd=sd, lat=lat, enc=enc, pooled=pooled, tids=tids, unet=unet, kw=kw)


def test_windowed_unet_vs_oracle(cuda, tiny, monkeypatch):
    """Tiny UNet, F = 20, 16x16 latent, B = 2, context (16, 4) against oracle.unet.unet_forward with its motion
    module replaced (here, by monkeypatch) by the windowed fp32 reference; e16: the unwindowed F = 16 error."""
    import oracle.unet as OU
    from test_temporal_context import windowed_motion_module
    from video_style_transfer_amd.unet_motion import TemporalContext
    cfg, sd, lat, enc, pooled, tids, unet, kw = (tiny[k] for k in ("cfg", "sd", "lat", "enc", "pooled", "tids", "unet",
                                                                   "kw"))
    t = torch.tensor([761.0, 761.0])
    tc = TemporalContext(16, 4)
    lat16 = lat[:, :, :16].contiguous()
    ref16 = OU.unet_forward(sd, cfg.to_dict(), lat16, t, enc, pooled, tids)
    out16 = unet(lat16.to(cuda), t.to(cuda), enc.to(cuda), **kw).sample
    e16 = rel(out16, ref16)
    monkeypatch.setattr(OU, "motion_module", lambda P, name, x, num_frames, heads=8, lora=None:
                        windowed_motion_module(P, name, x, num_frames, 16, 4, "pyramid", heads))
    ref = OU.unet_forward(sd, cfg.to_dict(), lat, t, enc, pooled, tids)
    monkeypatch.undo()
    out = unet(lat.to(cuda), t.to(cuda), enc.to(cuda), temporal_context=tc, **kw).sample
    e = rel(out, ref)
    print(f"[context] UNet tiny: windowed F=20 rel_l2={e:.3e}, unwindowed F=16 rel_l2={e16:.3e}")
    assert e <= 3e-2 and e <= 1.25 * e16 + 2e-3, (e, e16)
    # F = 16 with a context of length 16: the launches of the call without one
    same = unet(lat16.to(cuda), t.to(cuda), enc.to(cuda), temporal_context=tc, **kw).sample
    assert torch.equal(same, out16)


# ------------------------------------------------------------------ 6. the denoiser
def test_windowed_denoiser_graph_equals_eager(cuda, tiny):
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser
    unet, enc, pooled = tiny["unet"], tiny["enc"], tiny["pooled"]
    outs = {}
    for use_graph in (True, False):
        den = AnimateDiffDenoiser(unet, 20, 128, 128, num_inference_steps=10, device=cuda, use_graph=use_graph,
                                  context_length=16, context_stride=4)
        den.set_prompt_embeds(enc[1:2], pooled[1:2], enc[0:1], pooled[0:1])
        den.init_latents(seed=3)
        outs[use_graph] = den.run_steps(2).clone()
        assert (den.graph is not None) == use_graph
    assert torch.isfinite(outs[True]).all()
    assert torch.equal(outs[True], outs[False])


def test_long_clip_without_context_refused_before_any_launch(cuda, K, tiny):
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser
    unet, enc, kw = tiny["unet"], tiny["enc"], tiny["kw"]
    lat40 = torch.zeros(2, 4, 40, 16, 16, device=cuda)
    t = torch.tensor([761.0, 761.0], device=cuda)
    K.profile_launches(True)
    try:
        with pytest.raises(K._lib.VstError, match="context_length"):
            AnimateDiffDenoiser(unet, 40, 128, 128, num_inference_steps=10, device=cuda)
        with pytest.raises(K._lib.VstError, match="context_length"):
            unet(lat40, t, enc.to(cuda), **kw)
        assert K.collect_launches() == []
    finally:
        K.profile_launches(False)
    AnimateDiffDenoiser(unet, 40, 128, 128, num_inference_steps=10, device=cuda, context_length=16)  # accepted


def test_training_refuses_context(cuda, tiny):
    from video_style_transfer_amd.autograd import unet_train_tokens
    from video_style_transfer_amd.train import TrainStep
    from video_style_transfer_amd.unet_motion import TemporalContext
    tc = TemporalContext(16, 4)
    with pytest.raises(NotImplementedError, match="context_length"):
        unet_train_tokens(tiny["unet"], None, 2, 20, 16, 16, None, None, temporal_context=tc)
    step = TrainStep(tiny["unet"], None, None, temporal_context=tc)
    with pytest.raises(NotImplementedError, match="context_length"):
        step._loss(torch.zeros(1, 4, 20, 16, 16, device=cuda), None, None, None, None)


# ------------------------------------------------------------------ 7. frame sharding
def _shard_worker(rank, world, port, exchange):
    """One of two gloo ranks on one GPU: tiny UNet, the CFG pair of a 24-frame clip (12 frames per rank), context
    (16, 4); this rank's sharded forward must be the unsharded forward's bits for its frames."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from test_parity_gpu import _setup
        from video_style_transfer_amd.frame_shard import FrameShard
        from video_style_transfer_amd.unet_motion import TemporalContext
        from video_style_transfer_amd.utils import build_unet
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        Fr = 24
        cfg, sd, lat, enc, pooled, tids = _setup("tiny", Fr, 16, seed=9, B=2)
        unet = build_unet(cfg, state_dict=sd, device=dev)
        kw = dict(added_cond_kwargs={"text_embeds": pooled.to(dev), "time_ids": tids.to(dev)},
                  temporal_context=TemporalContext(16, 4))
        t = torch.tensor([421.0, 421.0])
        full = unet(lat.to(dev), t.to(dev), enc.to(dev), fusion_world=world, **kw).sample.float().cpu()
        sh = FrameShard(exchange=exchange)
        Fl, f0 = sh.local_frames(Fr)
        part = unet(lat[:, :, f0:f0 + Fl].contiguous().to(dev), t.to(dev), enc.to(dev), frame_shard=sh,
                    **kw).sample.float().cpu()
        same = torch.equal(part, full[:, :, f0:f0 + Fl]) and bool(torch.isfinite(part).all())
        print(f"[context] {exchange} rank {rank}: frames {f0}..{f0 + Fl - 1} sharded == unsharded: {same} "
              f"(max |diff| {(part - full[:, :, f0:f0 + Fl]).abs().max().item():.3e})", flush=True)
        return 0 if same else 1
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("exchange", ["all_to_all", "all_gather"])
def test_windowed_frame_shard_two_ranks_one_gpu(cuda, exchange):
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    world = 2
    procs = [subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__),
                               "--shard-worker", str(r), str(world), str(port), exchange],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = [p.communicate()[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        print(o[-1500:])
        assert p.returncode == 0, f"rank {r} exited {p.returncode}: {o[-1500:]}"


if __name__ == "__main__" and len(sys.argv) == 6 and sys.argv[1] == "--shard-worker":
    sys.exit(_shard_worker(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]))
