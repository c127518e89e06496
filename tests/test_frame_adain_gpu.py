"""StyleAligned AdaIN of q/k/v to the anchor frame: the kernel against fp64, its view contract, its
independence of the batch and its determinism, and the option through the processor, the UNet and the denoiser.

The fp64 reference is tests/test_frame_adain.py's adain_ref (checked there against closed forms).  Kernel gates:
  output      |got - ref| <= 2^-7 |ref| + 2^-8 sd_anchor   (one bf16 ulp of the result, plus a term for results near 0);
  statistics  |mu - ref| <= 1e-5 (|mu| + sd),  |sd - ref| <= 1e-5 sd   (centred fp32 sums; a one-pass sum of squares
              misses the second on the case with mean 8, sd 0.25).
The model-level gate is tests/test_cross_frame_gpu.py's: e <= 3e-2 and e <= 1.25 e0 + 2e-3, e0 the plain forward's error
against the unpatched oracle on the same inputs.
"""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def K():
    from video_style_transfer_amd import kernels
    return kernels


def make_x(nclip, Fr, N, C, anchor, ms, ss, seed=0):
    """bf16 [nclip*Fr*N, C]: per (clip, frame, column) a mean around ms and an sd around ss; one 8-column block constant
    over a whole non-anchor frame (F = 1: over the frame)."""
    g = torch.Generator().manual_seed(seed + N + C)
    mean = ms * (1.0 + 0.5 * torch.randn(nclip, Fr, 1, C, generator=g))
    sd = ss * (0.5 + torch.rand(nclip, Fr, 1, C, generator=g))
    x = torch.randn(nclip, Fr, N, C, generator=g) * sd + mean
    x[0, (anchor + 1) % Fr, :, 8:16] = mean[0, (anchor + 1) % Fr, :, 8:16]
    return x.to(BF16).reshape(nclip * Fr * N, C)


def gates(x, got, stats, nclip, Fr, N, anchor, name=""):
    """The kernel gates of the module docstring, each figure printed before it is asserted."""
    from test_frame_adain import adain_ref
    C = x.shape[1]
    ref, mu, sd = adain_ref(x.cpu(), nclip, Fr, N, anchor)
    got = got.cpu()
    stats = stats.cpu().double().view(nclip, Fr, 2, C)
    assert torch.isfinite(got.float()).all() and torch.isfinite(stats).all()
    g4, x4 = got.view(nclip, Fr, N, C), x.cpu().view(nclip, Fr, N, C)
    assert torch.equal(g4[:, anchor], x4[:, anchor]), "anchor rows changed"
    bound = 2.0 ** -7 * ref.abs() + (2.0 ** -8 * sd[:, anchor])[:, None, None].expand(nclip, Fr, N, C).reshape(ref.shape)
    worst = ((got.double() - ref).abs() / bound).max().item()
    e_mu = ((stats[:, :, 0] - mu).abs() / (mu.abs() + sd)).max().item()
    e_sd = ((stats[:, :, 1] - sd).abs() / sd).max().item()
    print(f"[frame-adain] {name}: output worst/bound={worst:.3f} mu err={e_mu:.2e} sd err={e_sd:.2e}")
    assert worst <= 1.0, (name, worst)
    assert e_mu <= 1e-5 and e_sd <= 1e-5, (name, e_mu, e_sd)
    # the constant block: sd = sqrt(eps), and the anchor's mean (the kernel's own, gated above) rounded once; no NaN
    f = (anchor + 1) % Fr
    if f != anchor:
        want = stats[0, anchor, 0, 8:16].float().to(BF16)
        assert torch.equal(g4[0, f, :, 8:16], want.expand(N, 8)), "constant column"
    assert (stats[0, f, 1, 8:16] - 1e-5 ** 0.5).abs().max() <= 1e-5 * 1e-5 ** 0.5


# ------------------------------------------------------------------ 1. kernel vs fp64
CASES = [(2, 3, 16, 72, 0, 0.0, 1.0),       # partial last slab
         (1, 4, 25, 128, 2, 4.0, 0.5),      # odd N, anchor inside the clip
         (2, 2, 2, 64, 1, 0.0, 1.0),        # the smallest N, anchor = last frame
         (1, 3, 256, 192, 0, -3.0, 2.0),    # the 16^2 level's N, three slabs
         (1, 2, 1024, 128, 0, 8.0, 0.25)]   # the 32^2 level's N (four row chunks), |mean| >> sd


@pytest.mark.parametrize("nclip,Fr,N,C,anchor,ms,ss", CASES)
def test_kernel_vs_fp64(cuda, K, nclip, Fr, N, C, anchor, ms, ss):
    x = make_x(nclip, Fr, N, C, anchor, ms, ss)
    xd = x.to(cuda)
    stats = K.frame_adain(xd, nclip, Fr, N, anchor)
    assert tuple(stats.shape) == (nclip * Fr, 2, C) and stats.dtype == F32
    gates(x, xd, stats, nclip, Fr, N, anchor, name=str((nclip, Fr, N, C, anchor, ms, ss)))


# ------------------------------------------------------------------ 2. view contract
def test_view_contract(cuda, K):
    """x the column view [64, 64 + C) of a wider buffer with guard rows before and after, stats a slice of a longer
    array; everything outside is NaN: afterwards the poison is bit-intact and the result has the contiguous call's
    bits."""
    nclip, Fr, N, C, anchor = 2, 3, 40, 72, 1
    T, GT, GB, C0, LD, GS = nclip * Fr * N, 8, 40, 64, 64 + 72 + 56, 64
    x = make_x(nclip, Fr, N, C, anchor, 2.0, 0.5, seed=3)
    dense = x.to(cuda)
    dense_stats = K.frame_adain(dense, nclip, Fr, N, anchor)

    arena = torch.full((GT + T + GB, LD), float("nan"), dtype=BF16, device=cuda)
    arena[GT:GT + T, C0:C0 + C] = x.to(cuda)
    view = arena[GT:GT + T, C0:C0 + C]
    ns = nclip * Fr * 2 * C
    sarena = torch.full((GS + ns + GS,), float("nan"), dtype=F32, device=cuda)
    sview = sarena[GS:GS + ns].view(nclip * Fr, 2, C)
    before, sbefore = arena.clone(), sarena.clone()

    ret = K.frame_adain(view, nclip, Fr, N, anchor, stats=sview)
    assert ret.data_ptr() == sview.data_ptr()
    outside = torch.ones_like(arena, dtype=torch.bool)
    outside[GT:GT + T, C0:C0 + C] = False
    assert torch.equal(arena.view(torch.int16)[outside], before.view(torch.int16)[outside]), "x's surroundings written"
    soutside = torch.ones_like(sarena, dtype=torch.bool)
    soutside[GS:GS + ns] = False
    assert torch.equal(sarena.view(torch.int32)[soutside], sbefore.view(torch.int32)[soutside]), "stats' guards written"
    assert torch.equal(view.contiguous().view(torch.int16), dense.view(torch.int16))
    assert torch.equal(sview.view(torch.int32), dense_stats.view(torch.int32))
    gates(x, view.contiguous(), sview, nclip, Fr, N, anchor, name="view")

    # operands the wrapper refuses: nothing is launched, nothing is written
    VstError = K._lib.VstError
    snap = arena.clone()
    with pytest.raises(VstError, match="frame_adain: x "):
        K.frame_adain(arena[GT:GT + T, C0 + 4:C0 + 4 + C], nclip, Fr, N, anchor)          # base not 16-byte aligned
    with pytest.raises(VstError, match="frame_adain: x "):
        K.frame_adain(arena[GT:GT + T, C0:C0 + C + 4], nclip, Fr, N, anchor)              # C % 8
    with pytest.raises(VstError, match="frame_adain: stats "):
        K.frame_adain(view, nclip, Fr, N, anchor, stats=sarena[GS + 1:GS + 1 + ns].view(nclip * Fr, 2, C))
    with pytest.raises(VstError, match="frame_adain: anchor "):
        K.frame_adain(view, nclip, Fr, N, Fr)
    torch.cuda.synchronize()
    assert torch.equal(arena.view(torch.int16), snap.view(torch.int16))


# ------------------------------------------------------------------ 3. independence and determinism
def test_independence_and_determinism(cuda, K):
    nclip, Fr, N, C, anchor = 2, 3, 300, 136, 2
    x = make_x(nclip, Fr, N, C, anchor, 1.0, 1.0, seed=5).to(cuda)
    a, b = x.clone(), x.clone()
    sa, sb = K.frame_adain(a, nclip, Fr, N, anchor), K.frame_adain(b, nclip, Fr, N, anchor)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and torch.equal(sa.view(torch.int32), sb.view(torch.int32))
    assert not torch.equal(a, x)
    # a clip's bits do not depend on the clips beside it
    T = Fr * N
    for c in range(nclip):
        one = x[c * T:(c + 1) * T].clone()
        s1 = K.frame_adain(one, 1, Fr, N, anchor)
        assert torch.equal(one.view(torch.int16), a[c * T:(c + 1) * T].view(torch.int16)), c
        assert torch.equal(s1.view(torch.int32), sa[c * Fr:(c + 1) * Fr].view(torch.int32)), c
    # F = 1: every frame its own anchor; the statistics are written, x is not
    one = x.clone()
    s1 = K.frame_adain(one, nclip * Fr, 1, N, 0)
    assert torch.equal(one.view(torch.int16), x.view(torch.int16))
    assert torch.equal(s1.view(torch.int32), sa.view(torch.int32))


# ------------------------------------------------------------------ 4. processor / UNet
def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm()).item()


@pytest.fixture(scope="module")
def tiny(cuda):
    from test_parity_gpu import _setup
    from video_style_transfer_amd.utils import build_unet
    cfg, sd, lat, enc, pooled, tids = _setup("tiny", 20, 16)
    unet = build_unet(cfg, state_dict=sd, device=cuda)
    kw = dict(added_cond_kwargs={"text_embeds": pooled.to(cuda), "time_ids": tids.to(cuda)})
    return dict(cfg=cfg, sd=sd, lat=lat, enc=enc, pooled=pooled, tids=tids, unet=unet, kw=kw)


def profiled(K, fn):
    K.profile_launches(True)
    try:
        out = fn()
        kinds = [r[0] for r in K.collect_launches()]
    finally:
        K.profile_launches(False)
    return out, kinds


def test_unet_vs_oracle(cuda, K, tiny, monkeypatch):
    """Tiny UNet, B = 2, F = 4, 16x16 latent whose frames differ in gain and offset, cross_frame ("first",) with
    adain="qkv", against oracle.unet.unet_forward whose spatial self-attention is replaced (here, by monkeypatch) by
    projection -> reference AdaIN -> the extended fp32 attention."""
    import oracle.unet as OU
    from test_cross_frame import frames_ref
    from test_frame_adain import adain_ref
    from video_style_transfer_amd.unet_motion import CrossFrameAttention
    cfg, sd, lat, enc, pooled, tids, unet, kw = (tiny[k] for k in ("cfg", "sd", "lat", "enc", "pooled", "tids", "unet",
                                                                   "kw"))
    Fr, sources = 4, ("first",)
    t = torch.tensor([761.0, 761.0])
    gain = torch.tensor([1.0, 0.25, 2.0, 0.5]).view(1, 1, Fr, 1, 1)
    offset = torch.tensor([0.0, 1.0, -1.0, 0.5]).view(1, 1, Fr, 1, 1)
    lat4 = (lat[:, :, :Fr] * gain + offset).to(BF16).float().contiguous()
    ref0 = OU.unet_forward(sd, cfg.to_dict(), lat4, t, enc, pooled, tids)

    def run(cross_frame=None, latents=lat4):
        return unet(latents.to(cuda), t.to(cuda), enc.to(cuda), cross_frame=cross_frame, **kw).sample

    out0 = run()
    e0 = rel(out0, ref0)

    orig = OU.attention

    def oracle_with(blocks):
        patched = []

        def extended(P, name, x, enc_, heads, lora):
            if enc_ is not None or "motion_modules" in name:
                return orig(P, name, x, enc_, heads, lora)
            patched.append(name)

            def pr(n, t_):
                return OU.proj(P, f"{name}.{'to_out.0' if n == 'to_out' else n}", t_, lora)
            BF, N, _ = x.shape
            qkv = [pr(n, x).reshape(BF * N, -1) for n in ("to_q", "to_k", "to_v")]
            assert qkv[0].shape[1] == heads * 64
            for i in range(blocks):
                qkv[i] = adain_ref(qkv[i], BF // Fr, Fr, N, 0)[0].float()
            return pr("to_out", frames_ref(*qkv, BF // Fr, Fr, N, heads, sources).view(BF, N, -1))

        monkeypatch.setattr(OU, "attention", extended)
        try:
            return OU.unet_forward(sd, cfg.to_dict(), lat4, t, enc, pooled, tids), patched
        finally:
            monkeypatch.undo()

    ref_none, _ = oracle_with(0)
    ref_qk, _ = oracle_with(2)
    ref, patched = oracle_with(3)
    assert patched and all(n.endswith(".attn1") for n in patched)

    out, kinds = profiled(K, lambda: run(CrossFrameAttention(sources, adain="qkv")))
    e = rel(out, ref)
    print(f"[frame-adain] UNet tiny F=4: adain=qkv rel_l2={e:.3e}, plain rel_l2={e0:.3e}")
    # one AdaIN per patched block, each right before its attention
    pair = [k for k in kinds if k in ("frame_adain", "spatial_attention_frames")]
    assert pair == ["frame_adain", "spatial_attention_frames"] * len(patched), (pair, len(patched))
    assert e <= 3e-2 and e <= 1.25 * e0 + 2e-3, (e, e0)

    # the option does something, on frames > 0, here and in the reference
    out_none, kinds_none = profiled(K, lambda: run(CrossFrameAttention(sources)))
    out_qk = run(CrossFrameAttention(sources, adain="qk"))
    d, d_ref = rel(out[:, :, 1:], out_none[:, :, 1:]), rel(ref[:, :, 1:], ref_none[:, :, 1:])
    d_qk, d_qk_ref = rel(out_qk[:, :, 1:], out_none[:, :, 1:]), rel(ref_qk[:, :, 1:], ref_none[:, :, 1:])
    e_qk = rel(out_qk, ref_qk)
    print(f"[frame-adain] qkv vs none: {d:.3e} (oracle {d_ref:.3e}); qk vs none: {d_qk:.3e} (oracle {d_qk_ref:.3e}); "
          f"adain=qk rel_l2={e_qk:.3e}")
    assert d > 2e-2 and d_ref > 2e-2, (d, d_ref)
    assert d_qk > 5e-3, d_qk
    assert e_qk <= 3e-2 and e_qk <= 1.25 * e0 + 2e-3, (e_qk, e0)
    # adain=None is the cross-frame attention as it was: no AdaIN launch, the bits of the plain sources
    assert "frame_adain" not in kinds_none
    assert torch.equal(out_none, run(sources))
    # a single-frame clip launches no AdaIN and is the plain forward, bit for bit
    lat1 = lat4[:, :, :1].contiguous()
    one = run(None, lat1)
    one_cf, kinds = profiled(K, lambda: run(CrossFrameAttention(("first", "prev"), adain="qkv"), lat1))
    assert "frame_adain" not in kinds and "spatial_attention_frames" not in kinds and torch.equal(one_cf, one)


# ------------------------------------------------------------------ 5. the denoiser
@pytest.mark.parametrize("Fr,context", [(4, None), (20, 16)])
def test_denoiser_graph_equals_eager(cuda, tiny, Fr, context):
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser
    from video_style_transfer_amd.unet_motion import CrossFrameAttention
    unet, enc, pooled = tiny["unet"], tiny["enc"], tiny["pooled"]
    outs = {}
    for adain in ("qk", None):
        for use_graph in (True, False) if adain else (False,):
            den = AnimateDiffDenoiser(unet, Fr, 128, 128, num_inference_steps=10, device=cuda, use_graph=use_graph,
                                      context_length=context, cross_frame=CrossFrameAttention(("first",), adain=adain))
            assert den.cross_frame.adain == adain
            den.set_prompt_embeds(enc[1:2], pooled[1:2], enc[0:1], pooled[0:1])
            den.init_latents(seed=3)
            outs[adain, use_graph] = den.run_steps(3).clone()
            assert (den.graph is not None) == use_graph
    assert torch.isfinite(outs["qk", True]).all()
    assert torch.equal(outs["qk", True], outs["qk", False])
    assert not torch.equal(outs["qk", False], outs[None, False])


# ------------------------------------------------------------------ 6. refusals before any launch
def test_refused_before_any_launch(cuda, K, tiny):
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser
    from video_style_transfer_amd.unet_motion import CrossFrameAttention
    unet, enc, kw = tiny["unet"], tiny["enc"], tiny["kw"]
    lat4 = torch.zeros(2, 4, 4, 16, 16, device=cuda)
    thin = torch.zeros(2, 4, 4, 2, 1, device=cuda)      # the deepest level holds one token per frame
    t = torch.tensor([761.0, 761.0], device=cuda)
    VstError = K._lib.VstError
    x = torch.zeros(4 * 16, 64, dtype=BF16, device=cuda)
    den_kw = dict(num_inference_steps=10, device=cuda)
    K.profile_launches(True)
    try:
        for bad in (CrossFrameAttention(("first",), adain="kv"), CrossFrameAttention(("prev",), adain="qk"),
                    CrossFrameAttention((4,), adain="qkv")):
            with pytest.raises(VstError, match="cross_frame"):
                unet(lat4, t, enc.to(cuda), cross_frame=bad, **kw)
            with pytest.raises(VstError, match="cross_frame"):
                AnimateDiffDenoiser(unet, 4, 128, 128, cross_frame=bad, **den_kw)
        with pytest.raises(VstError, match="cross_frame"):
            unet(thin, t, enc.to(cuda), cross_frame=CrossFrameAttention(("first",), adain="qk"), **kw)
        with pytest.raises(VstError, match="cross_frame"):
            AnimateDiffDenoiser(unet, 4, 16, 8, cross_frame=CrossFrameAttention(("first",), adain="qk"), **den_kw)
        with pytest.raises(VstError, match="cross_frame"):
            AnimateDiffDenoiser(unet, 4, 128, 128, cross_frame=CrossFrameAttention(("first",), adain="qk"),
                                shard=types.SimpleNamespace(world=2, rank=0), **den_kw)
        # the wrapper's own refusals
        for args in ((1, 4, 16, 4), (1, 4, 16, -1), (1, 64, 1, 0), (1, 4, 8, 0)):
            with pytest.raises(VstError, match="^frame_adain: "):
                K.frame_adain(x, *args)
        with pytest.raises(VstError, match="^frame_adain: eps "):
            K.frame_adain(x, 1, 4, 16, 0, eps=-1.0)
        with pytest.raises(VstError, match="^frame_adain: x "):
            K.frame_adain(x.cpu(), 1, 4, 16, 0)
        assert K.collect_launches() == []
    finally:
        K.profile_launches(False)
    assert not x.any()
    AnimateDiffDenoiser(unet, 4, 128, 128, cross_frame=CrossFrameAttention((3, "prev"), adain="qkv"), **den_kw)  # accepted
