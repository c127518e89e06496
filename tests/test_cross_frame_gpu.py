"""Cross-frame spatial self-attention (DESIGN.md "Cross-frame spatial self-attention"): the kernel against fp32 and
against the plain self-attention kernel's bits, its view contract, and the option through the processor, the UNet and
the denoiser.

The fp32 reference is tests/test_cross_frame.py's frames_ref (checked there against plain SDPA).  Kernel bars are
test_kernels_gpu.test_spatial_attention's (its `check` defaults).  The model-level bar compares the error with the
option against the error the plain path (existing code) makes against the unpatched oracle on the same inputs:
e <= 1.25 e0 + 2e-3, the form tests/test_temporal_context_gpu.py uses.
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
    print(f"[cross-frame] {name}: rel_l2={l2:.3e} rel_max={mx:.3e}")
    assert l2 <= rel_l2 and mx <= rel_max, f"{name}: rel_l2={l2:.3e} rel_max={mx:.3e}"


def cols(qkv, C):
    return qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]


# ------------------------------------------------------------------ 1. kernel vs fp32
CASES = [(2, 3, 2, 256, ("first",)),          # base case
         (1, 4, 1, 80, ("first", "prev")),    # per-source tail tile
         (2, 2, 1, 16, (1,)),                 # below one tile, anchor = last frame
         (1, 3, 3, 1024, ("prev",)),          # many tiles
         (3, 2, 1, 130, ("first",)),          # odd N
         (1, 1, 2, 256, ("first", "prev"))]   # everything de-duplicates


@pytest.mark.parametrize("nclip,Fr,heads,N,sources", CASES)
@pytest.mark.parametrize("qs", [1.0, 3.0])
def test_frames_vs_fp32(cuda, K, nclip, Fr, heads, N, sources, qs):
    """qs scales q: logit std 1 (near-uniform softmax) and 3 (peaked: max tracking / tile rescale matter)."""
    from test_cross_frame import frames_ref
    g = torch.Generator().manual_seed(N + heads + Fr)
    C = heads * 64
    qkv = rnd(nclip * Fr * N, 3 * C, gen=g)
    qkv[:, :C] = (qkv[:, :C].float() * qs).to(BF16)
    out = K.spatial_attention_frames(*cols(qkv.to(cuda), C), nclip, Fr, heads, N, sources)
    check(out, frames_ref(*cols(qkv, C), nclip, Fr, N, heads, sources), name=f"frames {nclip, Fr, heads, N, sources}")


@pytest.mark.parametrize("which", ["anchor", "own"])
def test_frames_peaked(cuda, K, which):
    """K rows of the anchor frame x4: the running max jumps when the walk enters the second source; K rows of the
    other frames x4: it is set in the own frame and the anchor's tiles only rescale by alpha = 1."""
    from test_cross_frame import frames_ref
    nclip, Fr, heads, N, sources = 1, 3, 1, 256, ("first",)
    g = torch.Generator().manual_seed(11)
    qkv = rnd(nclip * Fr * N, 192, gen=g)
    rows = slice(0, N) if which == "anchor" else slice(N, Fr * N)
    qkv[rows, 64:128] = (qkv[rows, 64:128].float() * 4).to(BF16)
    out = K.spatial_attention_frames(*cols(qkv.to(cuda), 64), nclip, Fr, heads, N, sources)
    check(out, frames_ref(*cols(qkv, 64), nclip, Fr, N, heads, sources), name=f"peaked {which}")


# ------------------------------------------------------------------ 2. bit anchors (N = 256: the plain entry's same loop)
def _gather(t, nclip, Fr, N, lists):
    """[sum over (clip, listed frame f) of len(list) * N, C]: the K or V rows of every listed frame's key list,
    physically concatenated."""
    t4 = t.view(nclip, Fr, N, -1)
    return torch.cat([t4[b, j] for b in range(nclip) for f, fl in lists for j in fl], 0).contiguous()


@pytest.mark.parametrize("qs", [1.0, 3.0])
def test_frames_bits_equal_plain_kernel(cuda, K, qs):
    nclip, Fr, heads, N = 2, 4, 2, 256
    C = heads * 64
    g = torch.Generator().manual_seed(5)
    qkv = rnd(nclip * Fr * N, 3 * C, gen=g)
    qkv[:, :C] = (qkv[:, :C].float() * qs).to(BF16)
    qkv = qkv.to(cuda)
    q, k, v = cols(qkv, C)
    plain = K.spatial_attention(q, k, v, nclip * Fr, heads, N, N)

    # no sources: the plain launch's bits on the whole output
    assert torch.equal(K.spatial_attention_frames(q, k, v, nclip, Fr, heads, N, ()), plain)
    # F = 1: every source de-duplicates
    assert torch.equal(K.spatial_attention_frames(q, k, v, nclip * Fr, 1, heads, N, ("first", "prev")), plain)

    for sources, nk in ((("first",), 2), (("first", "prev"), 3)):
        out = K.spatial_attention_frames(q, k, v, nclip, Fr, heads, N, sources).view(nclip, Fr, N, C)
        # frame 0 attends to itself only
        assert torch.equal(out[:, 0], plain.view(nclip, Fr, N, C)[:, 0])
        # frames with a full list: the plain kernel on K/V physically concatenated in torch
        lists = [(f, K.frame_list(f, Fr, sources)) for f in range(Fr)]
        lists = [(f, fl) for f, fl in lists if len(fl) == nk]
        assert [f for f, _ in lists] == list(range(nk - 1, Fr))
        fs = [f for f, _ in lists]
        qs_ = q.reshape(nclip, Fr, N, C)[:, fs].reshape(-1, C).contiguous()
        kc, vc = _gather(k, nclip, Fr, N, lists), _gather(v, nclip, Fr, N, lists)
        cat = K.spatial_attention(qs_, kc, vc, nclip * len(fs), heads, N, nk * N)
        assert torch.equal(out[:, fs].reshape(-1, C), cat), sources


# ------------------------------------------------------------------ 3. view contract
def test_frames_view_contract(cuda, K):
    """q/k/v column views of one NaN-padded [rows, 3C + pad] arena with NaN guard rows, out a strided view inside a
    sentinel arena (tests/test_view_contract_gpu.py's harness, copied in small)."""
    from test_cross_frame import frames_ref
    nclip, Fr, heads, N, sources = 2, 3, 2, 80, ("first", "prev")
    C, T = heads * 64, nclip * Fr * N
    GT, GB, GC, SENT = 8, 72, 8, 0x7FA5
    qkv = rnd(T, 3 * C, gen=torch.Generator().manual_seed(7))
    dense = qkv.to(cuda)
    dense_out = K.spatial_attention_frames(*cols(dense, C), nclip, Fr, heads, N, sources)

    ld_in = GC + 3 * C + GC
    a_in = torch.full((GT + T + GB, ld_in), float("nan"), dtype=BF16, device=cuda)
    a_in[GT:GT + T, GC:GC + 3 * C] = dense
    v_in = a_in[GT:GT + T, GC:GC + 3 * C]
    ld_out = GC + C + GC
    a_out = torch.empty((GT + T + GB, ld_out), dtype=BF16, device=cuda)
    a_out.view(torch.int16).fill_(SENT)
    v_out = a_out[GT:GT + T, GC:GC + C]

    ret = K.spatial_attention_frames(*cols(v_in, C), nclip, Fr, heads, N, sources, out=v_out)
    assert ret.data_ptr() == v_out.data_ptr()
    same = a_out.view(torch.int16) == SENT
    outside = ~same
    outside[GT:GT + T, GC:GC + C] = False
    assert not outside.any(), "guard band written"
    inner = a_out[GT:GT + T, GC:GC + C]
    assert not (same[GT:GT + T, GC:GC + C] | ~torch.isfinite(inner.float())).any(), "view unwritten or non-finite"
    assert torch.equal(inner.contiguous().view(torch.int16), dense_out.view(torch.int16))
    pad = torch.ones_like(a_in, dtype=torch.bool)
    pad[GT:GT + T, GC:GC + 3 * C] = False
    assert torch.isnan(a_in[pad]).all() and torch.equal(v_in, dense), "input arena written"
    check(inner, frames_ref(*cols(qkv, C), nclip, Fr, N, heads, sources), name="frames view")

    VstError = K._lib.VstError
    args = (*cols(v_in, C), nclip, Fr, heads, N, sources)
    before = a_out.clone()
    with pytest.raises(VstError):
        K.spatial_attention_frames(*args, out=torch.empty((T, C), dtype=F32, device=cuda))             # dtype
    with pytest.raises(VstError):
        K.spatial_attention_frames(*args, out=a_out[GT:GT + T + 1, GC:GC + C])                         # shape
    with pytest.raises(VstError):
        K.spatial_attention_frames(*args, out=torch.empty((T, 2 * C), dtype=BF16, device=cuda)[:, ::2])  # stride
    with pytest.raises(VstError):
        K.spatial_attention_frames(*args, out=torch.empty((T, C), dtype=BF16))                          # CPU
    torch.cuda.synchronize()
    assert torch.equal(a_out.view(torch.int16), before.view(torch.int16))


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


def test_cross_frame_unet_vs_oracle(cuda, K, tiny, monkeypatch):
    """Tiny UNet, B = 2, F = 4, 16x16 latent, cross_frame ("first",) against oracle.unet.unet_forward whose spatial
    self-attention is replaced (here, by monkeypatch) by the extended fp32 reference; e0: the plain forward's error
    against the unpatched oracle on the same inputs."""
    import oracle.unet as OU
    from test_cross_frame import frames_ref
    from video_style_transfer_amd.unet_motion import CrossFrameAttention
    cfg, sd, lat, enc, pooled, tids, unet, kw = (tiny[k] for k in ("cfg", "sd", "lat", "enc", "pooled", "tids", "unet",
                                                                   "kw"))
    Fr, sources = 4, ("first",)
    t = torch.tensor([761.0, 761.0])
    lat4 = lat[:, :, :Fr].contiguous()
    ref0 = OU.unet_forward(sd, cfg.to_dict(), lat4, t, enc, pooled, tids)
    out0 = unet(lat4.to(cuda), t.to(cuda), enc.to(cuda), **kw).sample
    e0 = rel(out0, ref0)

    orig, patched = OU.attention, []

    def extended(P, name, x, enc_, heads, lora):
        if enc_ is not None or "motion_modules" in name:
            return orig(P, name, x, enc_, heads, lora)
        patched.append(name)

        def pr(n, t_):
            return OU.proj(P, f"{name}.{'to_out.0' if n == 'to_out' else n}", t_, lora)
        BF, N, _ = x.shape
        q, k, v = (pr(n, x).reshape(BF * N, -1) for n in ("to_q", "to_k", "to_v"))
        assert q.shape[1] == heads * 64
        return pr("to_out", frames_ref(q, k, v, BF // Fr, Fr, N, heads, sources).view(BF, N, -1))

    monkeypatch.setattr(OU, "attention", extended)
    ref = OU.unet_forward(sd, cfg.to_dict(), lat4, t, enc, pooled, tids)
    monkeypatch.undo()
    assert patched and all(n.endswith(".attn1") for n in patched)

    K.profile_launches(True)
    try:
        out = unet(lat4.to(cuda), t.to(cuda), enc.to(cuda), cross_frame=CrossFrameAttention(sources), **kw).sample
        kinds = [r[0] for r in K.collect_launches()]
    finally:
        K.profile_launches(False)
    assert kinds.count("spatial_attention_frames") == len(patched), (kinds.count("spatial_attention_frames"), patched)
    e = rel(out, ref)
    print(f"[cross-frame] UNet tiny F=4: cross_frame rel_l2={e:.3e}, plain rel_l2={e0:.3e}")
    assert e <= 3e-2 and e <= 1.25 * e0 + 2e-3, (e, e0)
    # the option does something, on frames > 0 (frame 0's spatial attention is its own, but the motion modules mix
    # the frames afterwards, so frame 0 moves too; frames > 0 must)
    assert rel(out[:, :, 1:], out0[:, :, 1:]) > 1e-2
    assert rel(ref[:, :, 1:], ref0[:, :, 1:]) > 1e-2
    # the sources of a plain tuple are the option
    assert torch.equal(unet(lat4.to(cuda), t.to(cuda), enc.to(cuda), cross_frame=sources, **kw).sample, out)
    # off, and on a single-frame clip: today's forward, bit for bit
    assert torch.equal(unet(lat4.to(cuda), t.to(cuda), enc.to(cuda), cross_frame=None, **kw).sample, out0)
    lat1 = lat[:, :, :1].contiguous()
    one = unet(lat1.to(cuda), t.to(cuda), enc.to(cuda), **kw).sample
    K.profile_launches(True)
    try:
        one_cf = unet(lat1.to(cuda), t.to(cuda), enc.to(cuda), cross_frame=CrossFrameAttention(("first", "prev")),
                      **kw).sample
        kinds = [r[0] for r in K.collect_launches()]
    finally:
        K.profile_launches(False)
    assert "spatial_attention_frames" not in kinds and torch.equal(one_cf, one)


# ------------------------------------------------------------------ 5. the denoiser
@pytest.mark.parametrize("Fr,context", [(4, None), (20, 16)])
def test_cross_frame_denoiser_graph_equals_eager(cuda, tiny, Fr, context):
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser
    unet, enc, pooled = tiny["unet"], tiny["enc"], tiny["pooled"]
    outs = {}
    for cf in (("first", "prev"), None):
        for use_graph in (True, False) if cf else (False,):
            den = AnimateDiffDenoiser(unet, Fr, 128, 128, num_inference_steps=10, device=cuda, use_graph=use_graph,
                                      context_length=context, cross_frame=cf)
            den.set_prompt_embeds(enc[1:2], pooled[1:2], enc[0:1], pooled[0:1])
            den.init_latents(seed=3)
            outs[cf, use_graph] = den.run_steps(2).clone()
            assert (den.graph is not None) == use_graph
    on = ("first", "prev")
    assert torch.isfinite(outs[on, True]).all()
    assert torch.equal(outs[on, True], outs[on, False])
    assert not torch.equal(outs[on, False], outs[None, False])


# ------------------------------------------------------------------ 6. refusals before any launch
def test_cross_frame_refused_before_any_launch(cuda, K, tiny):
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser
    from video_style_transfer_amd.unet_motion import CrossFrameAttention
    unet, enc, kw = tiny["unet"], tiny["enc"], tiny["kw"]
    lat4 = torch.zeros(2, 4, 4, 16, 16, device=cuda)
    t = torch.tensor([761.0, 761.0], device=cuda)
    two_ranks = types.SimpleNamespace(world=2, rank=0)   # refused before the shard is touched
    VstError = K._lib.VstError
    C, N, Fr = 64, 16, 4
    qkv = rnd(Fr * N, 3 * C).to(cuda)
    q, k, v = cols(qkv, C)
    K.profile_launches(True)
    try:
        with pytest.raises(VstError, match="cross_frame"):
            unet(lat4, t, enc.to(cuda), cross_frame=CrossFrameAttention((4,)), **kw)
        with pytest.raises(VstError, match="cross_frame"):
            AnimateDiffDenoiser(unet, 4, 128, 128, num_inference_steps=10, device=cuda, cross_frame=("first", 4))
        with pytest.raises(VstError, match="cross_frame"):
            unet(lat4[:, :, :2], t, enc.to(cuda), cross_frame=("first",), frame_shard=two_ranks, **kw)
        with pytest.raises(VstError, match="cross_frame"):
            AnimateDiffDenoiser(unet, 4, 128, 128, num_inference_steps=10, device=cuda, cross_frame=("first",),
                                shard=two_ranks)
        # status-1 arguments through the wrapper: the library refuses, nothing is launched
        for bad in ((4,), ("first", 0), ("prev", "prev"), (1, 7)):
            with pytest.raises(VstError, match="status 1"):
                K.spatial_attention_frames(q, k, v, 1, Fr, 1, N, bad)
        q68 = torch.zeros(Fr * N, 68, dtype=BF16, device=cuda)[:, :64]   # row stride no multiple of 8
        with pytest.raises(VstError, match="status 1"):
            K.spatial_attention_frames(q68, k, v, 1, Fr, 1, N, ("first",))
        # the wrapper's own checks
        with pytest.raises(VstError):
            K.spatial_attention_frames(q, k, v, 1, Fr + 1, 1, N, ("first",))          # rows != nclip*F*N
        with pytest.raises(VstError):
            K.spatial_attention_frames(q, k, v.contiguous(), 1, Fr, 1, N, ("first",))  # k/v row strides differ
        with pytest.raises(VstError):
            K.spatial_attention_frames(q.cpu(), k, v, 1, Fr, 1, N, ("first",))
        with pytest.raises(VstError):
            K.spatial_attention_frames(q, k, v, 1, Fr, 1, N, ("first", "prev", 2))     # three sources
        assert K.collect_launches() == []
    finally:
        K.profile_launches(False)
    AnimateDiffDenoiser(unet, 4, 128, 128, num_inference_steps=10, device=cuda, cross_frame=("first", 3))  # accepted
