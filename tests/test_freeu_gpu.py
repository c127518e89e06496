"""FreeU in the up path on the GPU: the kernel against the closed form in fp64, its bit contracts
(identity, batch independence, in-place backbone, strided views), the UNet against the oracle with apply_freeu patched
into its resnets, and the denoiser (captured = eager, set_freeu / clear_freeu, composition with a sampler and a source
clip).

Kernel bound: |y - ref| <= 2^-8 |ref| + 1e-5 max|x| on every element: one bf16 rounding (2^-9 relative) doubled, plus
fp32 accumulation of the seven sums over <= 1024 terms (tests/test_freeu.py pins the closed form itself against
torch.fft).  The model-level bar is tests/test_cross_frame_gpu.py's: e <= 3e-2 and e <= 1.25 e0 + 2e-3, e0 the plain
forward's error against the unpatched oracle.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
SDXL = (0.9, 0.2, 1.3, 1.4)  # s1, s2, b1, b2


@pytest.fixture(scope="module")
def K():
    from video_style_transfer_amd import kernels
    return kernels


def table_of(cuda, s, b):
    """Both stages hold (s, b)."""
    return torch.tensor([[s, b], [s, b]], dtype=F32, device=cuda)


def make(nimg, H, W, Cs, Cx, seed=0):
    g = torch.Generator().manual_seed(seed + 7 * H + W + Cs)
    rows = nimg * H * W
    # maps with a mean, a gradient and noise: every one of the seven sums is far from zero
    skip = torch.randn(rows, Cs, generator=g) + 0.5 + torch.linspace(-1, 1, rows)[:, None]
    x = torch.randn(rows, Cx, generator=g) * 2
    return x.to(BF16), skip.to(BF16)


def filter_ref(skip, nimg, H, W, s):
    """fp64 closed form of the bf16 rows [nimg*H*W, Cs] -> fp64 rows."""
    from video_style_transfer_amd.freeu import fourier_filter_reference
    Cs = skip.shape[1]
    m = skip.double().view(nimg, H, W, Cs).permute(0, 3, 1, 2)
    return fourier_filter_reference(m, s).permute(0, 2, 3, 1).reshape(-1, Cs)


def backbone_ref(x, b):
    Cx = x.shape[1]
    out = x.clone()
    out[:, :Cx // 2] = (x[:, :Cx // 2].float() * torch.tensor(b, dtype=F32)).to(BF16)
    return out


def bits(t):
    return t.contiguous().view(torch.int16).cpu()


# ------------------------------------------------------------------ 1. kernel vs fp64
CASES = [(1, 2, 2, 64, 64), (3, 3, 5, 72, 80), (2, 4, 4, 256, 256), (2, 8, 8, 64, 128), (1, 16, 16, 1280, 1280),
         (2, 32, 32, 320, 640),
         (1, 36, 30, 8, 16)]   # more than 1024 rows: the slab is read twice instead of kept


@pytest.mark.parametrize("nimg,H,W,Cs,Cx", CASES)
@pytest.mark.parametrize("s,b", [(0.9, 1.3), (0.2, 1.4)])
def test_kernel_vs_fp64(cuda, K, nimg, H, W, Cs, Cx, s, b):
    x, skip = make(nimg, H, W, Cs, Cx)
    tab = table_of(cuda, s, b)
    s32, b32 = (float(v) for v in tab[0].cpu())
    for stage in (0, 1):
        xo, so = K.freeu(x.to(cuda), skip.to(cuda), nimg, H, W, tab, stage)
        ref = filter_ref(skip, nimg, H, W, s32)
        err = (so.double().cpu() - ref).abs()
        bound = 2.0 ** -8 * ref.abs() + 1e-5 * skip.float().abs().max().item()
        print(f"[freeu] {nimg, H, W, Cs, Cx} s={s}: max err {err.max():.3e}, max err/bound {(err / bound).max():.3f}")
        assert torch.isfinite(so.float()).all()
        assert (err <= bound).all(), (err / bound).max()
        assert torch.equal(bits(xo), bits(backbone_ref(x, b32)))


def test_identity(cuda, K):
    for nimg, H, W, Cs, Cx in CASES[1:4] + CASES[5:]:
        x, skip = make(nimg, H, W, Cs, Cx, seed=1)
        skip[0, 0] = -0.0
        xo, so = K.freeu(x.to(cuda), skip.to(cuda), nimg, H, W, table_of(cuda, 1.0, 1.0), 1)
        assert torch.equal(bits(xo), bits(x)) and torch.equal(bits(so), bits(skip))


@pytest.mark.parametrize("nimg,H,W,Cs,Cx", [(3, 3, 5, 72, 80), (3, 16, 16, 128, 64), (2, 32, 32, 320, 640)])
def test_image_bits_do_not_depend_on_the_batch(cuda, K, nimg, H, W, Cs, Cx):
    x, skip = make(nimg, H, W, Cs, Cx, seed=2)
    tab = table_of(cuda, 0.2, 1.4)
    xo, so = K.freeu(x.to(cuda), skip.to(cuda), nimg, H, W, tab, 0)
    r = slice(H * W, 2 * H * W)
    xo1, so1 = K.freeu(x[r].to(cuda), skip[r].to(cuda), 1, H, W, tab, 0)
    assert torch.equal(bits(so1), bits(so[r])) and torch.equal(bits(xo1), bits(xo[r]))


def test_stage_selects_the_table_row_on_the_device(cuda, K):
    """(s, b) are read from the table at launch: rewriting it in place changes the next launch."""
    nimg, H, W, Cs, Cx = 2, 8, 8, 64, 128
    x, skip = make(nimg, H, W, Cs, Cx, seed=3)
    xd, sd = x.to(cuda), skip.to(cuda)
    tab = torch.tensor([[0.9, 1.3], [0.2, 1.4]], dtype=F32, device=cuda)
    a0 = K.freeu(xd, sd, nimg, H, W, tab, 0)
    a1 = K.freeu(xd, sd, nimg, H, W, tab, 1)
    assert not torch.equal(a0[1], a1[1]) and not torch.equal(a0[0], a1[0])
    tab.copy_(torch.tensor([[0.2, 1.4], [0.9, 1.3]]))
    b0 = K.freeu(xd, sd, nimg, H, W, tab, 0)
    assert torch.equal(b0[0], a1[0]) and torch.equal(b0[1], a1[1])


def test_backbone_in_place(cuda, K):
    nimg, H, W, Cs, Cx = 2, 8, 8, 64, 128
    x, skip = make(nimg, H, W, Cs, Cx, seed=4)
    tab = table_of(cuda, 0.9, 1.3)
    xo, so = K.freeu(x.to(cuda), skip.to(cuda), nimg, H, W, tab, 0)
    xd = x.to(cuda)
    ret, so2 = K.freeu(xd, skip.to(cuda), nimg, H, W, tab, 0, x_out=xd)
    assert ret.data_ptr() == xd.data_ptr()
    assert torch.equal(xd, xo) and torch.equal(so2, so)


# ------------------------------------------------------------------ 2. view contract
def test_view_contract(cuda, K):
    """x and skip column views of NaN-padded arenas with NaN guard rows, the outputs strided views inside
    sentinel-filled arenas (tests/test_cross_frame_gpu.py::test_frames_view_contract's harness)."""
    nimg, H, W, Cs, Cx = 3, 3, 5, 72, 80
    T = nimg * H * W
    GT, GB, GC, SENT = 8, 40, 8, 0x7FA5
    x, skip = make(nimg, H, W, Cs, Cx, seed=5)
    tab = table_of(cuda, 0.2, 1.4)
    dense_x, dense_s = K.freeu(x.to(cuda), skip.to(cuda), nimg, H, W, tab, 0)

    def arena_in(t):
        a = torch.full((GT + T + GB, GC + t.shape[1] + GC), float("nan"), dtype=BF16, device=cuda)
        a[GT:GT + T, GC:GC + t.shape[1]] = t.to(cuda)
        return a, a[GT:GT + T, GC:GC + t.shape[1]]

    def arena_out(C):
        a = torch.empty((GT + T + GB, GC + C + 2 * GC), dtype=BF16, device=cuda)
        a.view(torch.int16).fill_(SENT)
        return a, a[GT:GT + T, GC:GC + C]

    ax, vx = arena_in(x)
    as_, vs = arena_in(skip)
    axo, vxo = arena_out(Cx)
    aso, vso = arena_out(Cs)
    rx, rs = K.freeu(vx, vs, nimg, H, W, tab, 0, x_out=vxo, skip_out=vso)
    assert rx.data_ptr() == vxo.data_ptr() and rs.data_ptr() == vso.data_ptr()
    for arena, C, dense in ((axo, Cx, dense_x), (aso, Cs, dense_s)):
        same = arena.view(torch.int16) == SENT
        outside = ~same
        outside[GT:GT + T, GC:GC + C] = False
        assert not outside.any(), "guard band written"
        inner = arena[GT:GT + T, GC:GC + C]
        assert not (same[GT:GT + T, GC:GC + C] | ~torch.isfinite(inner.float())).any(), "view unwritten or non-finite"
        assert torch.equal(bits(inner), bits(dense))
    for arena, view, src in ((ax, vx, x), (as_, vs, skip)):
        pad = torch.ones_like(arena, dtype=torch.bool)
        pad[GT:GT + T, GC:GC + src.shape[1]] = False
        assert torch.isnan(arena[pad]).all() and torch.equal(bits(view), bits(src)), "input arena written"

    VstError = K._lib.VstError
    args = (vx, vs, nimg, H, W, tab, 0)
    before = (axo.clone(), aso.clone())
    with pytest.raises(VstError):
        K.freeu(*args, x_out=vxo, skip_out=torch.empty((T, Cs), dtype=F32, device=cuda))             # dtype
    with pytest.raises(VstError):
        K.freeu(*args, x_out=vxo, skip_out=aso[GT:GT + T + 1, GC:GC + Cs])                           # shape
    with pytest.raises(VstError):
        K.freeu(*args, x_out=torch.empty((T, 2 * Cx), dtype=BF16, device=cuda)[:, ::2], skip_out=vso)  # stride
    with pytest.raises(VstError):
        K.freeu(*args, x_out=vxo, skip_out=torch.empty((T, Cs), dtype=BF16))                         # CPU
    with pytest.raises(VstError):
        K.freeu(vx, vs.float(), nimg, H, W, tab, 0, x_out=vxo, skip_out=vso)                         # input dtype
    with pytest.raises(VstError):
        K.freeu(vx, vs, nimg, H, W, tab.cpu(), 0, x_out=vxo, skip_out=vso)                           # CPU table
    with pytest.raises(VstError, match="status 1"):
        K.freeu(vx, vs, nimg, H, W, tab, 0, x_out=vxo, skip_out=vs)                                  # skip in place
    with pytest.raises(VstError, match="status 1"):
        K.freeu(vx, vs, nimg, H, W, tab, 2, x_out=vxo, skip_out=vso)                                 # stage
    with pytest.raises(VstError, match="status 1"):
        K.freeu(vx, as_[GT:GT + T, GC - 4:GC - 4 + Cs], nimg, H, W, tab, 0, x_out=vxo, skip_out=vso)   # alignment
    torch.cuda.synchronize()
    assert torch.equal(bits(axo), bits(before[0])) and torch.equal(bits(aso), bits(before[1]))


# ------------------------------------------------------------------ 3. UNet against the oracle
def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm()).item()


@pytest.fixture(scope="module")
def tiny(cuda):
    from test_parity_gpu import _setup
    from video_style_transfer_amd.utils import build_unet
    cfg, sd, lat, enc, pooled, tids = _setup("tiny", 4, 16)
    unet = build_unet(cfg, state_dict=sd, device=cuda)
    kw = dict(added_cond_kwargs={"text_embeds": pooled.to(cuda), "time_ids": tids.to(cuda)})
    return dict(cfg=cfg, sd=sd, lat=lat, enc=enc, pooled=pooled, tids=tids, unet=unet, kw=kw)


def test_freeu_unet_vs_oracle(cuda, K, tiny, monkeypatch):
    """Tiny UNet, B = 2, F = 4, 16x16 latent (stage 0 at 4x4, stage 1 at 8x8) against oracle.unet.unet_forward whose
    resnets of up_blocks.{0,1} first apply apply_freeu_reference to the (hidden, skip) halves of their concatenated
    input, split at the channel count of the last resnet output."""
    import oracle.unet as OU
    from video_style_transfer_amd.freeu import FreeU, apply_freeu_reference
    cfg, sd, lat, enc, pooled, tids, unet, kw = (tiny[k] for k in ("cfg", "sd", "lat", "enc", "pooled", "tids", "unet",
                                                                   "kw"))
    t = torch.tensor([761.0, 761.0])
    ref0 = OU.unet_forward(sd, cfg.to_dict(), lat, t, enc, pooled, tids)
    args = (lat.to(cuda), t.to(cuda), enc.to(cuda))
    K.profile_launches(True)
    try:
        out0 = unet(*args, **kw).sample
        kinds0 = [r[0] for r in K.collect_launches()]
    finally:
        K.profile_launches(False)
    assert "freeu" not in kinds0
    e0 = rel(out0, ref0)

    orig, patched, last = OU.resnet, [], [None]

    def resnet(P, name, x, temb, eps=1e-5):
        if name.startswith(("up_blocks.0.", "up_blocks.1.")):
            stage = int(name.split(".")[1])
            hidden, skip = apply_freeu_reference(stage, x[:, :last[0]], x[:, last[0]:], *SDXL)
            x = torch.cat([hidden, skip], 1)
            patched.append(name)
        y = orig(P, name, x, temb, eps)
        last[0] = y.shape[1]
        return y

    monkeypatch.setattr(OU, "resnet", resnet)
    ref = OU.unet_forward(sd, cfg.to_dict(), lat, t, enc, pooled, tids)
    monkeypatch.undo()
    assert len(patched) == 6

    K.profile_launches(True)
    try:
        out = unet(*args, freeu=SDXL, **kw).sample
        kinds = [r[0] for r in K.collect_launches()]
    finally:
        K.profile_launches(False)
    assert kinds.count("freeu") == 6
    e = rel(out, ref)
    print(f"[freeu] UNet tiny F=4: freeu rel_l2={e:.3e}, plain rel_l2={e0:.3e}, "
          f"freeu vs plain {rel(out, out0):.3e}")
    assert e <= 3e-2 and e <= 1.25 * e0 + 2e-3, (e, e0)
    assert rel(out, out0) > 1e-2 and rel(ref, ref0) > 1e-2
    # a FreeU object is the option; enable_freeu sets the default of forward(), disable_freeu removes it
    assert torch.equal(unet(*args, freeu=FreeU(*SDXL, device=cuda), **kw).sample, out)
    unet.enable_freeu(*SDXL)
    try:
        assert torch.equal(unet(*args, **kw).sample, out)
    finally:
        unet.disable_freeu()
    assert torch.equal(unet(*args, **kw).sample, out0)


# ------------------------------------------------------------------ 4. the denoiser
def denoiser(tiny, cuda, **kw):
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser
    enc, pooled = tiny["enc"], tiny["pooled"]
    den = AnimateDiffDenoiser(tiny["unet"], 4, 128, 128, num_inference_steps=10, device=cuda, **kw)
    den.set_prompt_embeds(enc[1:2], pooled[1:2], enc[0:1], pooled[0:1])
    den.init_latents(seed=3)
    return den


@pytest.fixture(scope="module")
def plain3(tiny, cuda):
    return denoiser(tiny, cuda, use_graph=False).run_steps(3).clone()


def test_denoiser_graph_equals_eager_and_identity(cuda, tiny, plain3):
    eager = denoiser(tiny, cuda, use_graph=False, freeu=SDXL).run_steps(3).clone()
    dg = denoiser(tiny, cuda, freeu=SDXL)
    graph = dg.run_steps(3).clone()
    assert dg.graph is not None and torch.isfinite(graph).all()
    assert torch.equal(graph, eager)
    assert not torch.equal(eager, plain3)
    ones = denoiser(tiny, cuda, use_graph=False, freeu=(1, 1, 1, 1)).run_steps(3)
    assert torch.equal(ones, plain3)


def test_denoiser_set_and_clear_freeu(cuda, tiny, plain3):
    new = (0.6, 0.4, 1.1, 1.2)
    fresh = denoiser(tiny, cuda, use_graph=False, freeu=new).run_steps(3).clone()
    den = denoiser(tiny, cuda, freeu=SDXL)
    den.run_steps(3)
    g = den.graph
    assert g is not None
    den.set_freeu(*new)
    assert den.graph is g
    den.init_latents(seed=3)
    assert torch.equal(den.run_steps(3), fresh)
    assert den.graph is g
    den.clear_freeu()
    assert den.graph is None
    den.init_latents(seed=3)
    assert torch.equal(den.run_steps(3), plain3)
    den.set_freeu(*new)   # turning it on again drops the plain captured step
    assert den.graph is None
    den.init_latents(seed=3)
    assert torch.equal(den.run_steps(3), fresh)


def test_denoiser_composes_with_sampler_and_source(cuda, tiny):
    from video_style_transfer_amd.scheduler import EulerDiscreteScheduler
    outs = {}
    for fu in (SDXL, None):
        for use_graph in (True, False) if fu else (False,):
            den = denoiser(tiny, cuda, use_graph=use_graph, freeu=fu, sampler="dpmpp_2m",
                           scheduler=EulerDiscreteScheduler(sigma_schedule="karras"))
            outs[fu, use_graph] = den.run_steps(3).clone()
    assert torch.isfinite(outs[SDXL, True]).all()
    assert torch.equal(outs[SDXL, True], outs[SDXL, False])
    assert not torch.equal(outs[SDXL, False], outs[None, False])

    g = torch.Generator().manual_seed(9)
    z0 = torch.randn(1, 4, 4, 16, 16, generator=g)
    mask = (torch.rand(1, 4, 16, 16, generator=g) > 0.5).float()
    outs = {}
    for fu in (SDXL, None):
        for use_graph in (True, False) if fu else (False,):
            den = denoiser(tiny, cuda, use_graph=use_graph, freeu=fu)
            den.set_source(z0, 0.5, mask=mask, seed=5)
            outs[fu, use_graph] = den.run_steps(3).clone()
    assert torch.isfinite(outs[SDXL, True]).all()
    assert torch.equal(outs[SDXL, True], outs[SDXL, False])
    assert not torch.equal(outs[SDXL, False], outs[None, False])
