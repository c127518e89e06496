"""FreeInit's frequency mix on the GPU: vst_free_init_mix against the torch.fft pipeline in fp64, its bit
contracts (Philox path = explicit noise, replayed graph, the two exact anchors, in place, determinism, batch
independence, views and workspace), the host refusals, and the denoiser (num_iters 1 = off, num_iters 2 = the manual
composition, no recapture, composition with a sampler and with FreeU).

Parity bar: max |kernel - fp64 pipeline| <= 4 x max |fp32 pipeline - fp64 pipeline|, both pipelines torch.fft on the
CPU on the same inputs (fftn, fftshift, mask, ifftshift, ifftn, real part: diffusers' _apply_free_init).  The 4 allows
for dense sums against butterflies; the yardstick is torch, never the kernel.  The all-ones anchor is held to the same
bar; its init=None case passes the re-noised latents x + init as x (what a caller of that form holds), so it runs at
the loop's scale: on x ~ N(0, 1) alone the fp32 pipeline multiplies r by an exact 0 and errs by 5e-7, below half an ulp
of the r ~ 14.6 that out = r + L(x - r), the form the zero anchor pins bit for bit, adds and subtracts.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
SHAPES = [(2, 4, 3, 5, 7), (1, 5, 5, 6, 10), (2, 4, 4, 8, 8), (1, 4, 16, 32, 32), (1, 4, 2, 1, 66)]
METHODS = ("butterworth", "gaussian", "ideal")
SCALE = float(torch.tensor(14.6, dtype=F32))   # init_noise_sigma of the SDXL schedule, as the fp32 the kernel is given
DIMS = (-3, -2, -1)


@pytest.fixture(scope="module")
def K():
    from video_style_transfer_amd import kernels
    return kernels


def make(shape, seed=0):
    """Inputs at the loop's scale: x ~ N(0, 1), init ~ N(0, 14.6^2), noise ~ N(0, 1) (r = SCALE * noise)."""
    g = torch.Generator().manual_seed(seed + sum(shape))
    x = torch.randn(shape, generator=g)
    init = SCALE * torch.randn(shape, generator=g)
    noise = torch.randn(shape, generator=g)
    return x, init, noise


def masks(shape, method="butterworth", **kw):
    """(M fp64 in fftshift order, M~ fp32 in DFT order) for a latent shape."""
    from video_style_transfer_amd.free_init import FreeInit, dft_order, freq_filter
    M = freq_filter(*shape[2:], FreeInit(method=method, **kw))
    return M, dft_order(M).to(F32)


def pipeline(x, init, noise, M, dtype):
    """diffusers' _apply_free_init on CPU in `dtype`: z_T = x + init, r = SCALE * noise, the mix in the shifted
    spectrum, the real part.  Returns fp64."""
    ctype = torch.complex128 if dtype == F64 else torch.complex64
    z_T = x.to(dtype) if init is None else x.to(dtype) + init.to(dtype)
    r = torch.tensor(SCALE, dtype=dtype) * noise.to(dtype)
    M = M.to(dtype)
    zf = torch.fft.fftshift(torch.fft.fftn(z_T.to(ctype), dim=DIMS), dim=DIMS)
    rf = torch.fft.fftshift(torch.fft.fftn(r.to(ctype), dim=DIMS), dim=DIMS)
    mixed = zf * M + rf * (1 - M)
    return torch.fft.ifftn(torch.fft.ifftshift(mixed, dim=DIMS), dim=DIMS).real.to(F64)


_BAR = {}


def inputs(shape, init=True):
    """make(shape); init=False: the init=None form of the same call, x holding the re-noised latents x + init (what
    the caller of that form passes: z = x alone), so both forms are tested at the loop's scale."""
    x, i, n = make(shape)
    return (x, i, n) if init else (x + i, None, n)


def bar(shape, M, key, init=True):
    """(fp64 pipeline result, the fp32 pipeline's max error) on inputs(shape, init), computed once per case."""
    if (shape, key, init) not in _BAR:
        x, i, n = inputs(shape, init)
        ref = pipeline(x, i, n, M, F64)
        e32 = (pipeline(x, i, n, M, F32) - ref).abs().max().item()
        _BAR[shape, key, init] = (ref, e32)
    return _BAR[shape, key, init]


def dev(cuda, *ts):
    return [None if t is None else t.to(cuda) for t in ts]


def counters(cuda, seed=1234, it=0):
    return torch.tensor([seed], dtype=I64, device=cuda), torch.tensor([it], dtype=I32, device=cuda)


# ------------------------------------------------------------------ 1. parity against torch.fft
@pytest.mark.parametrize("shape", SHAPES)
def test_parity_explicit_noise(cuda, K, shape):
    x, init, noise = make(shape)
    xd, idev, nd = dev(cuda, x, init, noise)
    for method in METHODS:
        M, Mt = masks(shape, method)
        ref, e32 = bar(shape, M, method)
        out = K.free_init_mix(xd, idev, Mt.to(cuda), SCALE, noise=nd)
        err = (out.double().cpu() - ref).abs().max().item()
        print(f"[free_init] {shape} {method}: kernel max err {err:.3e}, fp32 torch.fft max err {e32:.3e} "
              f"(ratio {err / max(e32, 1e-30):.2f})")
        assert torch.isfinite(out).all()
        assert err <= 4 * e32, (shape, method, err, e32)


# ------------------------------------------------------------------ 2. the Philox path
@pytest.mark.parametrize("shape", SHAPES)
def test_philox_path_equals_explicit_noise(cuda, K, shape):
    x, init, _ = make(shape, seed=1)
    xd, idev = dev(cuda, x, init)
    _, Mt = masks(shape)
    Mt = Mt.to(cuda)
    for seed_v, it_v in ((1234, 0), (2 ** 40 + 7, 3)):
        seed, it = counters(cuda, seed_v, it_v)
        n = K.noise_normal(seed, it, shape, stream_id=1)
        a = K.free_init_mix(xd, idev, Mt, SCALE, noise=n)
        b = K.free_init_mix(xd, idev, Mt, SCALE, seed=seed, it=it, stream_id=1)
        assert torch.equal(a, b)
        zero = K.free_init_mix(xd, idev, torch.zeros_like(Mt), SCALE, seed=seed, it=it)   # r itself, bit for bit
        assert torch.equal(zero, torch.tensor(SCALE, dtype=F32, device=cuda) * n)
    other = K.free_init_mix(xd, idev, Mt, SCALE, seed=seed, it=it, stream_id=2)
    assert not torch.equal(other, b)


def test_philox_counters_are_read_on_the_device_under_a_replayed_graph(cuda, K):
    shape = (2, 4, 4, 8, 8)
    x, init, _ = make(shape, seed=2)
    xd, idev = dev(cuda, x, init)
    Mt = masks(shape)[1].to(cuda)
    seed, it = counters(cuda, 11, 0)
    ws = K.free_init_workspace(shape, cuda)
    out = torch.empty_like(xd)
    kw = dict(seed=seed, it=it, workspace=ws)
    eager = {}
    for s, i in ((11, 0), (11, 1), (12, 1)):
        seed.fill_(s), it.fill_(i)
        eager[s, i] = K.free_init_mix(xd, idev, Mt, SCALE, **kw).clone()
    assert not torch.equal(eager[11, 0], eager[11, 1]) and not torch.equal(eager[11, 1], eager[12, 1])
    seed.fill_(11), it.fill_(0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        K.free_init_mix(xd, idev, Mt, SCALE, out=out, **kw)
    for s, i in ((11, 0), (11, 1), (12, 1), (11, 0)):
        seed.fill_(s), it.fill_(i)
        out.zero_()
        g.replay()
        assert torch.equal(out, eager[s, i]), (s, i)


# ------------------------------------------------------------------ 3. exact anchors and bit contracts
@pytest.mark.parametrize("shape", SHAPES)
def test_anchors_zero_and_one(cuda, K, shape):
    x, init, noise = make(shape, seed=3)
    xd, idev, nd = dev(cuda, x, init, noise)
    F, H, W = shape[2:]
    zeros = torch.zeros(F, H, W, dtype=F32, device=cuda)
    r = torch.tensor(SCALE, dtype=F32, device=cuda) * nd
    assert torch.equal(K.free_init_mix(xd, idev, zeros, SCALE, noise=nd), r)
    assert torch.equal(K.free_init_mix(xd, None, zeros, SCALE, noise=nd), r)
    ones64 = torch.ones(F, H, W, dtype=F64)
    for with_init in (True, False):
        x0, i0, n0 = inputs(shape, with_init)
        ref, e32 = bar(shape, ones64, "ones", with_init)
        want = x0.double() + i0.double() if with_init else x0.double()
        assert (ref - want).abs().max().item() <= 1e-12
        out = K.free_init_mix(*dev(cuda, x0, i0), zeros + 1, SCALE, noise=n0.to(cuda))
        err = (out.double().cpu() - want).abs().max().item()
        print(f"[free_init] {shape} ones init={with_init}: kernel max err {err:.3e}, fp32 torch.fft max err {e32:.3e} "
              f"(ratio {err / max(e32, 1e-30):.2f})")
        assert err <= 4 * e32, (shape, with_init, err, e32)


@pytest.mark.parametrize("shape", SHAPES)
def test_in_place_determinism_and_batch_independence(cuda, K, shape):
    x, init, noise = make(shape, seed=4)
    xd, idev, nd = dev(cuda, x, init, noise)
    Mt = masks(shape, "gaussian")[1].to(cuda)
    seed, it = counters(cuda, 5, 1)
    for kw in (dict(noise=nd), dict(seed=seed, it=it)):
        a = K.free_init_mix(xd, idev, Mt, SCALE, **kw)
        assert torch.equal(K.free_init_mix(xd, idev, Mt, SCALE, **kw), a)           # the same bits twice
        xi = xd.clone()
        ret = K.free_init_mix(xi, idev, Mt, SCALE, out=xi, **kw)                       # out is x
        assert ret.data_ptr() == xi.data_ptr() and torch.equal(xi, a)
        if shape[0] > 1:                                                              # clip 0 alone
            one = dict(noise=nd[:1]) if "noise" in kw else kw
            assert torch.equal(K.free_init_mix(xd[:1], idev[:1], Mt, SCALE, **one), a[:1])
    assert torch.equal(xd.cpu(), x) and torch.equal(idev.cpu(), init) and torch.equal(nd.cpu(), noise)


# ------------------------------------------------------------------ 4. views, workspace, refusals
def test_view_contract(cuda, K):
    """out and the workspace inside sentinel / NaN arenas: nothing outside the views is written, what lies past
    ws_bytes never reaches the result, the inputs are left alone (tests/test_freeu_gpu.py::test_view_contract's
    harness on flat fp32 blocks)."""
    shape = (2, 4, 3, 5, 7)
    n = 2 * 4 * 3 * 5 * 7
    G, SENT = 64, 0x7FA5A5A5
    x, init, noise = make(shape, seed=5)
    Mt = masks(shape)[1].to(cuda)
    dense = K.free_init_mix(*dev(cuda, x, init), Mt, SCALE, noise=noise.to(cuda))

    def arena_in(t):
        a = torch.full((G + t.numel() + G,), float("nan"), dtype=F32, device=cuda)
        a[G:G + t.numel()] = t.reshape(-1).to(cuda)
        return a, a[G:G + t.numel()].view(t.shape)

    ax, vx = arena_in(x)
    ai, vi = arena_in(init)
    an, vn = arena_in(noise)
    af, vf = arena_in(Mt)
    ao = torch.empty(G + n + G, dtype=F32, device=cuda)
    ao.view(I32).fill_(SENT)
    vo = ao[G:G + n].view(shape)
    need = K.free_init_workspace_bytes(shape) // 4
    assert need == 2 * 4 * 3 * 5 * 4 * 2
    aw = torch.full((G + need + G,), float("nan"), dtype=F32, device=cuda)   # NaN before and past the workspace
    vw = aw[G:G + need]
    ret = K.free_init_mix(vx, vi, vf, SCALE, noise=vn, out=vo, workspace=vw)
    assert ret.data_ptr() == vo.data_ptr()
    assert torch.equal(vo, dense) and torch.isfinite(vo).all()
    guard = torch.ones(G + n + G, dtype=torch.bool, device=cuda)
    guard[G:G + n] = False
    assert (ao.view(I32)[guard] == SENT).all(), "guard band of out written"
    assert torch.isnan(aw[:G]).all() and torch.isnan(aw[G + need:]).all(), "guard band of the workspace written"
    assert torch.isfinite(vw).all(), "the spectrum does not fill the workspace"
    for arena, view, src in ((ax, vx, x), (ai, vi, init), (an, vn, noise), (af, vf, Mt.cpu())):
        assert torch.isnan(arena[:G]).all() and torch.isnan(arena[G + src.numel():]).all()
        assert torch.equal(view.cpu(), src), "input written"
    # the Philox path through the same views
    seed, it = counters(cuda, 9, 2)
    dense_p = K.free_init_mix(*dev(cuda, x, init), Mt, SCALE, seed=seed, it=it)
    assert torch.equal(K.free_init_mix(vx, vi, vf, SCALE, seed=seed, it=it, out=vo, workspace=vw), dense_p)
    assert (ao.view(I32)[guard] == SENT).all() and torch.isnan(aw[:G]).all() and torch.isnan(aw[G + need:]).all()


def test_refusals_launch_nothing(cuda, K):
    VstError = K._lib.VstError
    shape = (2, 4, 3, 5, 7)
    x, init, noise = make(shape, seed=6)
    xd, idev, nd = dev(cuda, x, init, noise)
    Mt = masks(shape)[1].to(cuda)
    seed, it = counters(cuda)
    out = torch.full(shape, 7.0, dtype=F32, device=cuda)
    ws = K.free_init_workspace(shape, cuda)
    ws.fill_(3.0)
    big = torch.zeros(4 * xd.numel(), dtype=F32, device=cuda)
    n = xd.numel()
    wrapper = [
        dict(x=xd.double()), dict(x=xd.cpu()), dict(x=xd[:, :, :, :, ::2]), dict(x=xd[0]),           # x itself
        dict(init=idev[:1]), dict(init=idev.half()), dict(filt=Mt[:2]), dict(filt=Mt.double()),
        dict(filt=Mt.cpu()), dict(noise=nd[:, :2]), dict(noise=nd.cpu()),
        dict(noise=None), dict(noise=nd, seed=seed, it=it), dict(noise=None, seed=seed), dict(noise=None, it=it),
        dict(noise=None, seed=seed.int(), it=it), dict(noise=None, seed=seed, it=it.long()),
        dict(noise=None, seed=seed, it=it, stream_id=1 << 16), dict(noise=None, seed=seed, it=it, stream_id=-1),
        dict(out=out[:1]), dict(out=out.double()), dict(workspace=ws[:-1]), dict(workspace=ws.double()),
    ]
    for kw in wrapper:
        args = dict(x=xd, init=idev, filt=Mt, noise=nd, out=out, workspace=ws)
        args.update(kw)
        xa, ia, fa = args.pop("x"), args.pop("init"), args.pop("filt")
        with pytest.raises(VstError, match="^free_init_mix: "):
            K.free_init_mix(xa, ia, fa, SCALE, **args)
    library = [
        dict(out=idev),                                                    # out over init
        dict(out=nd),                                                      # out over the noise
        dict(x=big[:n].view(shape), out=big[4:n + 4].view(shape)),         # out over x, but not x itself
        dict(workspace=big[:ws.numel()], x=big[ws.numel() - 4:ws.numel() - 4 + n].view(shape)),   # workspace over x
        dict(workspace=torch.zeros(ws.numel() + 1, dtype=F32, device=cuda)[1:]),                  # 4-byte aligned only
    ]
    for kw in library:
        args = dict(x=xd, init=idev, filt=Mt, noise=nd, out=out, workspace=ws)
        args.update(kw)
        xa, ia, fa = args.pop("x"), args.pop("init"), args.pop("filt")
        with pytest.raises(VstError, match="status 1"):
            K.free_init_mix(xa, ia, fa, SCALE, **args)
    for wide in ((1, 1, 129, 2, 2), (1, 1, 2, 129, 2), (1, 1, 2, 2, 129)):   # past the supported range
        t = torch.zeros(wide, dtype=F32, device=cuda)
        with pytest.raises(VstError, match="status 3"):
            K.free_init_mix(t, None, torch.ones(wide[2:], dtype=F32, device=cuda), SCALE, noise=t.clone())
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (ws == 3.0).all() and torch.equal(idev.cpu(), init) and torch.equal(nd.cpu(), noise)
    # the longest supported axes run (one small volume each)
    for edge in ((1, 1, 128, 2, 3), (1, 1, 2, 128, 3), (1, 1, 3, 2, 128), (1, 1, 1, 128, 128)):
        xe, ie, ne = make(edge, seed=7)
        M, Mte = masks(edge)
        ref = pipeline(xe, ie, ne, M, F64)
        e32 = (pipeline(xe, ie, ne, M, F32) - ref).abs().max().item()
        got = K.free_init_mix(*dev(cuda, xe, ie), Mte.to(cuda), SCALE, noise=ne.to(cuda))
        err = (got.double().cpu() - ref).abs().max().item()
        print(f"[free_init] {edge}: kernel max err {err:.3e}, fp32 torch.fft max err {e32:.3e}")
        assert err <= 4 * e32, (edge, err, e32)


# ------------------------------------------------------------------ 5. the denoiser
SDXL = (0.9, 0.2, 1.3, 1.4)


@pytest.fixture(scope="module")
def tiny(cuda):
    from test_parity_gpu import _setup
    from video_style_transfer_amd.utils import build_unet
    cfg, sd, lat, enc, pooled, tids = _setup("tiny", 4, 16)
    return dict(enc=enc, pooled=pooled, unet=build_unet(cfg, state_dict=sd, device=cuda))


def denoiser(tiny, cuda, **kw):
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser
    enc, pooled = tiny["enc"], tiny["pooled"]
    den = AnimateDiffDenoiser(tiny["unet"], 4, 128, 128, num_inference_steps=10, device=cuda, **kw)
    den.set_prompt_embeds(enc[1:2], pooled[1:2], enc[0:1], pooled[0:1])
    return den


def manual_two_passes(tiny, cuda, seed, **kw):
    """Pass 0, the mix with the call's seed at counter 0 on stream 1, set_latents on a fresh denoiser, pass 1."""
    from video_style_transfer_amd import kernels as K
    from video_style_transfer_amd.free_init import FreeInit, dft_order, freq_filter
    den = denoiser(tiny, cuda, **kw)
    z_init = den.init_latents(seed).to(cuda, F32)
    x = den.run_steps().clone()
    filt = dft_order(freq_filter(*x.shape[2:], FreeInit())).to(cuda, F32)
    s, i = counters(cuda, seed, 0)
    mixed = K.free_init_mix(x, z_init, filt, float(den.scheduler.init_noise_sigma), seed=s, it=i, stream_id=1)
    fresh = denoiser(tiny, cuda, **kw)
    fresh.set_latents(mixed)
    return x, fresh.run_steps().clone()


@pytest.mark.parametrize("use_graph", [True, False])
def test_denoiser_one_iteration_is_the_plain_run(cuda, tiny, use_graph):
    from video_style_transfer_amd.free_init import FreeInit
    plain = denoiser(tiny, cuda, use_graph=use_graph)(seed=3).clone()
    one = denoiser(tiny, cuda, use_graph=use_graph, free_init=FreeInit(num_iters=1))(seed=3)
    assert torch.isfinite(plain).all() and torch.equal(one, plain)


@pytest.mark.parametrize("use_graph", [True, False])
def test_denoiser_two_iterations_equal_the_manual_composition(cuda, tiny, use_graph):
    from video_style_transfer_amd.free_init import FreeInit
    pass0, want = manual_two_passes(tiny, cuda, 3, use_graph=use_graph)
    den = denoiser(tiny, cuda, use_graph=use_graph, free_init=FreeInit(num_iters=2))
    g = None
    if use_graph:
        den.init_latents(3)
        den.run_steps(1)            # captures the step
        g = den.graph
        assert g is not None
    got = den(seed=3).clone()
    assert den.graph is g           # the second pass replays the step captured before the first: no recapture
    assert torch.isfinite(got).all() and torch.equal(got, want) and not torch.equal(got, pass0)
    assert torch.equal(den(seed=3), want)                     # a second call starts over: the same run
    assert not torch.equal(den(seed=4), want)
    den.disable_free_init()
    assert torch.equal(den(seed=3), pass0) and den.graph is g
    den.enable_free_init(num_iters=2)
    assert torch.equal(den(seed=3), want) and den.graph is g


def test_denoiser_composes_with_a_multistep_sampler(cuda, tiny):
    from video_style_transfer_amd.free_init import FreeInit
    from video_style_transfer_amd.scheduler import EulerDiscreteScheduler

    def kw():
        return dict(sampler="dpmpp_2m", scheduler=EulerDiscreteScheduler(sigma_schedule="karras"))
    pass0, want = manual_two_passes(tiny, cuda, 5, use_graph=False, **kw())
    for use_graph in (True, False):
        got = denoiser(tiny, cuda, use_graph=use_graph, free_init=FreeInit(num_iters=2), **kw())(seed=5)
        assert torch.equal(got, want) and not torch.equal(got, pass0)       # the history starts over with pass 1


def test_denoiser_composes_with_freeu(cuda, tiny):
    pass0, want = manual_two_passes(tiny, cuda, 5, use_graph=False, freeu=SDXL)
    for use_graph in (True, False):
        got = denoiser(tiny, cuda, use_graph=use_graph, free_init=dict(num_iters=2), freeu=SDXL)(seed=5)
        assert torch.isfinite(got).all() and torch.equal(got, want) and not torch.equal(got, pass0)


def test_denoiser_refuses_a_source_run(cuda, tiny):
    from video_style_transfer_amd.free_init import FreeInit
    den = denoiser(tiny, cuda, use_graph=False, free_init=FreeInit(num_iters=2))
    z0 = torch.zeros(1, 4, 4, 16, 16)
    with pytest.raises(ValueError, match="free_init.*source"):
        den(source=z0, strength=0.5)
    with pytest.raises(ValueError, match="free_init.*source"):
        den.set_source(z0, 0.5)
    with pytest.raises(ValueError, match="use_fast_sampling"):
        den.enable_free_init(use_fast_sampling=True)
