"""Few-step sampling on the GPU: vst_sampler_step against the fp32 restatement inside poisoned guard
bands, vst_cfg_rescale_factor against float64, and the denoiser on DPM-Solver++ 2M with Karras sigmas (against an fp32
restatement on top of oracle.unet.unet_forward; graph replay against eager; re-entry, interruption, the keep mask)."""
import pytest
import torch

from test_source_clip_gpu import guarded, guards_intact, same_bytes

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
B_, F_, H_, W_ = 2, 3, 5, 7  # HW = 35: no multiple of any vector width; B*F*HW = 210 pixels: one partial block
N_STEPS, GUIDANCE, PHI = 10, 7.5, 0.7


@pytest.fixture(scope="module")
def K(cuda):
    from video_style_transfer_amd import kernels
    return kernels


def karras(n=N_STEPS):
    from video_style_transfer_amd.scheduler import EulerDiscreteScheduler
    s = EulerDiscreteScheduler(sigma_schedule="karras")
    s.set_timesteps(n)
    return s


def tables(first_step=0, sampler="dpmpp_2m"):
    """(timesteps, sigmas, fp32 coefficient table) of the 10-step Karras schedule."""
    from video_style_transfer_amd.scheduler import sampler_coefficients
    s = karras()
    return s.timesteps, s.sigmas, sampler_coefficients(s.sigmas, sampler, first_step).float()


# ----------------------------------------------------------------------------- vst_sampler_step
def _mask(kind, mc, g):
    shape = (mc, F_, H_, W_)
    return (torch.rand(shape, generator=g) < 0.5).float() if kind == "binary" else torch.rand(shape, generator=g)


@pytest.mark.parametrize("ncopy", [1, 2])
@pytest.mark.parametrize("Cl", [4, 5])
def test_sampler_step_vs_reference(cuda, K, Cl, ncopy):
    """lat and hist after one step, first (c = 0) / middle / last (0, 1, 0) row, plain and masked, without and (ncopy 2)
    with a rescale factor.  Bound: 8 * 2^-24 * (|a| + |b| + |c|) * (max|x| + sigma * max|e|), eight roundings or FMA
    contractions of terms of that size (the chain e, e * factor, sigma * e, D, a x, b D, c hist, the blend).  Measured
    on an MI355X: at most 0.18 of the bound."""
    from video_style_transfer_amd.scheduler import rescale_factor_reference, sampler_step_reference
    g = torch.Generator().manual_seed(200 + 10 * Cl + ncopy)
    _, sig, co = tables()
    shape = (B_, Cl, F_, H_, W_)
    z0 = torch.randn(shape, generator=g)
    eps = torch.randn(shape, generator=g)
    noise = torch.randn(ncopy * B_ * F_ * H_ * W_, Cl, generator=g).to(BF)
    n = z0.numel()
    zb, zd = guarded(z0, cuda)
    eb, ed = guarded(eps, cuda)
    nb, nd = guarded(noise, cuda)
    sb, sd_ = guarded(sig, cuda)
    cb, cd = guarded(co, cuda)
    worst = 0.0
    for s in (0, 4, N_STEPS - 1):
        a, b, c = (abs(float(v)) for v in co[s])
        assert (c == 0) == (s != 4)
        lat = z0 + sig[s] * eps + 0.1 * torch.randn(shape, generator=g)  # latents as a run holds them at step s
        hist = torch.randn(shape, generator=g)
        stb, step = guarded(torch.tensor([s], dtype=torch.int32), cuda)
        for phi in ((0.0, PHI) if ncopy == 2 else (0.0,)):
            fac = rescale_factor_reference(noise, B_, GUIDANCE, phi) if phi > 0 else None
            fb, fd = guarded(fac, cuda) if fac is not None else (None, None)
            plain_out = None
            for kind, mc in ((None, 0), ("binary", 1), ("binary", B_), ("uniform", 1), ("uniform", B_)):
                m = _mask(kind, mc, g) if kind else None
                mb, md = guarded(m, cuda) if kind else (None, None)
                lb, ld = guarded(lat, cuda)
                hb, hd = guarded(hist, cuda)
                ins = [t for t in (zb, eb, nb, sb, cb, stb, fb, mb) if t is not None]
                before = [t.clone() for t in ins]
                kw = dict(z0=zd, eps=ed, mask=md) if kind else {}
                K.sampler_step(nd, ld, hd, sd_, cd, step, guidance=GUIDANCE, ncopy=ncopy, factor=fd, **kw)
                out, hout = ld.cpu(), hd.cpu()
                rkw = dict(z0=z0, eps=eps, mask=m) if kind else {}
                ref, D, rfac = sampler_step_reference(noise, lat, hist, sig, co, s, guidance=GUIDANCE, ncopy=ncopy,
                                                      guidance_rescale=phi, **rkw)
                assert (rfac is None) == (fac is None) and (fac is None or torch.equal(rfac, fac))
                e_hat = (lat - D) / sig[s]
                bound = 8 * 2.0 ** -24 * (a + b + c) * (lat.abs().max().item()
                                                        + float(sig[s]) * e_hat.abs().max().item())
                name = f"sampler_step Cl={Cl} ncopy={ncopy} step={s} phi={phi} mask={kind} mask_clips={mc}"
                err, herr = (out - ref).abs().max().item(), (hout - D).abs().max().item()
                worst = max(worst, err / bound, herr / bound)
                print(f"[sampler] {name}: max|err| lat={err:.3e} hist={herr:.3e} bound={bound:.3e}")
                assert torch.isfinite(out).all() and torch.isfinite(hout).all(), name
                assert err <= bound and herr <= bound, name
                assert guards_intact(lb, n) and guards_intact(hb, n), name
                assert all(same_bytes(x, y) for x, y in zip(before, ins)), name + ": an input changed"
                if kind is None:
                    plain_out = (out, hout)
                    continue
                assert torch.equal(hout, plain_out[1]), name  # the history is the unblended D
                kept = (m == 0).unsqueeze(1).expand(shape)
                free = (m == 1).unsqueeze(1).expand(shape)
                # kept pixels are the re-noised source, bit for bit, at every step; free ones the plain step's
                assert torch.equal(out[kept], (z0 + sig[s + 1] * eps)[kept]), name
                assert torch.equal(out[free], plain_out[0][free]), name
                if kind == "binary":
                    assert kept.any() and free.any()
    print(f"[sampler] Cl={Cl} ncopy={ncopy}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("masked", [False, True])
def test_history_poison_does_not_reach_the_latents(cuda, K, masked):
    """A c = 0 step does not read the history: NaN in it gives the latents of a zero history, and is overwritten."""
    g = torch.Generator().manual_seed(7)
    _, sig, co = tables(first_step=3)
    shape = (B_, 4, F_, H_, W_)
    lat, z0, eps = (torch.randn(shape, generator=g).to(cuda) for _ in range(3))
    noise = torch.randn(2 * B_ * F_ * H_ * W_, 4, generator=g).to(BF).to(cuda)
    m = (torch.rand(1, F_, H_, W_, generator=g) < 0.5).float().to(cuda)
    kw = dict(z0=z0, eps=eps, mask=m) if masked else {}
    for s in (0, 3, N_STEPS - 1):
        assert float(co[s, 2]) == 0.0
        step = torch.tensor([s], dtype=torch.int32, device=cuda)
        outs = []
        for fill in (float("nan"), 0.0):
            x, h = lat.clone(), torch.full(shape, fill, device=cuda)
            K.sampler_step(noise, x, h, sig.to(cuda), co.to(cuda), step, guidance=GUIDANCE, **kw)
            assert torch.isfinite(x).all() and torch.isfinite(h).all()
            outs.append((x, h))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # and a second-order row does read it
    x, h = lat.clone(), torch.full(shape, float("nan"), device=cuda)
    K.sampler_step(noise, x, h, sig.to(cuda), co.to(cuda), torch.tensor([5], dtype=torch.int32, device=cuda),
                   guidance=GUIDANCE, **kw)
    assert torch.isnan(x).any() and torch.isfinite(h).all()


# ----------------------------------------------------------------------------- vst_cfg_rescale_factor
# (B, Cl, F, H, W): 420 values per clip (less than one 1024-value partial block); 2340 (three blocks, the last one
# ragged: 292 values); 525 (an odd count: clips start at odd element offsets)
RESCALE_SHAPES = [(2, 4, 3, 5, 7), (2, 4, 5, 9, 13), (3, 5, 3, 5, 7)]


@pytest.mark.parametrize("mean,std", [(0.0, 1.0), (3.0, 0.5)])
@pytest.mark.parametrize("shape", RESCALE_SHAPES)
def test_cfg_rescale_factor_vs_float64(cuda, K, shape, mean, std):
    """Relative error of the factor <= 1e-5 (ten times the O(log n * 2^-24) of a fixed-order Chan merge) against
    float64 on the same bf16 values; a mean of 3 at std 0.5 is what a sum of squares would cancel on."""
    B, Cl, F, H, W = shape
    g = torch.Generator().manual_seed(sum(shape))
    noise = (mean + std * torch.randn(2 * B * F * H * W, Cl, generator=g)).to(BF)
    n2 = noise.double().reshape(2, B, -1)
    e = n2[0] + GUIDANCE * (n2[1] - n2[0])
    want = PHI * n2[1].std(dim=1) / e.std(dim=1) + (1 - PHI)
    nb, nd = guarded(noise, cuda)
    ws = K.cfg_rescale_workspace(shape, cuda)
    wb, wd = guarded(torch.zeros(ws.numel()), cuda)
    fb, fd = guarded(torch.zeros(B), cuda)
    keep = nb.clone()
    r = K.cfg_rescale_factor(nd, shape, guidance=GUIDANCE, phi=PHI, out=fd, workspace=wd)
    assert r is fd
    got = fd.cpu()
    err = ((got.double() - want).abs() / want.abs()).max().item()
    print(f"[sampler] rescale factor {shape} mean={mean} std={std}: {got.tolist()} max rel err={err:.3e}")
    assert torch.isfinite(got).all() and err <= 1e-5
    assert guards_intact(fb, B) and guards_intact(wb, ws.numel()) and same_bytes(nb, keep)
    # the same bits on a second call, and from the allocating form
    first = fd.clone()
    K.cfg_rescale_factor(nd, shape, guidance=GUIDANCE, phi=PHI, out=fd, workspace=wd)
    assert same_bytes(fd, first) and same_bytes(K.cfg_rescale_factor(nd, shape, guidance=GUIDANCE, phi=PHI), first)
    # the fp32 restatement agrees to its own rounding
    from video_style_transfer_amd.scheduler import rescale_factor_reference
    assert torch.allclose(got, rescale_factor_reference(noise, B, GUIDANCE, PHI), rtol=1e-4)
    # phi = 0 is the identity, exactly
    assert torch.equal(K.cfg_rescale_factor(nd, shape, guidance=GUIDANCE, phi=0.0).cpu(), torch.ones(B))


def test_cfg_rescale_factor_of_a_constant_is_one(cuda, K):
    """std(e_b) = 0: factor 1 where the reference's division gives NaN (clip 0 constant, clip 1 not)."""
    shape = (2, 4, 5, 9, 13)
    n = 4 * 5 * 9 * 13
    g = torch.Generator().manual_seed(3)
    noise = torch.randn(2, 2, n, generator=g)
    noise[:, 0] = 1.5
    noise = noise.reshape(-1, 4).to(BF).to(cuda)
    got = K.cfg_rescale_factor(noise, shape, guidance=GUIDANCE, phi=PHI).cpu()
    assert float(got[0]) == 1.0 and torch.isfinite(got).all() and 0.3 < float(got[1]) < 1.0


def test_sampler_wrappers_refuse_bad_arguments(cuda, K):
    from video_style_transfer_amd._lib import VstError
    _, sig, co = tables()
    sig, co = sig.to(cuda), co.to(cuda)
    step = torch.zeros(1, dtype=torch.int32, device=cuda)
    shape = (B_, 4, F_, H_, W_)
    z, h = torch.zeros(shape, device=cuda), torch.zeros(shape, device=cuda)
    noise = torch.zeros(2 * B_ * F_ * H_ * W_, 4, dtype=BF, device=cuda)
    m = torch.ones(1, F_, H_, W_, device=cuda)
    fac = torch.full((B_,), 7.0, device=cuda)
    out = torch.zeros(B_, device=cuda)
    S, R = K.sampler_step, K.cfg_rescale_factor
    bad = [lambda: S(noise.float(), z, h, sig, co, step), lambda: S(noise[:-1], z, h, sig, co, step),
           lambda: S(noise, z, h, sig, co, step, ncopy=1), lambda: S(noise, z, h, sig, co, step, ncopy=3),
           lambda: S(noise, z, z, sig, co, step), lambda: S(noise, z, h[:1], sig, co, step),
           lambda: S(noise, z, h.double(), sig, co, step), lambda: S(noise, z[0], h[0], sig, co, step),
           lambda: S(noise, z.transpose(3, 4), h, sig, co, step), lambda: S(noise, z, h, sig.double(), co, step),
           lambda: S(noise, z, h, sig, co[:-1], step), lambda: S(noise, z, h, sig, co.double(), step),
           lambda: S(noise, z, h, sig, co.t(), step), lambda: S(noise, z, h, sig, co, step.long()),
           lambda: S(noise, z, h, sig, co, step, factor=fac[:1]), lambda: S(noise, z, h, sig, co, step, factor=fac.cpu()),
           lambda: S(noise[:210], z, h, sig, co, step, ncopy=1, factor=fac),
           lambda: S(noise, z, h, sig, co, step, mask=m), lambda: S(noise, z, h, sig, co, step, z0=z, eps=z),
           lambda: S(noise, z, h, sig, co, step, z0=z[:1], eps=z, mask=m),
           lambda: S(noise, z, h, sig, co, step, z0=z, eps=z.half(), mask=m),
           lambda: S(noise, z, h, sig, co, step, z0=z, eps=z, mask=m[:, :2]),
           lambda: S(noise, z, h, sig, co, step, z0=z, eps=z, mask=torch.ones(3, F_, H_, W_, device=cuda)),
           lambda: R(noise.float(), shape, guidance=7.5, phi=0.5, out=out),
           lambda: R(noise[:-1], shape, guidance=7.5, phi=0.5, out=out),
           lambda: R(noise, shape[:4], guidance=7.5, phi=0.5, out=out),
           lambda: R(noise, (0,) + shape[1:], guidance=7.5, phi=0.5, out=out),
           lambda: R(noise, shape, guidance=7.5, phi=float("nan"), out=out),
           lambda: R(noise, shape, guidance=7.5, phi=1.5, out=out),
           lambda: R(noise, shape, guidance=7.5, phi=-0.1, out=out),
           lambda: R(noise, shape, guidance=7.5, phi=0.5, out=out[:1]),
           lambda: R(noise, shape, guidance=7.5, phi=0.5, out=out.double()),
           lambda: R(noise, shape, guidance=7.5, phi=0.5, out=out, workspace=torch.zeros(3, device=cuda)),
           lambda: R(noise, shape, guidance=7.5, phi=0.5, out=out, workspace=torch.zeros(64))]
    for i, fn in enumerate(bad):
        with pytest.raises(VstError):
            fn()
            pytest.fail(f"case {i} was accepted")
    assert not z.any() and not h.any() and not out.any()


# ----------------------------------------------------------------------------- the loop
@pytest.fixture(scope="module")
def tiny(cuda):
    from test_parity_gpu import _setup
    from video_style_transfer_amd.utils import build_unet
    cfg, sd, lat, enc, pooled, tids = _setup("tiny", 4, 16, seed=5, B=2)
    unet = build_unet(cfg, state_dict=sd, device=cuda)
    g = torch.Generator().manual_seed(77)
    z0 = torch.randn(1, 4, 4, 16, 16, generator=g)
    mask = (torch.rand(1, 4, 16, 16, generator=g) < 0.5).float()
    return dict(cfg=cfg, sd=sd, enc=enc, pooled=pooled, tids=tids, unet=unet, z0=z0, mask=mask)


def _denoiser(tiny, cuda, use_graph=True, sampler="dpmpp_2m", phi=0.0, new_args=True, **kw):
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser
    if new_args:
        kw.update(sampler=sampler, guidance_rescale=phi)
    kw.setdefault("scheduler", karras())
    den = AnimateDiffDenoiser(tiny["unet"], 4, 128, 128, num_inference_steps=N_STEPS, guidance_scale=GUIDANCE,
                              device=cuda, use_graph=use_graph, **kw)
    den.set_prompt_embeds(tiny["enc"][1:2], tiny["pooled"][1:2], tiny["enc"][0:1], tiny["pooled"][0:1])
    return den


def _eps(shape, seed):
    return torch.randn(shape, generator=torch.Generator(device="cpu").manual_seed(seed))


def _rows(t):
    """(1, C, F, H, W) UNet output -> token rows (F * HW, C), the layout the sampler step reads."""
    return t[0].permute(1, 2, 3, 0).reshape(-1, t.shape[1])


def _restated_run(tiny, lat, t_start, phi=0.0, steps=None, z0=None, eps=None, mask=None):
    """DESIGN.md §15 in fp32 on the CPU: steps t_start .. of DPM-Solver++ 2M on the Karras tables, CFG as two UNet calls
    per step, the whole update by sampler_step_reference (first order at t_start, then on its own history)."""
    from oracle.unet import unet_forward
    from video_style_transfer_amd.scheduler import sampler_step_reference
    ts, sig, co = tables(first_step=t_start)
    cfgd, sd, enc, pooled, tid = tiny["cfg"].to_dict(), tiny["sd"], tiny["enc"], tiny["pooled"], tiny["tids"][:1]
    hist = torch.full_like(lat, float("nan"))  # never read before it is written
    for i in range(t_start, N_STEPS if steps is None else t_start + steps):
        scaled = lat / ((sig[i] ** 2 + 1) ** 0.5)
        nu = unet_forward(sd, cfgd, scaled, ts[i:i + 1], enc[0:1], pooled[0:1], tid)
        nc = unet_forward(sd, cfgd, scaled, ts[i:i + 1], enc[1:2], pooled[1:2], tid)
        lat, hist, _ = sampler_step_reference(torch.cat([_rows(nu), _rows(nc)]), lat, hist, sig, co, i,
                                              guidance=GUIDANCE, guidance_rescale=phi, z0=z0, eps=eps, mask=mask)
    return lat


@pytest.fixture(scope="module")
def one_forward_error(tiny, cuda):
    """rel-L2 of e_hat = u + g (c - u) from ONE forward of the existing UNet against unet_forward on the same scaled
    input, at the middle step of the Karras schedule (its fractional timestep).  It is the error every step's update
    carries; the code under test adds none to it."""
    from oracle.unet import unet_forward
    from test_parity_gpu import rel
    ts, sig, _ = tables()
    z0, enc, pooled, tids = tiny["z0"], tiny["enc"], tiny["pooled"], tiny["tids"]
    lat = z0 + sig[5] * _eps(z0.shape, 42)
    scaled = (lat / ((sig[5] ** 2 + 1) ** 0.5)).expand(2, -1, -1, -1, -1).contiguous()
    t = ts[5:6].expand(2).contiguous()
    ref = unet_forward(tiny["sd"], tiny["cfg"].to_dict(), scaled, t, enc, pooled, tids)
    out = tiny["unet"](scaled.to(cuda), t.to(cuda), enc.to(cuda),
                       added_cond_kwargs={"text_embeds": pooled.to(cuda), "time_ids": tids.to(cuda)}).sample
    ec, _ = rel(out[0] + GUIDANCE * (out[1] - out[0]), ref[0] + GUIDANCE * (ref[1] - ref[0]))
    print(f"[sampler] one forward at step 5 (t={float(ts[5]):.2f}): e_hat rel_l2={ec:.3e}")
    return ec


@pytest.fixture(scope="module")
def full_runs(tiny, cuda):
    """The whole 10-step run from noise (seed 3), captured graph, without and with guidance rescale: shared."""
    res = {}
    for phi in (0.0, PHI):
        den = _denoiser(tiny, cuda, True, phi=phi)
        start = den.init_latents(3)
        out = den.run_steps().clone()
        assert den.graph is not None and int(den.step_idx) == 0
        res[phi] = (out, start)
    return res


@pytest.mark.parametrize("phi", [0.0, PHI])
def test_dpmpp_2m_run_vs_restatement(cuda, tiny, full_runs, one_forward_error, phi):
    """The accumulated update against the fp32 restatement: rel-L2 <= 1.5 * W * (one forward's e_hat error), W the
    largest (|b| + |c|) / |b + c| of the table (2.12 at 10 steps): the second-order rows weigh two forwards' errors
    with opposite signs.  Figures on an MI355X: one forward 6.93e-2, W = 2.119, update rel-L2 2.83e-2
    (phi 0) and 2.85e-2 (phi 0.7), 0.19 of what is allowed."""
    from test_parity_gpu import rel
    _, _, co = tables()
    W = float(((co[:, 1].abs() + co[:, 2].abs()) / (co[:, 1] + co[:, 2]).abs()).max())
    out, start = full_runs[phi]
    ref = _restated_run(tiny, start, 0, phi)
    assert torch.isfinite(out).all()
    eu, _ = rel(out.cpu() - start, ref - start)
    ef, _ = rel(out, ref)
    print(f"[sampler] dpmpp_2m phi={phi}: update rel_l2={eu:.3e} (latents {ef:.3e}), one forward rel_l2="
          f"{one_forward_error:.3e}, W={W:.3f}, ratio={eu / (W * one_forward_error):.3f}")
    assert 2.0 < W < 2.2
    assert eu <= 1.5 * W * one_forward_error, (eu, W, one_forward_error)


def test_rescale_changes_the_run(full_runs):
    assert not torch.equal(full_runs[0.0][0], full_runs[PHI][0])


@pytest.mark.parametrize("phi", [0.0, PHI])
def test_graph_equals_eager_and_survives_new_source(cuda, tiny, full_runs, phi):
    z0 = tiny["z0"]
    dg, de = _denoiser(tiny, cuda, True, phi=phi), _denoiser(tiny, cuda, False, phi=phi)
    og, oe = dg(seed=3).clone(), de(seed=3).clone()
    assert de.graph is None and dg.graph is not None
    assert torch.equal(og, oe) and torch.equal(og, full_runs[phi][0])
    # source runs at two strengths on the same captured step: the table is rewritten in place
    g0, ptrs = dg.graph, (dg.hist.data_ptr(), dg.coef.data_ptr(), dg.lat.data_ptr())
    for strength, t_start, seed in ((0.3, 7, 42), (0.5, 5, 7)):
        og = dg(source=z0, strength=strength, seed=seed).clone()
        oe = de(source=z0, strength=strength, seed=seed).clone()
        assert dg.graph is g0 and dg.t_start == t_start
        assert ptrs == (dg.hist.data_ptr(), dg.coef.data_ptr(), dg.lat.data_ptr())
        assert torch.equal(dg.coef.cpu(), tables(first_step=t_start)[2])
        assert torch.isfinite(og).all() and torch.equal(og, oe)
    # and a plain run afterwards is the plain run again (first order at step 0 again)
    assert torch.equal(dg(seed=3), full_runs[phi][0]) and dg.graph is g0


def test_first_step_after_reentry_is_first_order(cuda, tiny, one_forward_error):
    """set_source at strength 0.5 enters at step 5: its row has c = 0, so the history left by the run before (here:
    NaN) is not read; one step against the restatement's first step, gated as the whole run is."""
    from test_parity_gpu import rel
    z0 = tiny["z0"]
    den = _denoiser(tiny, cuda, True)
    den(seed=3)  # a whole run first: the table is the plain one, the history that run's
    den.set_source(z0, 0.5, seed=7)
    assert den.t_start == 5 and float(den.coef[5, 2]) == 0.0 and float(den.coef[6, 2]) != 0.0
    den.hist.fill_(float("nan"))
    start = den.lat.clone().cpu()
    out = den.run_steps(1).clone().cpu()
    assert torch.isfinite(out).all() and torch.isfinite(den.hist).all() and int(den.step_idx) == 6
    _, sig, _ = tables()
    torch.testing.assert_close(start, z0 + sig[5] * _eps(z0.shape, 7), rtol=2e-6, atol=2e-5)
    ref = _restated_run(tiny, start, 5, steps=1)
    eu, _ = rel(out - start, ref - start)
    print(f"[sampler] first step after re-entry: update rel_l2={eu:.3e}, one forward rel_l2={one_forward_error:.3e}")
    assert eu <= 1.5 * one_forward_error  # a first-order row: b alone, W = 1


@pytest.mark.parametrize("use_graph", [True, False])
def test_interrupted_run_equals_uninterrupted(cuda, tiny, full_runs, use_graph):
    den = _denoiser(tiny, cuda, use_graph)
    den.init_latents(3)
    den.run_steps(3)
    assert int(den.step_idx) == 3
    assert torch.equal(den.run_steps(), full_runs[0.0][0]) and int(den.step_idx) == 0


def test_history_survives_a_recapture(cuda, tiny, full_runs):
    """run_steps(k), set_lora_gates (the first call drops the captured step), run_steps(): the warm-up step of the
    new capture must not leave its own D in the history.  Gates of 1 are the plain run."""
    den = _denoiser(tiny, cuda, True)
    den.init_latents(3)
    den.run_steps(3)
    g0 = den.graph
    den.set_lora_gates(1.0, 1.0)
    assert den.graph is None
    out = den.run_steps().clone()
    assert den.graph is not None and den.graph is not g0
    ref = _denoiser(tiny, cuda, False)
    ref.init_latents(3)
    ref.run_steps(3)
    ref.set_lora_gates(1.0, 1.0)
    assert torch.equal(out, ref.run_steps())
    den.clear_lora_gates()
    ref.clear_lora_gates()


@pytest.mark.parametrize("phi", [0.0, PHI])
def test_masked_dpmpp_2m_keeps_the_source(cuda, tiny, phi):
    z0, mask = tiny["z0"], tiny["mask"]
    outs = []
    for use_graph in (True, False):
        den = _denoiser(tiny, cuda, use_graph, phi=phi)
        outs.append(den(source=z0, strength=0.5, mask=mask, seed=42).clone())
        assert den.masked and den.t_start == 5
    out = outs[0].cpu()
    assert torch.isfinite(out).all() and torch.equal(outs[0], outs[1])
    kept = (mask == 0).unsqueeze(1).expand_as(out)
    assert kept.any() and torch.equal(out[kept], z0[kept])
    assert not torch.equal(out[~kept], z0[~kept])


def test_defaults_are_the_unchanged_step(cuda, tiny, K, monkeypatch):
    """sampler="euler" with guidance_rescale 0 is a denoiser built without the new arguments, bit for bit, and never
    calls the new kernels; Euler with a rescale goes through them (the Euler table) and differs."""
    from video_style_transfer_amd.scheduler import EulerDiscreteScheduler
    calls = []
    real_step, real_factor = K.sampler_step, K.cfg_rescale_factor
    monkeypatch.setattr(K, "sampler_step", lambda *a, **k: (calls.append("step"), real_step(*a, **k))[1])
    monkeypatch.setattr(K, "cfg_rescale_factor", lambda *a, **k: (calls.append("factor"), real_factor(*a, **k))[1])
    outs = {}
    for key, kw in (("old", dict(new_args=False)), ("new", dict(sampler="euler", phi=0.0))):
        for use_graph in (True, False):
            den = _denoiser(tiny, cuda, use_graph, scheduler=EulerDiscreteScheduler(), **kw)
            assert not den.table_step and den.hist is None and den.coef is None and den.factor is None
            outs[key, use_graph] = den(seed=3).clone()
    assert calls == []
    assert all(torch.equal(outs["old", True], o) for o in outs.values())
    # the Euler table through vst_sampler_step is the Euler step to rounding (a x + b D against x + ds e)
    den = _denoiser(tiny, cuda, False, sampler="euler", phi=PHI, scheduler=EulerDiscreteScheduler())
    out = den(seed=3)
    assert calls.count("step") == N_STEPS and calls.count("factor") == N_STEPS
    assert torch.isfinite(out).all() and not torch.equal(out, outs["old", True])
