"""Stochastic samplers on the GPU: the counter layout of vst_noise_bits against the host Philox, the
normals against float64, their moments, vst_sampler_step_noise against the fp32 restatement inside poisoned guard
bands, and the denoiser on Euler ancestral, DPM-Solver++ 2M SDE and LCM (graph replay against eager, seeds,
interruption, the keep mask, and the run against an fp32 restatement on oracle.unet.unet_forward fed the device's
noise)."""
import numpy as np
import pytest
import torch

from test_sampler_gpu import _eps, _mask, _rows, karras, tiny  # noqa: F401  (tiny: the shared module fixture)
from test_source_clip_gpu import guarded, guards_intact, same_bytes

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
B_, F_, H_, W_ = 2, 3, 5, 7  # HW = 35: no multiple of any vector width; B*F*HW = 210 pixels: one partial block
N_STEPS, GUIDANCE, PHI = 10, 7.5, 0.7
SEEDS = (12345, 2 ** 40 + 5)  # the second needs the upper key word
CLS = (4, 5, 9)  # the 4-channel path; a ragged second group; three groups


@pytest.fixture(scope="module")
def K(cuda):
    from video_style_transfer_amd import kernels
    return kernels


def dev_seed(seed, cuda):
    v = seed & (2 ** 64 - 1)
    return torch.tensor([v - 2 ** 64 if v >= 2 ** 63 else v], dtype=torch.int64, device=cuda)


def dev_step(s, cuda):
    return torch.tensor([s], dtype=torch.int32, device=cuda)


def schedule(sampler):
    from video_style_transfer_amd.scheduler import EulerDiscreteScheduler
    if sampler != "lcm":
        return karras()
    s = EulerDiscreteScheduler(timestep_spacing="lcm")
    s.set_timesteps(N_STEPS)
    return s


def tables(sampler="dpmpp_2m_sde", first_step=0, eta=1.0):
    """(timesteps, sigmas, fp32 (a, b, c, d) table) of the sampler's 10-step schedule."""
    from video_style_transfer_amd.scheduler import sampler_coefficients
    s = schedule(sampler)
    return s.timesteps, s.sigmas, sampler_coefficients(s.sigmas, sampler, first_step, eta, s.timesteps).float()


# ----------------------------------------------------------------------------- the noise
@pytest.mark.parametrize("Cl", CLS)
def test_noise_bits_are_the_host_philox(cuda, K, Cl):
    """Every word, for two seeds (one above 2^32), steps 0 and 7, streams 0 and 3; and frames [2, 5) of a 5-frame clip
    are the slice of the whole clip's call."""
    from video_style_transfer_amd.scheduler import noise_reference
    shape = (B_, Cl, F_, H_, W_)
    n = B_ * Cl * F_ * H_ * W_
    for seed in SEEDS:
        sd = dev_seed(seed, cuda)
        for s in (0, 7):
            for stream in (0, 3):
                ob, od = guarded(torch.zeros(shape, dtype=torch.int32), cuda)
                r = K.noise_bits(sd, dev_step(s, cuda), shape, stream_id=stream, out=od)
                assert r is od and guards_intact(ob, n)
                want, _ = noise_reference(seed, s, stream, shape)
                assert torch.equal(od.cpu().view(torch.uint32), want), (seed, s, stream)
        whole = K.noise_bits(sd, dev_step(7, cuda), (B_, Cl, 5, H_, W_))
        ob, od = guarded(torch.zeros(shape, dtype=torch.int32), cuda)
        K.noise_bits(sd, dev_step(7, cuda), shape, F_total=5, f0=2, out=od)
        assert guards_intact(ob, n) and torch.equal(od, whole[:, :, 2:5])
        assert torch.equal(od.cpu().view(torch.uint32), noise_reference(seed, 7, 0, shape, F_total=5, f0=2)[0])
        assert int(sd.cpu()) == (seed if seed < 2 ** 63 else seed - 2 ** 64)  # the seed is only read


@pytest.mark.parametrize("Cl", CLS)
def test_noise_normal_vs_float64(cuda, K, Cl):
    """The u_k are exact, so the error is that of logf, sqrtf, sinpif / cospif (3, 3 and 4 ulp by the OpenCL-profile
    bounds HIP's math library documents) and one product: gate 16 * 2^-23 * max(1, r) per element, r = sqrt(-2 ln u0)
    of the element's pair.  Measured on an MI355X: the worst error is 0.080 (Cl 4) and 0.085 (Cl 5, 9) of
    the gate."""
    from video_style_transfer_amd.scheduler import noise_reference
    shape = (B_, Cl, F_, H_, W_)
    n = B_ * Cl * F_ * H_ * W_
    worst = 0.0
    for seed in SEEDS:
        for s, stream in ((0, 0), (7, 3)):
            ob, od = guarded(torch.zeros(shape), cuda)
            K.noise_normal(dev_seed(seed, cuda), dev_step(s, cuda), shape, stream_id=stream, out=od)
            bits, want = noise_reference(seed, s, stream, shape)
            first = np.arange(Cl) & ~1  # the channel holding u0 of each channel's pair
            u0 = ((bits.numpy()[:, first] >> 9).astype(np.float64) + 0.5) * 2.0 ** -23
            gate = 16 * 2.0 ** -23 * np.maximum(1.0, np.sqrt(-2.0 * np.log(u0)))
            got = od.cpu()
            ratio = float(((got.double() - want).abs() / torch.from_numpy(gate)).max())
            worst = max(worst, ratio)
            assert torch.isfinite(got).all() and guards_intact(ob, n)
            assert ratio <= 1.0, (seed, s, stream, ratio)
    print(f"[noise] Cl={Cl}: worst |normal - fp64| / gate = {worst:.3f}")


def test_noise_moments(cuda, K):
    """One (1, 4, 16, 64, 64) fill, N = 2^18 standard normals: |mean| <= 5 / sqrt(N) and |var - 1| <= 5 sqrt(2 / N)
    (five standard errors of the two estimators), and the sample correlation between steps 0 and 1 and between two
    seeds is within 5 / sqrt(N) of 0."""
    shape = (1, 4, 16, 64, 64)
    N = 2 ** 18
    a = K.noise_normal(dev_seed(SEEDS[0], cuda), dev_step(0, cuda), shape).cpu().double().reshape(-1)
    b = K.noise_normal(dev_seed(SEEDS[0], cuda), dev_step(1, cuda), shape).cpu().double().reshape(-1)
    c = K.noise_normal(dev_seed(SEEDS[1], cuda), dev_step(0, cuda), shape).cpu().double().reshape(-1)
    assert a.numel() == N
    mean, var = float(a.mean()), float(a.var())
    corr = [float(torch.corrcoef(torch.stack([a, x]))[0, 1]) for x in (b, c)]
    print(f"[noise] N=2^18: mean={mean:.3e} (gate {5 / N ** 0.5:.3e}) var-1={var - 1:.3e} (gate "
          f"{5 * (2 / N) ** 0.5:.3e}) corr step={corr[0]:.3e} seed={corr[1]:.3e}")
    assert abs(mean) <= 5 / N ** 0.5
    assert abs(var - 1) <= 5 * (2 / N) ** 0.5
    assert all(abs(r) <= 5 / N ** 0.5 for r in corr)


# ----------------------------------------------------------------------------- vst_sampler_step_noise
@pytest.mark.parametrize("ncopy", [1, 2])
@pytest.mark.parametrize("Cl", CLS)
def test_sampler_step_noise_vs_reference(cuda, K, Cl, ncopy):
    """lat and hist after one step of the DPM-Solver++ 2M SDE table, first (c = 0) / middle / last (0, 1, 0, 0) row,
    plain and masked, without and (ncopy 2) with a rescale factor, against sampler_step_reference fed the device's
    xi.  Bound: test_sampler_step_vs_reference's 8 * 2^-24 * (|a| + |b| + |c|) * (max|x| + sigma * max|e|) plus
    2^-24 * 2 |d| max|xi| for one more product and sum.  With the d column zeroed the bits are K.sampler_step's on the
    3-column table.  Measured on an MI355X: at most 0.21 of the bound (Cl 5, ncopy 2; 0.15 at Cl 4)."""
    from video_style_transfer_amd.scheduler import rescale_factor_reference, sampler_step_reference
    g = torch.Generator().manual_seed(300 + 10 * Cl + ncopy)
    seed = SEEDS[1]
    _, sig, co = tables()
    co0 = co.clone()
    co0[:, 3] = 0
    co3 = co[:, :3].contiguous()
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
    seedb, seedd = guarded(dev_seed(seed, cuda).cpu(), cuda)
    worst = 0.0
    for s in (0, 4, N_STEPS - 1):
        a, b, c, d = (abs(float(v)) for v in co[s])
        assert (c == 0) == (s != 4) and (d == 0) == (s == N_STEPS - 1)
        lat = z0 + sig[s] * eps + 0.1 * torch.randn(shape, generator=g)  # latents as a run holds them at step s
        hist = torch.randn(shape, generator=g)
        stb, step = guarded(torch.tensor([s], dtype=torch.int32), cuda)
        xi = K.noise_normal(seedd, step, shape).cpu()
        for phi in ((0.0, PHI) if ncopy == 2 else (0.0,)):
            fac = rescale_factor_reference(noise, B_, GUIDANCE, phi) if phi > 0 else None
            fb, fd = guarded(fac, cuda) if fac is not None else (None, None)
            plain_out = None
            for kind, mc in ((None, 0), ("binary", 1), ("binary", B_), ("uniform", 1), ("uniform", B_)):
                m = _mask(kind, mc, g) if kind else None
                mb, md = guarded(m, cuda) if kind else (None, None)
                lb, ld = guarded(lat, cuda)
                hb, hd = guarded(hist, cuda)
                ins = [t for t in (zb, eb, nb, sb, cb, stb, seedb, fb, mb) if t is not None]
                before = [t.clone() for t in ins]
                kw = dict(z0=zd, eps=ed, mask=md) if kind else {}
                K.sampler_step_noise(nd, ld, hd, sd_, cd, step, seedd, guidance=GUIDANCE, ncopy=ncopy, factor=fd, **kw)
                out, hout = ld.cpu(), hd.cpu()
                rkw = dict(z0=z0, eps=eps, mask=m) if kind else {}
                ref, D, _ = sampler_step_reference(noise, lat, hist, sig, co, s, guidance=GUIDANCE, ncopy=ncopy,
                                                   guidance_rescale=phi, xi=xi, **rkw)
                e_hat = (lat - D) / sig[s]
                bound = (8 * 2.0 ** -24 * (a + b + c) * (lat.abs().max().item()
                                                         + float(sig[s]) * e_hat.abs().max().item())
                         + 2.0 ** -24 * 2 * d * xi.abs().max().item())
                name = f"sampler_step_noise Cl={Cl} ncopy={ncopy} step={s} phi={phi} mask={kind} mask_clips={mc}"
                err, herr = (out - ref).abs().max().item(), (hout - D).abs().max().item()
                worst = max(worst, err / bound, herr / bound)
                print(f"[noise] {name}: max|err| lat={err:.3e} hist={herr:.3e} bound={bound:.3e}")
                assert torch.isfinite(out).all() and torch.isfinite(hout).all(), name
                assert err <= bound and herr <= bound, name
                assert guards_intact(lb, n) and guards_intact(hb, n), name
                assert all(same_bytes(x, y) for x, y in zip(before, ins)), name + ": an input changed"
                # d = 0 in every row: no noise, the deterministic step's bits
                l0, h0 = lat.to(cuda), hist.to(cuda)
                l3, h3 = lat.to(cuda), hist.to(cuda)
                K.sampler_step_noise(nd, l0, h0, sd_, co0.to(cuda), step, seedd, guidance=GUIDANCE, ncopy=ncopy,
                                     factor=fd, **kw)
                K.sampler_step(nd, l3, h3, sd_, co3.to(cuda), step, guidance=GUIDANCE, ncopy=ncopy, factor=fd, **kw)
                assert torch.equal(l0, l3) and torch.equal(h0, h3), name + ": d = 0 is not the deterministic step"
                assert torch.equal(h0.cpu(), hout), name  # the history does not see the noise
                if kind is None:
                    plain_out = (out, hout)
                    assert (d == 0) == torch.equal(out, l3.cpu()), name  # and d != 0 does add it
                    continue
                assert torch.equal(hout, plain_out[1]), name  # the history is the unblended D
                kept = (m == 0).unsqueeze(1).expand(shape)
                free = (m == 1).unsqueeze(1).expand(shape)
                # kept pixels are the re-noised source with the run's fixed eps, bit for bit; free ones the plain step's
                assert torch.equal(out[kept], (z0 + sig[s + 1] * eps)[kept]), name
                assert torch.equal(out[free], plain_out[0][free]), name
                if kind == "binary":
                    assert kept.any() and free.any()
    print(f"[noise] Cl={Cl} ncopy={ncopy}: worst error / bound = {worst:.3f}")


def test_step_on_a_frame_window_draws_the_whole_clips_noise(cuda, K):
    """Frames [2, 5) of a 5-frame clip stepped alone (F_total 5, f0 2) store what the whole clip's step stores there:
    a frame shard draws the noise of the unsharded run."""
    g = torch.Generator().manual_seed(9)
    _, sig, co = tables()
    sig, co = sig.to(cuda), co.to(cuda)
    Ft, f0, Fw = 5, 2, 3
    shape = (B_, 4, Ft, H_, W_)
    lat, hist = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    noise = torch.randn(2, B_, Ft, H_ * W_, 4, generator=g).to(BF)
    step, seed = dev_step(4, cuda), dev_seed(SEEDS[0], cuda)
    lw, hw_ = lat.to(cuda), hist.to(cuda)
    K.sampler_step_noise(noise.reshape(-1, 4).to(cuda), lw, hw_, sig, co, step, seed, guidance=GUIDANCE)
    lp = lat[:, :, f0:f0 + Fw].contiguous().to(cuda)
    hp = hist[:, :, f0:f0 + Fw].contiguous().to(cuda)
    npart = noise[:, :, f0:f0 + Fw].reshape(-1, 4).contiguous().to(cuda)
    K.sampler_step_noise(npart, lp, hp, sig, co, step, seed, F_total=Ft, f0=f0, guidance=GUIDANCE)
    assert torch.equal(lp, lw[:, :, f0:f0 + Fw]) and torch.equal(hp, hw_[:, :, f0:f0 + Fw])
    lq = lat[:, :, f0:f0 + Fw].contiguous().to(cuda)
    K.sampler_step_noise(npart, lq, hp.clone(), sig, co, step, seed, guidance=GUIDANCE)  # as a clip of its own
    assert not torch.equal(lq, lp)


def test_noise_wrappers_refuse_bad_arguments(cuda, K):
    from video_style_transfer_amd._lib import VstError
    _, sig, co = tables()
    sig, co = sig.to(cuda), co.to(cuda)
    step, seed = dev_step(0, cuda), dev_seed(1, cuda)
    shape = (B_, 4, F_, H_, W_)
    z, h = torch.zeros(shape, device=cuda), torch.zeros(shape, device=cuda)
    noise = torch.zeros(2 * B_ * F_ * H_ * W_, 4, dtype=BF, device=cuda)
    m = torch.ones(1, F_, H_, W_, device=cuda)
    fac = torch.full((B_,), 7.0, device=cuda)
    ob, on = torch.zeros(shape, dtype=torch.int32, device=cuda), torch.zeros(shape, device=cuda)
    S, NB, NN = K.sampler_step_noise, K.noise_bits, K.noise_normal
    bad = [lambda: S(noise.float(), z, h, sig, co, step, seed), lambda: S(noise[:-1], z, h, sig, co, step, seed),
           lambda: S(noise, z, h, sig, co, step, seed, ncopy=1), lambda: S(noise, z, h, sig, co, step, seed, ncopy=3),
           lambda: S(noise, z, z, sig, co, step, seed), lambda: S(noise, z, h[:1], sig, co, step, seed),
           lambda: S(noise, z, h, sig, co[:, :3].contiguous(), step, seed),  # a 3-column table
           lambda: S(noise, z, h, sig, co[:-1], step, seed), lambda: S(noise, z, h, sig, co.double(), step, seed),
           lambda: S(noise, z, h, sig, co, step.long(), seed), lambda: S(noise, z, h, sig, co, step, seed.int()),
           lambda: S(noise, z, h, sig, co, step, seed.cpu()), lambda: S(noise, z, h, sig, co, step, seed.repeat(2)),
           lambda: S(noise, z, h, sig, co, step, None),
           lambda: S(noise, z, h, sig, co, step, seed, F_total=F_ - 1),
           lambda: S(noise, z, h, sig, co, step, seed, F_total=F_ + 1, f0=2),
           lambda: S(noise, z, h, sig, co, step, seed, F_total=F_ + 1, f0=-1),
           lambda: S(noise, z, h, sig, co, step, seed, factor=fac[:1]),
           lambda: S(noise[:210], z, h, sig, co, step, seed, ncopy=1, factor=fac),
           lambda: S(noise, z, h, sig, co, step, seed, mask=m), lambda: S(noise, z, h, sig, co, step, seed, z0=z, eps=z),
           lambda: S(noise, z, h, sig, co, step, seed, z0=z, eps=z, mask=m[:, :2]),
           lambda: NB(seed, step, shape, out=on), lambda: NN(seed, step, shape, out=ob),
           lambda: NB(seed, step, shape[:4], out=ob), lambda: NB(seed, step, (0,) + shape[1:]),
           lambda: NB(seed, step, shape, out=ob[:1]), lambda: NB(seed, step, shape, out=ob.transpose(3, 4)),
           lambda: NB(seed, step, shape, stream_id=1 << 16, out=ob), lambda: NB(seed, step, shape, stream_id=-1, out=ob),
           lambda: NB(seed, step, shape, F_total=F_ - 1, out=ob), lambda: NB(seed, step, shape, F_total=F_ + 1, f0=2, out=ob),
           lambda: NB(seed, step, shape, f0=-1, out=ob), lambda: NB(seed.int(), step, shape, out=ob),
           lambda: NB(seed.cpu(), step, shape, out=ob), lambda: NB(seed, step.long(), shape, out=ob),
           lambda: NN(seed, step, shape, stream_id=1 << 16, out=on), lambda: NN(seed, step, shape, F_total=2, out=on),
           lambda: NN(seed, step.cpu(), shape, out=on), lambda: NN(None, step, shape, out=on)]
    for i, fn in enumerate(bad):
        with pytest.raises(VstError):
            fn()
            pytest.fail(f"case {i} was accepted")
    assert not z.any() and not h.any() and not ob.any() and not on.any()
    # the C entries themselves refuse what the wrappers cannot express or check first
    from video_style_transfer_amd import _lib
    lib = _lib.load()
    p = lambda t: t.data_ptr()  # noqa: E731
    assert lib.vst_noise_bits(p(ob), p(seed), p(step), 1 << 16, B_, 4, F_, F_, 0, H_ * W_, None) == 1
    assert lib.vst_noise_normal(p(on), p(seed), p(step), 0, B_, 4, F_, F_ + 1, 2, H_ * W_, None) == 1
    assert lib.vst_noise_normal(p(on), p(seed), p(step), 0, B_, 4, F_, F_, -1, H_ * W_, None) == 1
    assert lib.vst_noise_normal(p(on), p(seed), p(step), 0, B_, (1 << 18) + 1, F_, F_, 0, H_ * W_, None) == 1
    assert lib.vst_noise_normal(p(on), p(seed), p(step), 0, B_, 4, 0, F_, 0, H_ * W_, None) == 1
    assert lib.vst_noise_normal(p(on), None, p(step), 0, B_, 4, F_, F_, 0, H_ * W_, None) == 1
    assert lib.vst_sampler_step_noise(p(noise), 2, 7.5, p(z), p(h), B_, 4, F_, F_, 1, H_ * W_, p(sig), p(co), p(step),
                                      p(seed), None, None, None, None, 0, None) == 1
    assert lib.vst_sampler_step_noise(p(noise), 2, 7.5, p(z), p(h), B_, 4, F_, F_, 0, H_ * W_, p(sig), p(co), p(step),
                                      None, None, None, None, None, 0, None) == 1
    torch.cuda.synchronize()
    assert not z.any() and not h.any() and not ob.any() and not on.any()


# ----------------------------------------------------------------------------- the loop
CASES = [("euler_a", GUIDANCE), ("dpmpp_2m_sde", GUIDANCE), ("lcm", 1.0)]  # LCM runs at guidance 1: one UNet copy
NOISE_SEED = 11


def _denoiser(tiny, cuda, sampler, guidance, use_graph=True, eta=1.0):  # noqa: F811
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser
    den = AnimateDiffDenoiser(tiny["unet"], 4, 128, 128, num_inference_steps=N_STEPS, guidance_scale=guidance,
                              device=cuda, use_graph=use_graph, scheduler=schedule(sampler), sampler=sampler, eta=eta)
    den.set_prompt_embeds(tiny["enc"][1:2], tiny["pooled"][1:2], tiny["enc"][0:1], tiny["pooled"][0:1])
    return den


def _run(den, latent_seed=3, noise_seed=NOISE_SEED, split=None):
    start = den.init_latents(latent_seed)
    den.set_noise_seed(noise_seed)
    if split:
        den.run_steps(split)
    return den.run_steps().clone(), start


@pytest.fixture(scope="module")
def runs(tiny, cuda):  # noqa: F811
    """The whole 10-step run from noise (latents seed 3, noise seed 11) on a captured step, per sampler: shared."""
    res = {}
    for sampler, guidance in CASES:
        den = _denoiser(tiny, cuda, sampler, guidance)
        out, start = _run(den)
        assert den.graph is not None and int(den.step_idx) == 0 and den.coef.shape == (N_STEPS, 4)
        assert (den.ncopy == 1) == (sampler == "lcm")
        res[sampler] = (den, out, start)
    return res


@pytest.mark.parametrize("sampler,guidance", CASES)
def test_captured_run_equals_eager(cuda, tiny, runs, sampler, guidance):  # noqa: F811
    eager = _denoiser(tiny, cuda, sampler, guidance, use_graph=False)
    out, _ = _run(eager)
    assert eager.graph is None and torch.isfinite(out).all()
    assert torch.equal(out, runs[sampler][1])


@pytest.mark.parametrize("sampler,guidance", CASES)
def test_seed_replays_on_the_same_captured_step(cuda, tiny, runs, sampler, guidance):  # noqa: F811
    den, out, _ = runs[sampler]
    g0, ptr = den.graph, den.noise_seed.data_ptr()
    assert torch.equal(_run(den)[0], out)  # the noise has no state: the same seed is the same run
    other, _ = _run(den, noise_seed=NOISE_SEED + 1)
    assert torch.isfinite(other).all() and not torch.equal(other, out)
    big, _ = _run(den, noise_seed=2 ** 64 - 3)  # the whole uint64 range
    assert int(den.noise_seed) == -3 and not torch.equal(big, out) and not torch.equal(big, other)
    a, b = den(seed=5).clone(), den(seed=5).clone()  # a call's seed is also the noise seed
    assert int(den.noise_seed) == 5 and torch.equal(a, b)
    assert den.graph is g0 and den.noise_seed.data_ptr() == ptr
    assert torch.equal(_run(den)[0], out)


@pytest.mark.parametrize("sampler,guidance", CASES)
def test_interrupted_run_equals_uninterrupted(cuda, tiny, runs, sampler, guidance):  # noqa: F811
    den, out, _ = runs[sampler]
    got, _ = _run(den, split=4)
    assert torch.equal(got, out) and int(den.step_idx) == 0


def test_eta_zero_sde_is_dpmpp_2m(cuda, tiny, runs):  # noqa: F811
    from test_sampler_gpu import _denoiser as det_denoiser
    sde = _denoiser(tiny, cuda, "dpmpp_2m_sde", GUIDANCE, eta=0.0)
    det = det_denoiser(tiny, cuda, True, sampler="dpmpp_2m")
    assert not sde.coef[:, 3].any() and torch.equal(sde.coef[:, :3], det.coef)
    out, _ = _run(sde)
    det.init_latents(3)
    assert torch.equal(out, det.run_steps())
    assert not torch.equal(out, runs["dpmpp_2m_sde"][1])


@pytest.mark.parametrize("sampler,guidance", CASES)
def test_masked_source_run_keeps_the_source(cuda, tiny, sampler, guidance):  # noqa: F811
    z0, mask = tiny["z0"], tiny["mask"]
    den = _denoiser(tiny, cuda, sampler, guidance)
    out = den(source=z0, strength=0.5, mask=mask, seed=42).clone().cpu()
    assert den.masked and den.t_start == 5 and den.graph is not None
    assert torch.isfinite(out).all()
    kept = (mask == 0).unsqueeze(1).expand_as(out)
    assert kept.any() and torch.equal(out[kept], z0[kept])
    assert not torch.equal(out[~kept], z0[~kept])


def _forward_error(tiny, cuda, sampler, guidance):  # noqa: F811
    """rel-L2 of e_hat = u + g (c - u) from ONE forward of the UNet against unet_forward on the same scaled input, at
    the middle step of the sampler's schedule: test_sampler_gpu.one_forward_error at this sampler's guidance."""
    from oracle.unet import unet_forward
    from test_parity_gpu import rel
    ts, sig, _ = tables(sampler)
    z0, enc, pooled, tids = tiny["z0"], tiny["enc"], tiny["pooled"], tiny["tids"]
    lat = z0 + sig[5] * _eps(z0.shape, 42)
    scaled = (lat / ((sig[5] ** 2 + 1) ** 0.5)).expand(2, -1, -1, -1, -1).contiguous()
    t = ts[5:6].expand(2).contiguous()
    ref = unet_forward(tiny["sd"], tiny["cfg"].to_dict(), scaled, t, enc, pooled, tids)
    out = tiny["unet"](scaled.to(cuda), t.to(cuda), enc.to(cuda),
                       added_cond_kwargs={"text_embeds": pooled.to(cuda), "time_ids": tids.to(cuda)}).sample
    ec, _ = rel(out[0] + guidance * (out[1] - out[0]), ref[0] + guidance * (ref[1] - ref[0]))
    return ec


@pytest.mark.parametrize("sampler,guidance", CASES)
def test_run_vs_restatement(cuda, K, tiny, runs, sampler, guidance):  # noqa: F811
    """The accumulated update against the fp32 restatement (CFG as two unet_forward calls per step, one at guidance
    1; the whole update by sampler_step_reference fed the device's xi of every step), gated as
    test_dpmpp_2m_run_vs_restatement is: rel-L2 <= 1.5 * W * (one forward's e_hat error), W the largest
    (|b| + |c|) / |b + c| of this sampler's own table (1 where c = 0).  Figures on an MI355X, update
    rel-L2 / one forward / W / rel-L2 over (W * one forward), which may reach 1.5: euler_a 1.09e-2 / 6.93e-2 / 1 / 0.157;
    dpmpp_2m_sde 7.65e-3 / 6.93e-2 / 2.119 / 0.052; lcm at guidance 1 1.58e-3 / 7.62e-3 / 1 / 0.207."""
    from oracle.unet import unet_forward
    from test_parity_gpu import rel
    from video_style_transfer_amd.scheduler import sampler_step_reference
    ts, sig, co = tables(sampler)
    W = float(((co[:, 1].abs() + co[:, 2].abs()) / (co[:, 1] + co[:, 2]).abs()).max())
    assert (W == 1.0) == (sampler != "dpmpp_2m_sde")
    den, out, start = runs[sampler]
    assert torch.equal(den.coef.cpu(), co)
    one = _forward_error(tiny, cuda, sampler, guidance)
    cfgd, sd, enc, pooled, tid = tiny["cfg"].to_dict(), tiny["sd"], tiny["enc"], tiny["pooled"], tiny["tids"][:1]
    seed = dev_seed(NOISE_SEED, cuda)
    lat, hist = start, torch.full_like(start, float("nan"))  # never read before it is written
    ncopy = 2 if guidance > 1 else 1
    for i in range(N_STEPS):
        scaled = lat / ((sig[i] ** 2 + 1) ** 0.5)
        rows = [_rows(unet_forward(sd, cfgd, scaled, ts[i:i + 1], enc[k:k + 1], pooled[k:k + 1], tid))
                for k in ((0, 1) if ncopy == 2 else (1,))]
        xi = K.noise_normal(seed, dev_step(i, cuda), tuple(start.shape)).cpu()
        lat, hist, _ = sampler_step_reference(torch.cat(rows), lat, hist, sig, co, i, guidance=guidance, ncopy=ncopy,
                                              xi=xi)
    assert torch.isfinite(out).all()
    eu, _ = rel(out.cpu() - start, lat - start)
    ef, _ = rel(out, lat)
    print(f"[noise] {sampler} g={guidance}: update rel_l2={eu:.3e} (latents {ef:.3e}), one forward rel_l2={one:.3e}, "
          f"W={W:.3f}, ratio={eu / (W * one):.3f}")
    assert eu <= 1.5 * W * one, (eu, W, one)
