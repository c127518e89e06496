"""Video-to-video on the GPU: the source-clip kernels against torch fp32 on the CPU inside poisoned
guard bands, the three exact identities of the keep mask, and the denoiser entered part-way from a source clip
(against an fp32 restatement of the definitions on top of oracle.unet.unet_forward; graph replay against eager)."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
GUARD = 64  # elements of poison on either side of every buffer


@pytest.fixture(scope="module")
def K(cuda):
    from video_style_transfer_amd import kernels
    return kernels


def _poison(dtype):
    return float("nan") if dtype.is_floating_point else 0x5A


def guarded(t, dev):
    """(whole buffer, view holding t): t copied into the middle of a buffer whose two ends are poison."""
    buf = torch.full((t.numel() + 2 * GUARD,), _poison(t.dtype), dtype=t.dtype, device=dev)
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def guards_intact(buf, n):
    """Both bands of a guarded buffer of n payload elements still hold the poison, bit for bit."""
    fresh = torch.full((GUARD,), _poison(buf.dtype), dtype=buf.dtype, device=buf.device)
    return same_bytes(buf[:GUARD], fresh) and same_bytes(buf[GUARD + n:], fresh)


def sigma_table(n=10):
    from video_style_transfer_amd.scheduler import EulerDiscreteScheduler
    s = EulerDiscreteScheduler()
    s.set_timesteps(n)
    return s.sigmas.float()


def close_ulp(out, ref, name):
    """A few fp32 ulp: the device may contract a * b + c into one FMA where the CPU rounds twice."""
    err = (out - ref).abs().max().item()
    print(f"[source] {name}: max|err|={err:.3e} max|ref|={ref.abs().max().item():.3e}")
    assert torch.isfinite(out).all(), name
    torch.testing.assert_close(out, ref, rtol=2e-6, atol=2e-6 * ref.abs().max().item(), msg=lambda m: f"{name}: {m}")


# ----------------------------------------------------------------------------- kernels
B_, F_, H_, W_ = 2, 3, 5, 7  # HW = 35: no multiple of any vector width; B*F*HW = 210 pixels: one partial block


@pytest.mark.parametrize("Cl", [4, 5])
def test_noise_latents_vs_torch(cuda, K, Cl):
    g = torch.Generator().manual_seed(10 + Cl)
    sig = sigma_table(10)
    z0 = torch.randn(B_, Cl, F_, H_, W_, generator=g)
    eps = torch.randn(B_, Cl, F_, H_, W_, generator=g)
    n = z0.numel()
    zb, zd = guarded(z0, cuda)
    eb, ed = guarded(eps, cuda)
    sb, sd_ = guarded(sig, cuda)
    for s in (0, 5, 9):
        stb, step = guarded(torch.tensor([s], dtype=torch.int32), cuda)
        ob, out = guarded(torch.zeros_like(z0), cuda)
        before = [b.clone() for b in (zb, eb, sb, stb)]
        r = K.noise_latents(zd, ed, sd_, step, out=out)
        assert r is out
        close_ulp(out.cpu(), z0 + sig[s] * eps, f"noise_latents Cl={Cl} step={s}")
        assert guards_intact(ob, n)
        assert all(same_bytes(a, b) for a, b in zip(before, (zb, eb, sb, stb))), "an input changed"
    fresh = K.noise_latents(zd, ed, sd_, step)  # allocating form
    assert torch.equal(fresh, out)


def _masks(kind, mc, g):
    shape = (mc, F_, H_, W_)
    if kind == "zeros":
        return torch.zeros(shape)
    if kind == "ones":
        return torch.ones(shape)
    if kind == "binary":
        return (torch.rand(shape, generator=g) < 0.5).float()
    return torch.rand(shape, generator=g)


def _ref_masked(noise, ncopy, guidance, lat, sig, s, z0, eps, m):
    """The definition, fp32 on the CPU.  noise rows ((k*B + b)*F + f)*HW + p, Cl channels."""
    B, Cl, F, H, W = lat.shape
    n5 = noise.float().view(ncopy, B, F, H, W, Cl).permute(0, 1, 5, 2, 3, 4)
    e = n5[0] + guidance * (n5[1] - n5[0]) if ncopy == 2 else n5[0]
    new = lat + (sig[s + 1] - sig[s]) * e
    mm = m.unsqueeze(1)  # broadcast over channels (and over clips when mask_clips == 1)
    return mm * new + (1 - mm) * (z0 + sig[s + 1] * eps), new


@pytest.mark.parametrize("ncopy", [1, 2])
@pytest.mark.parametrize("Cl", [4, 5])
def test_euler_cfg_step_masked_vs_torch(cuda, K, Cl, ncopy):
    g = torch.Generator().manual_seed(100 + 10 * Cl + ncopy)
    N = 10
    sig = sigma_table(N)
    shape = (B_, Cl, F_, H_, W_)
    z0 = torch.randn(shape, generator=g)
    eps = torch.randn(shape, generator=g)
    noise = torch.randn(ncopy * B_ * F_ * H_ * W_, Cl, generator=g).to(BF)
    n = z0.numel()
    zb, zd = guarded(z0, cuda)
    eb, ed = guarded(eps, cuda)
    nb, nd = guarded(noise, cuda)
    sb, sd_ = guarded(sig, cuda)
    for s in (0, 4, N - 1):
        lat = z0 + sig[s] * eps + 0.1 * torch.randn(shape, generator=g)  # latents as a run holds them at step s
        stb, step = guarded(torch.tensor([s], dtype=torch.int32), cuda)
        # the plain step against the definition on its own: it shares the masked step's code, so identity 1 below
        # does not test it independently
        pb, plain = guarded(lat, cuda)
        before = [b.clone() for b in (nb, sb, stb)]
        K.euler_cfg_step(nd, plain, sd_, step, guidance=7.5, ncopy=ncopy)
        name = f"plain Euler Cl={Cl} ncopy={ncopy} step={s}"
        close_ulp(plain.cpu(), _ref_masked(noise, ncopy, 7.5, lat, sig, s, z0, eps, torch.ones(1, F_, H_, W_))[1], name)
        assert guards_intact(pb, n), name
        assert all(same_bytes(a, b) for a, b in zip(before, (nb, sb, stb))), name + ": input changed"
        for kind in ("zeros", "ones", "binary", "uniform"):
            for mc in (1, B_):
                m = _masks(kind, mc, g)
                mb, md = guarded(m, cuda)
                lb, ld = guarded(lat, cuda)
                before = [b.clone() for b in (zb, eb, nb, sb, stb, mb)]
                K.euler_cfg_step_masked(nd, ld, sd_, step, zd, ed, md, guidance=7.5, ncopy=ncopy)
                out = ld.cpu()
                name = f"masked Euler Cl={Cl} ncopy={ncopy} step={s} mask={kind} mask_clips={mc}"
                ref, _ = _ref_masked(noise, ncopy, 7.5, lat, sig, s, z0, eps, m)
                close_ulp(out, ref, name)
                assert guards_intact(lb, n), name
                assert all(same_bytes(a, b) for a, b in zip(before, (zb, eb, nb, sb, stb, mb))), name + ": input changed"
                free = (m == 1).unsqueeze(1).expand(shape)
                kept = (m == 0).unsqueeze(1).expand(shape)
                # identity 1: where m == 1 the masked step stores the plain step's bits
                assert torch.equal(out[free], plain.cpu()[free]), name
                if kind == "ones":
                    assert torch.equal(ld, plain), name
                # identity 2: after the last step (sigma = 0) kept pixels are the source, bit for bit
                if s == N - 1:
                    assert torch.equal(out[kept], z0[kept]), name
                    if kind == "zeros":
                        assert torch.equal(out, z0), name


@pytest.mark.parametrize("ncopy", [1, 2])
@pytest.mark.parametrize("entry", ["euler", "euler_masked", "sampler", "sampler_masked"])
def test_misaligned_noise_stores_the_aligned_bytes(cuda, K, entry, ncopy):
    """Cl = 4 with noise rows 2 bytes off an 8-byte boundary: the row loads must not assume the alignment, and every
    entry point stores the bytes it stores on aligned noise.  m is fractional: the blend of the masked Euler step is
    contractible and rounds differently in the 4-channel and the per-channel instance (one ulp), so equal bytes need
    the 4-channel arithmetic on both sides, whatever the loads."""
    from video_style_transfer_amd.scheduler import sampler_coefficients
    g = torch.Generator().manual_seed(300 + ncopy)
    sig = sigma_table(10)
    coef = sampler_coefficients(sig, "dpmpp_2m").float().to(cuda)
    shape = (B_, 4, F_, H_, W_)
    lat, hist, z0, eps = (torch.randn(shape, generator=g).to(cuda) for _ in range(4))
    m = torch.rand(B_, F_, H_, W_, generator=g).to(cuda)
    noise = torch.randn(ncopy * B_ * F_ * H_ * W_, 4, generator=g).to(BF)
    aligned = noise.to(cuda)
    shifted = torch.empty(noise.numel() + 1, dtype=BF, device=cuda)[1:].view(noise.shape)
    shifted.copy_(noise)
    assert aligned.data_ptr() % 8 == 0 and shifted.data_ptr() % 8 == 2 and shifted.is_contiguous()
    sd_, step = sig.to(cuda), torch.tensor([4], dtype=torch.int32, device=cuda)  # a second-order row: hist is read
    assert float(coef[4, 2]) != 0.0
    kw = dict(guidance=7.5, ncopy=ncopy)
    fn = {"euler": lambda nz, x, h: K.euler_cfg_step(nz, x, sd_, step, **kw),
          "euler_masked": lambda nz, x, h: K.euler_cfg_step_masked(nz, x, sd_, step, z0, eps, m, **kw),
          "sampler": lambda nz, x, h: K.sampler_step(nz, x, h, sd_, coef, step, **kw),
          "sampler_masked": lambda nz, x, h: K.sampler_step(nz, x, h, sd_, coef, step, z0=z0, eps=eps, mask=m, **kw)}[entry]
    outs = []
    for nz in (aligned, shifted):
        x, h = lat.clone(), hist.clone()
        fn(nz, x, h)
        outs.append((x, h))
    (xa, ha), (xs, hs) = outs
    differ = (xa != xs).sum().item()
    print(f"[source] {entry} ncopy={ncopy}, noise 2 bytes off: {differ} of {xa.numel()} latents differ, "
          f"max|diff|={(xa - xs).abs().max().item():.3e} at max|lat|={xa.abs().max().item():.3e}")
    assert torch.isfinite(xa).all() and not torch.equal(xa, lat)
    assert same_bytes(xa, xs) and same_bytes(ha, hs)
    assert same_bytes(shifted, aligned)


def test_source_wrappers_refuse_bad_arguments(cuda, K):
    from video_style_transfer_amd._lib import VstError
    sig = sigma_table(10).to(cuda)
    step = torch.zeros(1, dtype=torch.int32, device=cuda)
    z = torch.zeros(B_, 4, F_, H_, W_, device=cuda)
    noise = torch.zeros(2 * B_ * F_ * H_ * W_, 4, dtype=BF, device=cuda)
    m = torch.ones(1, F_, H_, W_, device=cuda)
    bad = [lambda: K.noise_latents(z.double(), z, sig, step), lambda: K.noise_latents(z, z[:1], sig, step),
           lambda: K.noise_latents(z, z.transpose(3, 4), sig, step),
           lambda: K.noise_latents(z, z, sig, step.long()), lambda: K.noise_latents(z, z, sig, step, out=z[:1]),
           lambda: K.noise_latents(z, z, sig.double(), step),
           lambda: K.euler_cfg_step_masked(noise.float(), z, sig, step, z, z, m),
           lambda: K.euler_cfg_step_masked(noise[:-1], z, sig, step, z, z, m),
           lambda: K.euler_cfg_step_masked(noise, z, sig, step, z, z, m, ncopy=1),
           lambda: K.euler_cfg_step_masked(noise, z, sig, step, z[:1], z, m),
           lambda: K.euler_cfg_step_masked(noise, z, sig, step, z, z.half(), m),
           lambda: K.euler_cfg_step_masked(noise, z, sig, step, z, z, m[:, :2]),
           lambda: K.euler_cfg_step_masked(noise, z, sig, step, z, z, torch.ones(3, F_, H_, W_, device=cuda)),
           lambda: K.euler_cfg_step_masked(noise, z, sig, step, z, z, m.transpose(2, 3)),
           lambda: K.euler_cfg_step_masked(noise, z[0], sig, step, z[0], z[0], m),
           lambda: K.euler_cfg_step(noise.float(), z, sig, step),
           lambda: K.euler_cfg_step(noise[:-1], z, sig, step),
           lambda: K.euler_cfg_step(noise, z.transpose(3, 4), sig, step),
           lambda: K.euler_cfg_step(noise, z, sig, step.long()),
           lambda: K.euler_cfg_step(noise.cpu(), z, sig, step),
           lambda: K.euler_cfg_step(noise, z.cpu(), sig, step),
           lambda: K.u8_to_frames(torch.zeros(1, 4, 4, 3, device=cuda)),
           lambda: K.u8_to_frames(torch.zeros(4, 4, 3, dtype=torch.uint8, device=cuda)),
           lambda: K.u8_to_frames(torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device=cuda), ldd=2),
           lambda: K.u8_to_frames(torch.zeros(1, 4, 4, 6, dtype=torch.uint8, device=cuda)[..., :3])]
    for i, fn in enumerate(bad):
        with pytest.raises(VstError):
            fn()
            pytest.fail(f"case {i} was accepted")
    assert not z.any()


@pytest.mark.parametrize("ldd", [3, 8])
def test_u8_to_frames_all_values(cuda, K, ldd):
    """Every uint8 value in every channel: the bf16 torch gives for ((v.float() / 255 - 0.5) / 0.5).bfloat16()."""
    v = torch.arange(256, dtype=torch.uint8)
    x = torch.stack([v, v.flip(0), v.roll(85)], -1).reshape(2, 8, 16, 3)  # (n, H, W, C), HW = 128
    xb, xd = guarded(x, cuda)
    keep = xb.clone()
    out = K.u8_to_frames(xd, ldd)
    assert out.shape == (256, ldd) and out.dtype == BF
    ref = torch.zeros(256, ldd, dtype=BF)
    ref[:, :3] = ((x.reshape(256, 3).float() / 255 - 0.5) / 0.5).bfloat16()
    assert torch.equal(out.cpu(), ref)
    assert same_bytes(xb, keep)
    # the inverse boundary: frames_to_u8 of these rows gives the frames back wherever bf16 holds the value's bin
    back = K.frames_to_u8(out, 2, 3, 8, 16)
    assert (back.cpu().int() - x.int()).abs().max() <= 1


def test_encode_frames_equals_encode_of_normalised(cuda):
    from test_vae_gpu import _setup as vae_setup
    cfg, sd, vae = vae_setup("tiny", 3)
    g = torch.Generator().manual_seed(4)
    u8 = torch.randint(0, 256, (2, 64, 64, 3), generator=g, dtype=torch.uint8)
    x = ((u8.float() / 255 - 0.5) / 0.5).permute(0, 3, 1, 2).contiguous()
    want = vae.encode(x.to(cuda)).latent_dist.mode(cfg.scaling_factor)  # (n, 4, h, w)
    got = vae.encode_frames(u8.to(cuda))  # (1, 4, n, h, w)
    hh = 64 // 2 ** (len(cfg.block_out_channels) - 1)
    assert got.dtype == torch.float32 and got.shape == (1, 4, 2, hh, hh) and got.is_contiguous()
    assert torch.isfinite(got).all()
    assert torch.equal(got[0].permute(1, 0, 2, 3), want)
    two = vae.encode_frames(u8.to(cuda).unsqueeze(1))  # (clips = 2, F = 1, ...)
    assert torch.equal(two[:, :, 0], want)
    # with a generator: a sample, around the mode, reproducible from the generator's state
    gd = torch.Generator(device=cuda).manual_seed(5)
    s1 = vae.encode_frames(u8.to(cuda), generator=gd)
    gd.manual_seed(5)
    s2 = vae.encode_frames(u8.to(cuda), generator=gd)
    assert torch.equal(s1, s2) and not torch.equal(s1, got) and torch.isfinite(s1).all()
    from video_style_transfer_amd._lib import VstError
    with pytest.raises(VstError):
        vae.encode_frames(u8)  # CPU
    with pytest.raises(VstError):
        vae.encode_frames(u8.to(cuda).float())


# ----------------------------------------------------------------------------- the loop
N_STEPS, GUIDANCE = 10, 7.5


@pytest.fixture(scope="module")
def tiny(cuda):
    from test_parity_gpu import _setup
    from video_style_transfer_amd.utils import build_unet
    cfg, sd, lat, enc, pooled, tids = _setup("tiny", 4, 16, seed=5, B=2)
    unet = build_unet(cfg, state_dict=sd, device=cuda)
    g = torch.Generator().manual_seed(77)
    z0 = torch.randn(1, 4, 4, 16, 16, generator=g)
    mask = (torch.rand(1, 4, 16, 16, generator=g) < 0.5).float()
    mask2 = torch.rand(1, 4, 16, 16, generator=g)
    return dict(cfg=cfg, sd=sd, enc=enc, pooled=pooled, tids=tids, unet=unet, z0=z0, mask=mask, mask2=mask2)


def _denoiser(tiny, cuda, use_graph=True, frames=4, **kw):
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser
    den = AnimateDiffDenoiser(tiny["unet"], frames, 128, 128, num_inference_steps=N_STEPS, guidance_scale=GUIDANCE,
                              device=cuda, use_graph=use_graph, **kw)
    den.set_prompt_embeds(tiny["enc"][1:2], tiny["pooled"][1:2], tiny["enc"][0:1], tiny["pooled"][0:1])
    return den


def _eps(shape, seed):
    return torch.randn(shape, generator=torch.Generator(device="cpu").manual_seed(seed))


def _restated_run(tiny, z0, eps, t_start, mask=None):
    """The definitions of DESIGN.md §13 in fp32 on the CPU: start latents, Euler steps t_start .. N-1 with CFG as two
    UNet calls, the keep-mask blend after every update.  Returns (final latents, latents entering step t_start)."""
    from oracle.unet import euler_schedule, unet_forward
    ts, sig, _ = euler_schedule(N_STEPS)
    cfgd, sd, enc, pooled, tid = tiny["cfg"].to_dict(), tiny["sd"], tiny["enc"], tiny["pooled"], tiny["tids"][:1]
    lat = z0 + sig[t_start] * eps
    start = lat.clone()
    for i in range(t_start, N_STEPS):
        scaled = lat / ((sig[i] ** 2 + 1) ** 0.5)
        nu = unet_forward(sd, cfgd, scaled, ts[i:i + 1], enc[0:1], pooled[0:1], tid)
        nc = unet_forward(sd, cfgd, scaled, ts[i:i + 1], enc[1:2], pooled[1:2], tid)
        lat = lat + (sig[i + 1] - sig[i]) * (nu + GUIDANCE * (nc - nu))
        if mask is not None:
            m = mask.unsqueeze(1)
            lat = m * lat + (1 - m) * (z0 + sig[i + 1] * eps)
    return lat, start


@pytest.fixture(scope="module")
def one_forward_error(tiny, cuda):
    """rel-L2 of ONE forward of the loop against unet_forward on the same scaled input (the latents entering step 7
    of the strength-0.3 run).  One forward of the loop is the CFG pair batched as B = 2, and what a step adds to the
    latents is ds * e_hat with e_hat = u + g (c - u): the accumulated update is a sum of such terms, so the error
    that bounds it is e_hat's, HIP against fp32, not the per-branch one.  At g = 7.5 the two differ by CFG's
    amplification (c - u is small against u, its error is not): both are printed, the gate uses e_hat's."""
    from oracle.unet import euler_schedule, unet_forward
    from test_parity_gpu import rel
    ts, sig, _ = euler_schedule(N_STEPS)
    z0, enc, pooled, tids = tiny["z0"], tiny["enc"], tiny["pooled"], tiny["tids"]
    lat = z0 + sig[7] * _eps(z0.shape, 42)
    scaled = (lat / ((sig[7] ** 2 + 1) ** 0.5)).expand(2, -1, -1, -1, -1).contiguous()
    t = ts[7:8].expand(2).contiguous()
    ref = unet_forward(tiny["sd"], tiny["cfg"].to_dict(), scaled, t, enc, pooled, tids)
    out = tiny["unet"](scaled.to(cuda), t.to(cuda), enc.to(cuda),
                       added_cond_kwargs={"text_embeds": pooled.to(cuda), "time_ids": tids.to(cuda)}).sample
    e2, _ = rel(out, ref)
    ec, _ = rel(out[0] + GUIDANCE * (out[1] - out[0]), ref[0] + GUIDANCE * (ref[1] - ref[0]))
    print(f"[source] one forward at step 7: e_hat rel_l2={ec:.3e} (UNet output, both branches: {e2:.3e})")
    return ec


@pytest.fixture(scope="module")
def strength03(tiny, cuda):
    """The strength-0.3 runs (steps 7-9) shared by the tests below: HIP (graph) and the fp32 restatement, each
    without and with the binary mask."""
    z0, mask = tiny["z0"], tiny["mask"]
    eps = _eps(z0.shape, 42)
    res = {}
    for key, m in (("plain", None), ("masked", mask)):
        den = _denoiser(tiny, cuda)
        out = den(source=z0, strength=0.3, mask=m, seed=42).cpu()
        assert den.t_start == 7 and den.graph is not None
        ref, start = _restated_run(tiny, z0, eps, 7, m)
        res[key] = (out, ref, start)
    return res


@pytest.mark.parametrize("key", ["plain", "masked"])
def test_source_run_vs_restatement(cuda, tiny, strength03, one_forward_error, key):
    """Figures on an MI355X: one forward's e_hat rel_l2 6.8e-2 (UNet output 7.5e-3); update rel_l2
    4.5e-2 without the mask (0.67x one forward, against the 1.5x allowed) and 6.8e-3 with it (0.10x)."""
    from test_parity_gpu import assert_close, rel
    out, ref, start = strength03[key]
    assert_close(out, ref, 1e-2, 5e-2, name=f"source run strength 0.3 ({key})")
    # z0 dominates the latents; the accumulated update is gated on its own, against the error of one forward
    eu, _ = rel(out - start, ref - start)
    print(f"[source] {key}: update rel_l2={eu:.3e}, one forward rel_l2={one_forward_error:.3e}, "
          f"ratio={eu / one_forward_error:.2f}")
    assert eu <= 1.5 * one_forward_error, (eu, one_forward_error)
    if key == "masked":
        kept = (tiny["mask"] == 0).unsqueeze(1).expand_as(out)
        assert torch.equal(out[kept], tiny["z0"][kept])  # identity 2 through the whole loop


def test_mask_changes_free_pixels_next_to_kept_ones(tiny, strength03):
    out_p, out_m = strength03["plain"][0], strength03["masked"][0]
    assert torch.isfinite(out_m).all()
    m = tiny["mask"]
    near_kept = torch.nn.functional.max_pool2d(1 - m, 3, 1, 1) > 0  # a kept pixel in the 3x3 neighbourhood
    border = ((m == 1) & near_kept).unsqueeze(1).expand_as(out_m)
    assert border.any()
    differ = (out_m != out_p)[border].float().mean().item()
    print(f"[source] free pixels bordering kept ones that differ from the unmasked run: {differ:.3f}")
    assert differ > 0.5


def test_all_ones_mask_is_the_unmasked_run(cuda, tiny, strength03):
    den = _denoiser(tiny, cuda)
    out = den(source=tiny["z0"], strength=0.3, mask=torch.ones(1, 4, 16, 16), seed=42)
    assert den.masked
    assert torch.equal(out.cpu(), strength03["plain"][0])


def test_strength_one_is_a_plain_run_from_noised_source(cuda, tiny, K):
    z0 = tiny["z0"]
    den = _denoiser(tiny, cuda)
    out = den(source=z0, strength=1.0, seed=9).clone()
    assert den.t_start == 0
    ref = _denoiser(tiny, cuda)
    step0 = torch.zeros(1, dtype=torch.int32, device=cuda)
    ref.set_latents(K.noise_latents(z0.to(cuda), _eps(z0.shape, 9).to(cuda), ref.sigmas, step0))
    assert torch.equal(out, ref.run_steps())


def test_graph_equals_eager_and_survives_new_source(cuda, tiny, strength03):
    z0, mask, mask2 = tiny["z0"], tiny["mask"], tiny["mask2"]
    dg, de = _denoiser(tiny, cuda, True), _denoiser(tiny, cuda, False)
    og = dg(source=z0, strength=0.3, mask=mask, seed=42).clone()
    oe = de(source=z0, strength=0.3, mask=mask, seed=42).clone()
    assert de.graph is None and dg.graph is not None
    assert torch.equal(og, oe) and torch.equal(og.cpu(), strength03["masked"][0])
    # another strength, source and mask values on the same buffers: the same graph object, still eager's bits
    g0, ptrs = dg.graph, (dg.src.data_ptr(), dg.eps.data_ptr(), dg.mask.data_ptr(), dg.lat.data_ptr())
    z1 = z0.flip(2) * 0.5
    og = dg(source=z1, strength=0.5, mask=mask2, seed=7).clone()
    oe = de(source=z1, strength=0.5, mask=mask2, seed=7).clone()
    assert dg.graph is g0 and dg.t_start == 5
    assert ptrs == (dg.src.data_ptr(), dg.eps.data_ptr(), dg.mask.data_ptr(), dg.lat.data_ptr())
    assert torch.equal(og, oe) and not torch.equal(og.cpu(), strength03["masked"][0])
    # removing the mask changes the Euler kernel: the captured step is dropped
    dg.set_source(z0, 0.3, seed=42)
    assert dg.graph is None and not dg.masked
    assert torch.equal(dg.run_steps().cpu(), strength03["plain"][0])
    dg.set_source(z0, 0.3, mask, seed=42)  # and adding one again
    assert dg.graph is None and dg.masked
    # after source runs a plain run is the plain run of a fresh denoiser
    plain = dg(seed=3).clone()
    assert dg.t_start == 0 and not dg.masked
    fresh = _denoiser(tiny, cuda)
    assert torch.equal(plain, fresh(seed=3))


def test_set_source_refusals_leave_state_alone(cuda, tiny):
    z0, mask = tiny["z0"], tiny["mask"]
    den = _denoiser(tiny, cuda)
    den.set_source(z0, 0.5, mask, seed=1)
    state = (den.lat.clone(), den.src.clone(), den.eps.clone(), den.mask.clone(), den.step_idx.clone(), den.t_start)
    for args in ((z0, 0.01), (z0, 1.5), (z0, float("nan")), (z0[:, :3], 0.5), (z0[:, :, :3], 0.5),
                 (z0[..., :8], 0.5), (z0, 0.5, mask * 1.5), (z0, 0.5, mask - 0.5), (z0, 0.5, mask * float("nan")),
                 (z0, 0.5, mask[:, :2]), (z0, 0.5, mask[..., :8]), (z0, 0.5, mask[0])):
        with pytest.raises(ValueError):
            den.set_source(*args)
    with pytest.raises(ValueError):
        den(strength=0.5)
    with pytest.raises(ValueError):
        den(source=z0)
    now = (den.lat, den.src, den.eps, den.mask, den.step_idx)
    assert all(torch.equal(a, b) for a, b in zip(state, now)) and den.t_start == state[5] and den.masked


def test_run_steps_default_and_capture_keep_the_start(cuda, tiny):
    """capture() puts the step counter back where set_source left it; run_steps() then runs num_steps - t_start."""
    den = _denoiser(tiny, cuda)
    den.set_source(tiny["z0"], 0.3, tiny["mask"], seed=42)
    den.capture()
    assert int(den.step_idx) == 7
    den.run_steps()
    assert int(den.step_idx) == 0  # wrapped after step 9


def test_source_graph_equals_eager_cross_frame(cuda, tiny):
    outs = []
    for use_graph in (True, False):
        den = _denoiser(tiny, cuda, use_graph, cross_frame=("first",))
        outs.append(den(source=tiny["z0"], strength=0.3, mask=tiny["mask"], seed=42).clone())
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


def test_source_graph_equals_eager_long_clip(cuda):
    from test_parity_gpu import _setup
    from video_style_transfer_amd.utils import build_unet
    cfg, sd, lat, enc, pooled, tids = _setup("tiny", 20, 16)
    t20 = dict(unet=build_unet(cfg, state_dict=sd, device=cuda), enc=enc, pooled=pooled)
    g = torch.Generator().manual_seed(78)
    z0 = torch.randn(1, 4, 20, 16, 16, generator=g)
    mask = (torch.rand(1, 20, 16, 16, generator=g) < 0.5).float()
    outs = []
    for use_graph in (True, False):
        den = _denoiser(t20, cuda, use_graph, frames=20, context_length=16, context_stride=4)
        outs.append(den(source=z0, strength=0.2, mask=mask, seed=42).clone())
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


def test_shard_slicing_of_source_buffers(cuda, tiny):
    """A rank holding the second half of the clip fills src / eps / mask / lat with the second half of the whole
    clip's (no step is run: everything set_source adds is per element)."""
    g = torch.Generator().manual_seed(79)
    z0 = torch.randn(2, 4, 4, 16, 16, generator=g)
    mask = torch.rand(2, 4, 16, 16, generator=g)
    whole = _denoiser(tiny, cuda, False, num_clips=2)
    whole.set_source(z0, 0.5, mask, seed=11)
    stub = types.SimpleNamespace(world=1, rank=0, local_frames=lambda F: (F // 2, F // 2))
    for src_in, mask_in in ((z0, mask), (z0[:, :, 2:], mask[:, 2:]), (z0, mask[:1])):
        half = _denoiser(tiny, cuda, False, num_clips=2, shard=stub)
        assert (half.F, half.f0) == (2, 2)
        half.set_source(src_in, 0.5, mask_in, seed=11)
        assert half.t_start == 5 and int(half.step_idx) == 5
        want_mask = whole.mask[:, 2:] if mask_in.shape[0] == 2 else whole.mask[:1, 2:].expand(2, -1, -1, -1)
        assert torch.equal(half.src, whole.src[:, :, 2:]) and torch.equal(half.eps, whole.eps[:, :, 2:])
        assert torch.equal(half.mask, want_mask) and torch.equal(half.lat, whole.lat[:, :, 2:])
