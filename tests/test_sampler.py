"""Few-step sampling, host side: the Karras sigma table, the sampler coefficient tables, the order of
the two samplers on an analytic problem, the fp32 restatement of the step, and what is refused.  Needs the built
library but no GPU."""
import math
import types

import pytest
import torch


def _scheduler(n, schedule="karras"):
    from video_style_transfer_amd.scheduler import EulerDiscreteScheduler
    s = EulerDiscreteScheduler(sigma_schedule=schedule)
    s.set_timesteps(n)
    return s


# ----------------------------------------------------------------------------- tables
@pytest.mark.parametrize("n", [10, 20, 50])
def test_discrete_schedule_is_todays_table(n):
    from video_style_transfer_amd.scheduler import EulerDiscreteScheduler
    old = EulerDiscreteScheduler()
    old.set_timesteps(n)
    new = _scheduler(n, "discrete")
    assert torch.equal(old.timesteps, new.timesteps) and torch.equal(old.sigmas, new.sigmas)
    assert old.init_noise_sigma == new.init_noise_sigma
    with pytest.raises(ValueError):
        EulerDiscreteScheduler(sigma_schedule="exponential")


@pytest.mark.parametrize("n", [10, 20, 25, 50])
def test_karras_sigmas_and_timesteps(n):
    d, k = _scheduler(n, "discrete"), _scheduler(n)
    sig, ts = k.sigmas, k.timesteps
    assert sig.dtype == torch.float32 and ts.dtype == torch.float32
    assert sig.shape == (n + 1,) and ts.shape == (n,)
    assert float(sig[-1]) == 0.0 and bool((sig[1:] < sig[:-1]).all())
    assert float(sig[0]) == float(d.sigmas[0]) and float(sig[n - 1]) == pytest.approx(float(d.sigmas[n - 1]), rel=1e-6)
    assert bool((ts[1:] < ts[:-1]).all()) and float(ts.min()) >= 0.0 and float(ts.max()) <= 999.0
    # the end points are sigmas of the discrete table, so their timesteps are its (integer) ones
    assert float(ts[0]) == pytest.approx(float(d.timesteps[0]), abs=1e-3)
    assert float(ts[-1]) == pytest.approx(float(d.timesteps[-1]), abs=1e-3)
    # rho = 7: uniform steps in sigma^(1/7)
    r = sig[:n].double() ** (1.0 / 7.0)
    assert torch.allclose(r[1:] - r[:-1], (r[-1] - r[0]) / (n - 1) * torch.ones(n - 1, dtype=torch.float64), atol=1e-6)


def test_sigma_to_t_inverts_the_training_table():
    import numpy as np
    from video_style_transfer_amd.scheduler import sigma_to_t
    s = _scheduler(10)
    train = (((1 - s.alphas_cumprod) / s.alphas_cumprod) ** 0.5).double().numpy()
    ls = np.log(train)
    assert np.allclose(sigma_to_t(train[[0, 17, 500, 999]], ls), [0, 17, 500, 999], atol=1e-9)
    mid = math.exp(0.5 * (ls[300] + ls[301]))
    assert sigma_to_t(np.array([mid]), ls)[0] == pytest.approx(300.5, abs=1e-9)
    assert sigma_to_t(np.array([1e-6, 1e6]), ls).tolist() == [0.0, 999.0]  # outside the table: clamped


@pytest.mark.parametrize("sampler", ["euler", "dpmpp_2m"])
@pytest.mark.parametrize("first_step", [0, 3])
def test_coefficient_table_properties(sampler, first_step):
    from video_style_transfer_amd.scheduler import sampler_coefficients
    sig = _scheduler(10).sigmas
    co = sampler_coefficients(sig, sampler, first_step)
    assert co.dtype == torch.float64 and co.shape == (10, 3)
    assert torch.allclose(co.sum(1), torch.ones(10, dtype=torch.float64), atol=1e-14)  # a constant is a fixed point
    assert float(co[first_step, 2]) == 0.0 and float(co[0, 2]) == 0.0
    assert co[-1].tolist() == [0.0, 1.0, 0.0]
    if sampler == "dpmpp_2m":
        others = [i for i in range(1, 9) if i != first_step]
        assert bool((co[others, 2] < 0).all()) and bool((co[others, 1] > 0).all())  # it extrapolates past D
        # the second-order rows are k-diffusion's: denoised_d = (1 + 1/(2r)) D - D_prev / (2r), x' = a x - expm1(-h) d
        i = others[0]
        t = -sig.double().log()
        h, r = t[i + 1] - t[i], (t[i] - t[i - 1]) / (t[i + 1] - t[i])
        assert float(co[i, 1]) == pytest.approx(float(-torch.expm1(-h) * (1 + 1 / (2 * r))), rel=1e-12)
        assert float(co[i, 2]) == pytest.approx(float(torch.expm1(-h) / (2 * r)), rel=1e-12)
    else:
        assert not co[:, 2].any()


def test_euler_table_is_the_euler_step():
    from video_style_transfer_amd.scheduler import sampler_coefficients
    sig = _scheduler(10).sigmas.double()
    co = sampler_coefficients(sig, "euler")
    g = torch.Generator().manual_seed(0)
    x = torch.randn(64, generator=g, dtype=torch.float64) * 5
    e = torch.randn(64, generator=g, dtype=torch.float64)
    for i in range(10):
        D = x - sig[i] * e
        assert (co[i, 0] * x + co[i, 1] * D - (x + (sig[i + 1] - sig[i]) * e)).abs().max().item() <= 1e-12


def test_coefficient_refusals():
    from video_style_transfer_amd.scheduler import sampler_coefficients
    sig = _scheduler(10).sigmas
    for args in ((sig, "heun"), (sig, "dpmpp_2m", 10), (sig, "dpmpp_2m", -1), (sig.flip(0), "euler"),
                 (sig[:1], "euler"), (torch.tensor([1.0, 1.0, 0.0]), "euler")):
        with pytest.raises(ValueError):
            sampler_coefficients(*args)


# ----------------------------------------------------------------------------- order on an analytic problem
def _gaussian_error(s, n, sampler):
    """|x(0) - exact| for Gaussian data of std s, whose exact denoiser is D(x, sigma) = x s^2 / (s^2 + sigma^2) and whose
    probability-flow solution is x(sigma) = x(sigma_0) sqrt((s^2 + sigma^2) / (s^2 + sigma_0^2)); x(sigma_0) at one std
    of the marginal; float64 throughout, Karras sigmas."""
    from video_style_transfer_amd.scheduler import sampler_coefficients
    sig = _scheduler(n).sigmas.double()
    co = sampler_coefficients(sig, sampler)
    x = x_start = math.sqrt(s * s + float(sig[0]) ** 2)
    prev = 0.0
    for i in range(n):
        D = x * s * s / (s * s + float(sig[i]) ** 2)
        x, prev = float(co[i, 0]) * x + float(co[i, 1]) * D + float(co[i, 2]) * prev, D
    return abs(x - x_start * s / math.sqrt(s * s + float(sig[0]) ** 2))


@pytest.mark.parametrize("s", [0.5, 1.0])
def test_dpmpp_2m_at_20_steps_beats_euler_at_50(s):
    e50, d20 = _gaussian_error(s, 50, "euler"), _gaussian_error(s, 20, "dpmpp_2m")
    print(f"[sampler] s={s}: Euler 50 steps {e50:.3e}, DPM++ 2M 20 steps {d20:.3e}, ratio {e50 / d20:.2f}")
    assert d20 * 2.0 <= e50  # measured 4.5x (s = 0.5) and 3.3x (s = 1.0)


def test_order_of_the_two_samplers():
    """Halving the step divides a first-order error by about 2 and a second-order one by about 4 (s = 1.0; at s = 0.5
    the DPM++ 2M error changes sign between 40 and 50 steps, so its ratio there says nothing)."""
    d = _gaussian_error(1.0, 20, "dpmpp_2m") / _gaussian_error(1.0, 40, "dpmpp_2m")
    e = _gaussian_error(1.0, 20, "euler") / _gaussian_error(1.0, 40, "euler")
    print(f"[sampler] err(20)/err(40): DPM++ 2M {d:.2f}, Euler {e:.2f}")
    assert d >= 3.0  # measured 5.8
    assert e <= 2.5  # measured 1.92


# ----------------------------------------------------------------------------- the fp32 restatement
def _step_inputs(B=2, Cl=4, F=3, H=5, W=7, seed=0):
    g = torch.Generator().manual_seed(seed)
    shape = (B, Cl, F, H, W)
    noise = (torch.randn(2 * B * F * H * W, Cl, generator=g) * torch.tensor([1.0, 0.5, 2.0, 1.0])[:Cl]).bfloat16()
    return noise, torch.randn(shape, generator=g) * 3, torch.randn(shape, generator=g)


def test_reference_rescale_identity_and_unit():
    from video_style_transfer_amd.scheduler import rescale_factor_reference, sampler_coefficients, sampler_step_reference
    sig = _scheduler(10).sigmas
    co = sampler_coefficients(sig, "dpmpp_2m")
    noise, lat, hist = _step_inputs()
    plain = sampler_step_reference(noise, lat, hist, sig, co, 4, guidance=7.5, guidance_rescale=0.0)
    assert plain[2] is None
    assert torch.equal(rescale_factor_reference(noise, 2, 7.5, 0.0), torch.ones(2))  # phi = 0: the identity
    # phi = 1: the rescaled guided noise has the cond branch's std, clip by clip
    f = rescale_factor_reference(noise, 2, 7.5, 1.0)
    n2 = noise.float().reshape(2, 2, -1)
    e = (n2[0] + 7.5 * (n2[1] - n2[0])) * f[:, None]
    assert torch.allclose(e.std(dim=1), n2[1].std(dim=1), rtol=1e-5)
    assert bool((f < 1).all())  # guidance 7.5 inflates the std; the rescale undoes it
    # the step with phi = 1 is the plain step on the rescaled noise: D moves by sigma * (1 - f) * e
    full = sampler_step_reference(noise, lat, hist, sig, co, 4, guidance=7.5, guidance_rescale=1.0)
    assert torch.equal(full[2], f)
    e5 = (lat - plain[1]) / sig[4]
    assert torch.allclose(full[1], lat - sig[4] * e5 * f.view(2, 1, 1, 1, 1), atol=1e-4)
    # std(e) = 0 (both branches constant): factor 1, not the reference's NaN
    assert torch.equal(rescale_factor_reference(torch.ones_like(noise), 2, 7.5, 0.7), torch.ones(2))
    with pytest.raises(ValueError):
        sampler_step_reference(noise[:210], lat, hist, sig, co, 4, ncopy=1, guidance_rescale=0.5)


def test_reference_step_history_and_mask():
    from video_style_transfer_amd.scheduler import sampler_coefficients, sampler_step_reference
    sig = _scheduler(10).sigmas
    co = sampler_coefficients(sig, "dpmpp_2m")
    noise, lat, hist = _step_inputs(seed=1)
    nan = torch.full_like(hist, float("nan"))
    first = sampler_step_reference(noise, lat, nan, sig, co, 0)  # c = 0: the history is not read
    assert torch.isfinite(first[0]).all() and torch.equal(first[0], sampler_step_reference(noise, lat, hist, sig, co, 0)[0])
    assert not torch.isfinite(sampler_step_reference(noise, lat, nan, sig, co, 4)[0]).any()
    last = sampler_step_reference(noise, lat, hist, sig, co, 9)
    assert torch.equal(last[0], last[1])  # (0, 1, 0): the last step returns the denoised estimate
    z0, eps = torch.randn_like(lat), torch.randn_like(lat)
    m = (torch.rand(1, 3, 5, 7, generator=torch.Generator().manual_seed(2)) < 0.5).float()
    out, D, _ = sampler_step_reference(noise, lat, hist, sig, co, 4, z0=z0, eps=eps, mask=m)
    free = sampler_step_reference(noise, lat, hist, sig, co, 4)[0]
    kept = (m == 0).unsqueeze(1).expand_as(lat)
    assert torch.equal(out[kept], (z0 + sig[5] * eps)[kept]) and torch.equal(out[~kept], free[~kept])
    assert torch.equal(D, sampler_step_reference(noise, lat, hist, sig, co, 4)[1])  # the history is the unblended D
    one = sampler_step_reference(noise[:210], lat, hist, sig, co, 4, ncopy=1)  # no CFG: the only row is eps_hat
    assert torch.allclose(one[1], lat - sig[4] * noise[:210].float().reshape(2, 3, 5, 7, 4).permute(0, 4, 1, 2, 3))


# ----------------------------------------------------------------------------- refusals
def test_denoiser_refuses_bad_sampler_arguments():
    """Refused before the UNet or the device is touched, so no GPU is needed (and none is given: unet=None)."""
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser, check_sampler
    world2 = types.SimpleNamespace(world=2, rank=0, local_frames=lambda F: (F // 2, 0))
    world1 = types.SimpleNamespace(world=1, rank=0, local_frames=lambda F: (F, 0))
    bad = [dict(sampler="heun"), dict(sampler="dpmpp_2m_sde"), dict(sampler=None),
           dict(guidance_rescale=0.7, guidance_scale=1.0), dict(guidance_rescale=0.7, guidance_scale=0.0),
           dict(guidance_rescale=0.7, shard=world2), dict(sampler="dpmpp_2m", guidance_rescale=0.7, shard=world2),
           dict(guidance_rescale=float("nan")), dict(guidance_rescale=float("inf")), dict(guidance_rescale=-0.1),
           dict(guidance_rescale=1.5), dict(guidance_rescale="much")]
    for kw in bad:
        with pytest.raises(ValueError):
            AnimateDiffDenoiser(None, 4, 64, 64, **kw)
            pytest.fail(f"{kw} was accepted")
    assert check_sampler("dpmpp_2m", 7.5, 0.0, world2) == 0.0  # the multistep update is elementwise: shards are fine
    assert check_sampler("euler", 7.5, 0.7, world1) == 0.7
    assert check_sampler("dpmpp_2m", 1.0, 0, None) == 0.0  # no CFG, no rescale


def test_wrappers_refuse_cpu_tensors():
    from video_style_transfer_amd import _lib, kernels as K
    z = torch.zeros(1, 4, 2, 3, 3)
    noise = torch.zeros(2 * 18, 4, dtype=torch.bfloat16)
    with pytest.raises(_lib.VstError):
        K.sampler_step(noise, z, z.clone(), torch.ones(5), torch.zeros(4, 3), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(_lib.VstError):
        K.cfg_rescale_factor(noise, z.shape, guidance=7.5, phi=0.5)


def test_entries_refuse_bad_arguments_without_gpu():
    from video_style_transfer_amd import _lib
    lib = _lib.load()
    ok = dict(noise=1, ncopy=2, g=7.5, lat=8, hist=16, B=2, Cl=4, F=3, HW=35, sig=1, coef=1, step=1, factor=None,
              z0=None, eps=None, mask=None, mc=0)

    def step(**kw):
        a = dict(ok, **kw)
        return lib.vst_sampler_step(a["noise"], a["ncopy"], a["g"], a["lat"], a["hist"], a["B"], a["Cl"], a["F"],
                                    a["HW"], a["sig"], a["coef"], a["step"], a["factor"], a["z0"], a["eps"], a["mask"],
                                    a["mc"], None)
    masked = dict(z0=1, eps=1, mask=1, mc=2)
    for bad in (dict(noise=None), dict(lat=None), dict(hist=None), dict(hist=8), dict(sig=None), dict(coef=None),
                dict(step=None), dict(ncopy=0), dict(ncopy=3), dict(B=0), dict(Cl=0), dict(F=-1), dict(HW=0),
                dict(factor=1, ncopy=1), dict(z0=1), dict(eps=1), dict(z0=1, eps=1), dict(masked, z0=None),
                dict(masked, eps=None), dict(masked, mc=3), dict(masked, mc=0)):
        assert step(**bad) == 1, bad
    assert lib.vst_cfg_rescale_factor_workspace_bytes(2, 4, 3, 35) == 2 * 1 * 24
    assert lib.vst_cfg_rescale_factor_workspace_bytes(2, 4, 5, 117) == 2 * 3 * 24  # 2340 values: three blocks
    assert lib.vst_cfg_rescale_factor_workspace_bytes(0, 4, 3, 35) == 0
    okr = dict(noise=1, g=7.5, phi=0.7, B=2, Cl=4, F=3, HW=35, factor=1, ws=1)

    def rescale(**kw):
        a = dict(okr, **kw)
        return lib.vst_cfg_rescale_factor(a["noise"], a["g"], a["phi"], a["B"], a["Cl"], a["F"], a["HW"], a["factor"],
                                          a["ws"], None)
    for bad in (dict(noise=None), dict(factor=None), dict(ws=None), dict(B=0), dict(Cl=0), dict(F=0), dict(HW=-3),
                dict(phi=float("nan")), dict(phi=-0.5), dict(phi=1.5), dict(B=70000)):
        assert rescale(**bad) == 1, bad
