"""Stochastic samplers on the host: the Philox restatement against the Random123 known answers, the
(a, b, c, d) tables of Euler ancestral, DPM-Solver++ 2M SDE and LCM, the LCM timestep spacing, the refusals, and the
exports of the built library."""
import math

import numpy as np
import pytest
import torch

from video_style_transfer_amd.scheduler import (SAMPLERS, STOCHASTIC_SAMPLERS, EulerDiscreteScheduler, noise_reference,
                                                philox4x32, sampler_coefficients, sampler_step_reference)

N_STEPS = 10


def karras(n=N_STEPS):
    s = EulerDiscreteScheduler(sigma_schedule="karras")
    s.set_timesteps(n)
    return s


def lcm(n):
    s = EulerDiscreteScheduler(timestep_spacing="lcm")
    s.set_timesteps(n)
    return s


KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
        "d16cfe09 94fdcceb 5001e420 24126ea1")]


def test_philox_known_answers():
    for counter, key, want in KAT:
        got = philox4x32(counter, key)
        assert got.dtype == np.uint32 and " ".join(f"{int(v):08x}" for v in got) == want
    # batched: the three vectors in one call
    got = philox4x32(np.array([c for c, _, _ in KAT]), np.array([k for _, k, _ in KAT]))
    assert [" ".join(f"{int(v):08x}" for v in row) for row in got] == [w for _, _, w in KAT]


def test_noise_reference_layout():
    """Element (b, c, f, p) is word c & 3 of the call at (P, step, stream << 16 | c >> 2), and a frame window of a
    clip is the slice of the whole clip."""
    seed, step, stream = 2 ** 40 + 5, 7, 3
    B, Cl, F, H, W = 2, 9, 5, 3, 4
    bits, normal = noise_reference(seed, step, stream, (B, Cl, F, H, W))
    assert bits.dtype == torch.uint32 and normal.dtype == torch.float64 and bits.shape == normal.shape == (B, Cl, F, H, W)
    for b, c, f, p in ((0, 0, 0, 0), (1, 8, 4, 11), (1, 5, 2, 7), (0, 3, 1, 1)):
        P = (b * F + f) * H * W + p
        x = philox4x32((P & 0xFFFFFFFF, P >> 32, step, stream << 16 | c >> 2), (seed & 0xFFFFFFFF, seed >> 32))
        assert int(bits[b, c, f].reshape(-1)[p]) == int(x[c & 3])
        u = [((int(v) >> 9) + 0.5) * 2.0 ** -23 for v in x]
        j = c & 2
        r = math.sqrt(-2.0 * math.log(u[j]))
        want = r * (math.sin if c & 1 else math.cos)(2.0 * math.pi * u[j + 1])
        assert abs(float(normal[b, c, f].reshape(-1)[p]) - want) <= 1e-12
    part, npart = noise_reference(seed, step, stream, (B, Cl, 3, H, W), F_total=5, f0=2)
    assert torch.equal(part, bits[:, :, 2:5]) and torch.equal(npart, normal[:, :, 2:5])
    assert not torch.equal(noise_reference(seed, step + 1, stream, (B, Cl, F, H, W))[0], bits)
    assert not torch.equal(noise_reference(seed + 1, step, stream, (B, Cl, F, H, W))[0], bits)
    assert not torch.equal(noise_reference(seed, step, 0, (B, Cl, F, H, W))[0], bits)
    for bad in (dict(stream_id=1 << 16), dict(stream_id=-1), dict(f0=3), dict(f0=-1)):
        kw = dict(seed=1, step=0, stream_id=0, shape=(1, 4, 3, 2, 2), F_total=5, f0=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            noise_reference(**kw)


@pytest.mark.parametrize("name,det", [("euler_a", "euler"), ("dpmpp_2m_sde", "dpmpp_2m")])
def test_eta_zero_is_the_deterministic_table(name, det):
    sig = karras().sigmas
    for first in (0, 4):
        t = sampler_coefficients(sig, name, first, eta=0.0)
        assert t.shape == (N_STEPS, 4) and t.dtype == torch.float64
        assert float((t[:, :3] - sampler_coefficients(sig, det, first)).abs().max()) <= 1e-12
        assert not t[:, 3].any()


@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0, 2.5])
@pytest.mark.parametrize("name", ["euler_a", "dpmpp_2m_sde"])
def test_table_identities(name, eta):
    """a + b + c = 1 (a denoised estimate equal to x is a fixed point) and (a s)^2 + d^2 = s'^2 (the noise level of
    x' is the next sigma), to 1e-12 in fp64."""
    sig = karras().sigmas.double()
    t = sampler_coefficients(sig, name, 0, eta=eta)
    assert float((t[:, :3].sum(1) - 1).abs().max()) <= 1e-12
    assert float(((t[:, 0] * sig[:-1]) ** 2 + t[:, 3] ** 2 - sig[1:] ** 2).abs().max()) <= 1e-12
    assert torch.equal(t[-1], torch.tensor([0.0, 1.0, 0.0, 0.0], dtype=torch.float64))
    assert bool((t[:-1, 3] > 0).all()) == (eta > 0)


def test_first_order_rows():
    sig = karras().sigmas
    for first in (0, 3, N_STEPS - 2):
        t = sampler_coefficients(sig, "dpmpp_2m_sde", first)
        second = [i for i in range(N_STEPS) if float(t[i, 2]) != 0.0]
        assert second == [i for i in range(1, N_STEPS - 1) if i != first]
        i = first
        h = math.log(float(sig[i])) - math.log(float(sig[i + 1]))
        assert abs(float(t[i, 1]) + math.expm1(-2.0 * h)) <= 1e-12  # E at eta 1
    for name in ("euler_a", "lcm"):
        s = lcm(8) if name == "lcm" else karras()
        assert not sampler_coefficients(s.sigmas, name, 0, timesteps=s.timesteps)[:, 2].any()


def test_existing_tables_are_unchanged():
    sig = karras().sigmas
    for name in ("euler", "dpmpp_2m"):
        t = sampler_coefficients(sig, name, 2)
        assert t.shape == (N_STEPS, 3)
        assert torch.equal(t, sampler_coefficients(sig, name, 2, eta=0.3))  # eta does not reach them
    assert SAMPLERS[:2] == ("euler", "dpmpp_2m") and STOCHASTIC_SAMPLERS == ("euler_a", "dpmpp_2m_sde", "lcm")


def test_lcm_schedule_and_table():
    assert lcm(4).timesteps.tolist() == [999.0, 759.0, 499.0, 259.0]
    assert lcm(8).timesteps.tolist() == [999.0, 879.0, 759.0, 639.0, 499.0, 379.0, 259.0, 139.0]
    s = lcm(4)
    train = ((1 - s.alphas_cumprod) / s.alphas_cumprod) ** 0.5
    assert torch.equal(s.sigmas, torch.cat([train[[999, 759, 499, 259]], torch.zeros(1)]))
    assert s.init_noise_sigma == (float(s.sigmas[0]) ** 2 + 1) ** 0.5
    t = sampler_coefficients(s.sigmas, "lcm", timesteps=s.timesteps)
    assert t.shape == (4, 4)
    for i in range(3):
        ts, sg = 10.0 * float(s.timesteps[i]), float(s.sigmas[i])
        want = [0.25 / (ts * ts + 0.25) / math.sqrt(sg * sg + 1), ts / math.sqrt(ts * ts + 0.25), 0.0,
                float(s.sigmas[i + 1])]
        assert float((t[i] - torch.tensor(want, dtype=torch.float64)).abs().max()) <= 1e-15
    assert t[3].tolist() == [0.0, 1.0, 0.0, 0.0]
    assert torch.equal(t, sampler_coefficients(s.sigmas, "lcm", eta=0.0, timesteps=s.timesteps))  # eta is not used
    with pytest.raises(ValueError):
        lcm(51)
    with pytest.raises(ValueError):
        EulerDiscreteScheduler(timestep_spacing="lcm", sigma_schedule="karras")
    with pytest.raises(ValueError):
        EulerDiscreteScheduler(timestep_spacing="lcm", original_inference_steps=0)


def test_refusals():
    from video_style_transfer_amd.pipeline import check_sampler
    sig = karras().sigmas
    for eta in (-0.1, float("nan"), float("inf"), "much", None):
        with pytest.raises(ValueError):
            sampler_coefficients(sig, "euler_a", eta=eta)
        with pytest.raises(ValueError):
            check_sampler("dpmpp_2m_sde", 7.5, 0.0, eta=eta)
    with pytest.raises(ValueError):
        sampler_coefficients(sig, "heun")
    with pytest.raises(ValueError):
        check_sampler("heun", 7.5, 0.0)
    with pytest.raises(ValueError):
        sampler_coefficients(sig, "lcm")  # no timesteps
    with pytest.raises(ValueError):
        sampler_coefficients(sig, "lcm", timesteps=karras().timesteps[:-1])
    with pytest.raises(ValueError):
        check_sampler("lcm", 1.0, 0.0, scheduler=EulerDiscreteScheduler())  # 'leading' spacing
    assert check_sampler("lcm", 1.0, 0.0, scheduler=EulerDiscreteScheduler(timestep_spacing="lcm")) == 0.0
    assert check_sampler("lcm", 1.0, 0.0) == 0.0  # none given: the denoiser builds the LCM one
    assert check_sampler("euler_a", 7.5, 0.7, eta=0.0) == 0.7


def test_step_reference_takes_the_noise():
    g = torch.Generator().manual_seed(1)
    s = karras()
    co = sampler_coefficients(s.sigmas, "dpmpp_2m_sde").float()
    shape = (1, 4, 2, 3, 3)
    lat, hist, xi = (torch.randn(shape, generator=g) for _ in range(3))
    noise = torch.randn(2 * 18, 4, generator=g).to(torch.bfloat16)
    new, D, _ = sampler_step_reference(noise, lat, hist, s.sigmas, co, 4, xi=xi)
    plain, D3, _ = sampler_step_reference(noise, lat, hist, s.sigmas, co[:, :3].contiguous(), 4)
    assert torch.equal(D, D3) and torch.equal(new, plain + float(co[4, 3]) * xi)
    with pytest.raises(ValueError):
        sampler_step_reference(noise, lat, hist, s.sigmas, co, 4)  # d != 0 and no xi
    last, _, _ = sampler_step_reference(noise, lat, hist, s.sigmas, co, N_STEPS - 1)  # d == 0: xi is not needed
    assert torch.equal(last, sampler_step_reference(noise, lat, hist, s.sigmas, co[:, :3].contiguous(), N_STEPS - 1)[0])


def test_library_exports_the_noise_entries():
    from video_style_transfer_amd import _lib
    lib = _lib.load()
    for name in ("vst_noise_bits", "vst_noise_normal", "vst_sampler_step_noise"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    # every entry refuses a NULL pointer before any launch (no device is touched)
    assert lib.vst_noise_bits(None, None, None, 0, 1, 4, 1, 1, 0, 1, None) == 1
    assert lib.vst_noise_normal(None, None, None, 0, 1, 4, 1, 1, 0, 1, None) == 1
    assert lib.vst_sampler_step_noise(None, 2, 7.5, None, None, 1, 4, 1, 1, 0, 1, None, None, None, None, None, None,
                                      None, None, 0, None) == 1
