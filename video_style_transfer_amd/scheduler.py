"""EulerDiscreteScheduler tables for the denoise loop (inference_animatediff.py:217-219, :104-131).

SDXL scheduler config: scaled_linear betas (0.00085 -> 0.012, 1000 train steps), 'leading'
timestep spacing, steps_offset 1, epsilon prediction, linear sigma interpolation, no Karras.
Host-side math only (once per schedule); the per-step arithmetic (scale_model_input, CFG
combine, Euler update) runs in vst_pack_latents / vst_euler_cfg_step on the device, reading
these tables through a device step counter so a captured HIP graph replays every step.
Few-step sampling adds, opt-in, the Karras sigma table, the per-step coefficient table of the
table-driven samplers (vst_sampler_step) and an fp32 restatement of that whole step for the tests.
Stochastic samplers add the (a, b, c, d) tables of Euler ancestral, DPM-Solver++ 2M SDE and LCM, the LCM
timestep spacing, and a host restatement of the device's counter-based noise (philox4x32, noise_reference).
"""
from __future__ import annotations

import math

import numpy as np
import torch


def start_index(num_inference_steps: int, strength: float) -> int:
    """First step of a run that starts from a source clip (diffusers img2img `get_timesteps`): with
    k = min(int(N * strength), N) steps to run, t_start = max(N - k, 0).  strength in (0, 1]; one that leaves no step
    to run is refused."""
    n = int(num_inference_steps)
    s = float(strength)
    if n <= 0:
        raise ValueError(f"num_inference_steps {num_inference_steps} must be positive")
    if not (math.isfinite(s) and 0.0 < s <= 1.0):
        raise ValueError(f"strength {strength} must be in (0, 1]")
    k = min(int(n * s), n)
    if k == 0:
        raise ValueError(f"strength {strength} leaves no step to run at {n} inference steps")
    return max(n - k, 0)


class EulerDiscreteScheduler:
    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, steps_offset=1,
                 timestep_spacing="leading", sigma_schedule="discrete", original_inference_steps=50):
        """sigma_schedule "discrete": the interpolated training sigmas at the spaced timesteps (the reference's
        config).  "karras": the rho = 7 schedule of Karras et al. 2022 (eq. 5) between the first and the last of
        those sigmas, as diffusers' `_convert_to_karras` builds it,
            sigma_i = (smax^(1/rho) + i / (n - 1) * (smin^(1/rho) - smax^(1/rho)))^rho,  then 0 appended,
        with the fractional timesteps of diffusers' `_sigma_to_t`: with ls the log of the 1000 training sigmas and
        k the last index with ls[k] <= log sigma (at most 998), w = clip((ls[k] - log sigma) / (ls[k] - ls[k+1]), 0, 1)
        and t = (1 - w) * k + w * (k + 1).  (diffusers is not a dependency; this restates those two functions.)
        timestep_spacing "lcm" (DESIGN.md §16): the schedule of diffusers' LCMScheduler.set_timesteps.  With
        k = num_train_timesteps // original_inference_steps the origin timesteps are arange(1, original + 1) * k - 1,
        reversed; the n run timesteps are those at indices floor(linspace(0, original, n, endpoint=False)); the sigmas
        are the training sigmas at these integer timesteps, then 0."""
        if sigma_schedule not in ("discrete", "karras"):
            raise ValueError(f"sigma_schedule {sigma_schedule!r}: 'discrete' or 'karras'")
        if timestep_spacing == "lcm":
            if sigma_schedule != "discrete":
                raise ValueError("timestep_spacing 'lcm' takes the training sigmas (sigma_schedule 'discrete')")
            if not 1 <= int(original_inference_steps) <= num_train_timesteps:
                raise ValueError(f"original_inference_steps {original_inference_steps} outside [1, "
                                 f"{num_train_timesteps}]")
        self.original_inference_steps = int(original_inference_steps)
        self.sigma_schedule = sigma_schedule
        self.num_train_timesteps = num_train_timesteps
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.steps_offset = steps_offset
        self.timestep_spacing = timestep_spacing
        self.timesteps = None
        self.sigmas = None

    def set_timesteps(self, num_inference_steps: int, device=None):
        n = num_inference_steps
        if self.timestep_spacing == "lcm":
            orig = self.original_inference_steps
            if not 1 <= n <= orig:
                raise ValueError(f"num_inference_steps {n} outside [1, original_inference_steps = {orig}]")
            origin = (np.arange(1, orig + 1) * (self.num_train_timesteps // orig) - 1)[::-1]
            idx = np.floor(np.linspace(0, orig, n, endpoint=False)).astype(np.int64)
            ts = origin[idx].astype(np.float32)
        elif self.timestep_spacing == "leading":
            ratio = self.num_train_timesteps // n
            ts = (np.arange(0, n) * ratio).round()[::-1].copy().astype(np.float32) + self.steps_offset
        elif self.timestep_spacing == "trailing":
            ratio = self.num_train_timesteps / n
            ts = (np.arange(self.num_train_timesteps, 0, -ratio)).round().copy().astype(np.float32) - 1
        else:  # linspace
            ts = np.linspace(0, self.num_train_timesteps - 1, n, dtype=np.float32)[::-1].copy()
        sig = (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy()
        train = sig
        sig = np.interp(ts, np.arange(0, len(sig)), sig)
        if self.sigma_schedule == "karras":
            sig = karras_sigmas(sig[0], sig[-1], n)
            ts = sigma_to_t(sig, np.log(train.astype(np.float64))).astype(np.float32)
        sig = np.concatenate([sig, [0.0]]).astype(np.float32)
        self.timesteps = torch.from_numpy(ts).to(device)
        self.sigmas = torch.from_numpy(sig).to(device)
        self.num_inference_steps = n

    @property
    def init_noise_sigma(self) -> float:
        m = float(self.sigmas.max())
        return m if self.timestep_spacing in ("linspace", "trailing") else (m ** 2 + 1) ** 0.5

    def scale_model_input(self, sample, step_index):
        return sample / ((self.sigmas[step_index] ** 2 + 1) ** 0.5)

    def add_noise(self, original_samples, noise, timesteps):
        """Training noising (train_animatediff.py:234-236): x + sigma(t) * eps (no input scaling).  The sigma table
        is kept on the samples' device, so the call issues no host copy (graph-capturable)."""
        dev = original_samples.device
        cache = self.__dict__.setdefault("_sig_dev", {})
        if dev not in cache:
            cache[dev] = (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).to(dev)
        s = cache[dev][timesteps.long()].to(original_samples.dtype)
        while s.dim() < original_samples.dim():
            s = s.unsqueeze(-1)
        return original_samples + s * noise


def karras_sigmas(sigma_max: float, sigma_min: float, n: int, rho: float = 7.0) -> np.ndarray:
    """n float64 sigmas from sigma_max down to sigma_min, uniform in sigma^(1/rho) (Karras et al. 2022, eq. 5; diffusers
    `_convert_to_karras`)."""
    ramp = np.linspace(0.0, 1.0, n, dtype=np.float64)
    hi, lo = float(sigma_max) ** (1.0 / rho), float(sigma_min) ** (1.0 / rho)
    return (hi + ramp * (lo - hi)) ** rho


def sigma_to_t(sigma, log_sigmas: np.ndarray) -> np.ndarray:
    """Fractional training timestep of each sigma by linear interpolation in log sigma (diffusers `_sigma_to_t`)."""
    ls = np.log(np.maximum(np.asarray(sigma, dtype=np.float64), 1e-10))
    dists = ls[np.newaxis, :] - log_sigmas[:, np.newaxis]
    low = np.cumsum(dists >= 0, axis=0).argmax(axis=0).clip(max=log_sigmas.shape[0] - 2)
    lo, hi = log_sigmas[low], log_sigmas[low + 1]
    w = np.clip((lo - ls) / (lo - hi), 0.0, 1.0)
    return (1.0 - w) * low + w * (low + 1)


SAMPLERS = ("euler", "dpmpp_2m", "euler_a", "dpmpp_2m_sde", "lcm")
STOCHASTIC_SAMPLERS = SAMPLERS[2:]  # their rows have a fourth column, the weight of fresh noise


def check_eta(eta) -> float:
    try:
        v = float(eta)
    except (TypeError, ValueError):
        raise ValueError(f"eta {eta!r} is not a number") from None
    if not (math.isfinite(v) and v >= 0.0):
        raise ValueError(f"eta {eta} must be finite and >= 0")
    return v


def _stochastic_coefficients(sig, sampler, first_step, eta, timesteps) -> torch.Tensor:
    n = sig.numel() - 1
    if sampler == "lcm":
        if timesteps is None:
            raise ValueError("sampler 'lcm' needs the schedule's timesteps (timestep_spacing 'lcm')")
        ts = torch.as_tensor(timesteps).detach().cpu().to(torch.float64).reshape(-1)
        if ts.numel() != n:
            raise ValueError(f"{ts.numel()} timesteps for {n} steps")
    out = torch.zeros(n, 4, dtype=torch.float64)
    for i in range(n):
        s, s1 = float(sig[i]), float(sig[i + 1])
        if s1 == 0.0:
            row = [0.0, 1.0, 0.0, 0.0]
        elif sampler == "euler_a":
            up = min(s1, eta * math.sqrt(s1 * s1 * (s * s - s1 * s1) / (s * s)))
            down = math.sqrt(s1 * s1 - up * up)
            row = [down / s, 1.0 - down / s, 0.0, up]
        elif sampler == "dpmpp_2m_sde":
            h = math.log(s) - math.log(s1)
            E = -math.expm1(-h - eta * h)
            a, d = (s1 / s) * math.exp(-eta * h), s1 * math.sqrt(-math.expm1(-2.0 * eta * h))
            if i == 0 or i == int(first_step):
                row = [a, E, 0.0, d]
            else:
                r = (math.log(float(sig[i - 1])) - math.log(s)) / h
                row = [a, E * (1.0 + 1.0 / (2.0 * r)), -E / (2.0 * r), d]
        else:  # lcm
            t = 10.0 * float(ts[i])
            row = [0.25 / (t * t + 0.25) / math.sqrt(s * s + 1.0), t / math.sqrt(t * t + 0.25), 0.0, s1]
        out[i] = torch.tensor(row, dtype=torch.float64)
    return out


def sampler_coefficients(sigmas, sampler: str, first_step: int = 0, eta: float = 1.0, timesteps=None) -> torch.Tensor:
    """The per-step coefficients (a, b, c) of one sampler step in this project's VE latent convention,
        x' = a * x + b * D + c * D_prev,   D = x - sigma_i * eps_hat   (the denoised estimate),
    as a float64 table [n][3] for the n + 1 sigmas given (the last one 0); the device keeps it as fp32.
    "euler": (s'/s, 1 - s'/s, 0) with s = sigma_i, s' = sigma_{i+1}: x + (s' - s) * eps_hat rewritten on D.
    "dpmpp_2m": DPM-Solver++(2M) (Lu et al. 2022, alg. 2) as k-diffusion's `sample_dpmpp_2m` steps it: with
    t = -ln sigma, h = t_{i+1} - t_i and r = (t_i - t_{i-1}) / h,
        a = s'/s,  b = -expm1(-h) * (1 + 1 / (2 r)),  c = expm1(-h) / (2 r);
    first order (b = -expm1(-h), c = 0) at `first_step`, the step a run enters at, where there is no D_prev (and at
    step 0, which has no sigma before it); (0, 1, 0) where s' = 0 (the last step returns D).  a + b + c = 1 in
    every row.
    The stochastic samplers return [n][4] rows (a, b, c, d), x' = a x + b D + c D_prev + d xi with xi
    fresh standard normal noise; `eta` (finite, >= 0) scales it and 0 gives the deterministic sampler's (a, b, c):
    "euler_a": k-diffusion's `get_ancestral_step`, up = min(s', eta sqrt(s'^2 (s^2 - s'^2) / s^2)),
        down = sqrt(s'^2 - up^2): (down/s, 1 - down/s, 0, up).
    "dpmpp_2m_sde": k-diffusion's `sample_dpmpp_2m_sde` (midpoint), E = -expm1(-h - eta h):
        ((s'/s) exp(-eta h), E (1 + 1/(2r)), -E/(2r), s' sqrt(-expm1(-2 eta h))), first order (b = E, c = 0) where
        "dpmpp_2m" is.  In both, a + b + c = 1 and (a s)^2 + d^2 = s'^2.
    "lcm": diffusers' `LCMScheduler.step` (sigma_data 0.5, timestep_scaling 10) restated on VE latents; with
        ts = 10 t_i from `timesteps` (the schedule's, timestep_spacing "lcm"), c_skip = 0.25 / (ts^2 + 0.25) and
        c_out = ts / sqrt(ts^2 + 0.25): (c_skip / sqrt(s^2 + 1), c_out, 0, s'); eta is not used.
    Their last row (s' = 0) is (0, 1, 0, 0)."""
    if sampler not in SAMPLERS:
        raise ValueError(f"sampler {sampler!r}: one of {SAMPLERS}")
    eta = check_eta(eta)
    sig = torch.as_tensor(sigmas).detach().cpu().to(torch.float64).reshape(-1)
    n = sig.numel() - 1
    if n < 1 or not bool((sig[:-1] > 0).all()) or not bool((sig[1:] < sig[:-1]).all()) or float(sig[-1]) < 0:
        raise ValueError("sigmas must be positive and strictly decreasing, n + 1 entries with n >= 1")
    if not 0 <= int(first_step) < n:
        raise ValueError(f"first_step {first_step} outside the {n}-step schedule")
    if sampler in STOCHASTIC_SAMPLERS:
        return _stochastic_coefficients(sig, sampler, first_step, eta, timesteps)
    out = torch.zeros(n, 3, dtype=torch.float64)
    for i in range(n):
        s, s1 = float(sig[i]), float(sig[i + 1])
        if s1 == 0.0:
            out[i] = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)
            continue
        a = s1 / s
        if sampler == "euler":
            out[i] = torch.tensor([a, 1.0 - a, 0.0], dtype=torch.float64)
            continue
        h = math.log(s) - math.log(s1)
        e = math.expm1(-h)
        if i == 0 or i == int(first_step):
            out[i] = torch.tensor([a, -e, 0.0], dtype=torch.float64)
        else:
            r = (math.log(float(sig[i - 1])) - math.log(s)) / h
            out[i] = torch.tensor([a, -e * (1.0 + 1.0 / (2.0 * r)), e / (2.0 * r)], dtype=torch.float64)
    return out


def rescale_factor_reference(noise, B: int, guidance: float, phi: float) -> torch.Tensor:
    """fp32 [B]: phi * std(cond_b) / std(eps_hat_b) + (1 - phi) per clip, the factor `rescale_noise_cfg`
    (animatediff/pipeline_animatediff_xl.py:414-425) multiplies eps_hat by; std is torch's default (unbiased) over all
    of clip b.  noise: (2 * B * F * HW, Cl) UNet output rows, uncond clips then cond clips.  Deliberate difference: 1
    where std(eps_hat_b) is 0 (the reference divides by it and gives NaN)."""
    n2 = noise.float().reshape(2, B, -1)
    e = n2[0] + guidance * (n2[1] - n2[0])
    sc, se = n2[1].std(dim=1), e.std(dim=1)
    ok = se > 0
    return torch.where(ok, phi * sc / torch.where(ok, se, torch.ones_like(se)) + (1.0 - phi), torch.ones_like(se))


def sampler_step_reference(noise, lat, hist, sigmas, coef, step: int, *, guidance: float = 7.5, ncopy: int = 2,
                           guidance_rescale: float = 0.0, z0=None, eps=None, mask=None, xi=None):
    """One whole sampler step as vst_sampler_step (with vst_cfg_rescale_factor before it) defines it, fp32 torch:
    noise (ncopy * B * F * HW, Cl) UNet output rows ((k * B + b) * F + f) * HW + p, k = 0 uncond, k = 1 cond;
    lat / hist / z0 / eps (B, Cl, F, H, W); sigmas [n + 1]; coef [n][3] (sampler_coefficients); mask (1 or B, F, H, W).
        eps_hat = u + g (c - u)                      (ncopy 1: the only row)
        eps_hat *= factor[b]                         (guidance_rescale > 0: rescale_factor_reference)
        D = lat - sigma_s * eps_hat
        lat' = a_s * lat + b_s * D + c_s * hist      (hist is not read where c_s == 0)
        lat' = m * lat' + (1 - m) * (z0 + sigma_{s+1} * eps)   (with a mask)
    With coef [n][4] (a stochastic sampler, vst_sampler_step_noise) and xi of lat's shape (the step's noise,
    kernels.noise_normal), lat' += d_s * xi before the blend (xi is not read where d_s == 0).
    Returns (lat', D, factor or None): D is the history the next step reads."""
    B, Cl, F, H, W = lat.shape
    sig = torch.as_tensor(sigmas).float().cpu()
    row = [float(v) for v in torch.as_tensor(coef)[step].float()]
    (a, b, c), d = row[:3], (row[3] if len(row) == 4 else 0.0)
    if d != 0.0 and xi is None:
        raise ValueError(f"row {step} adds noise (d = {d}): pass xi")
    n5 = noise.float().reshape(ncopy, B, F, H, W, Cl).permute(0, 1, 5, 2, 3, 4)
    e = n5[0] + guidance * (n5[1] - n5[0]) if ncopy == 2 else n5[0]
    factor = None
    if guidance_rescale > 0:
        if ncopy != 2:
            raise ValueError("guidance_rescale needs both CFG branches")
        factor = rescale_factor_reference(noise, B, guidance, guidance_rescale)
        e = e * factor.view(B, 1, 1, 1, 1)
    lat = lat.float()
    D = lat - sig[step] * e
    new = a * lat + b * D
    if c != 0.0:
        new = new + c * hist.float()
    if d != 0.0:
        new = new + d * xi.float()
    if mask is not None:
        m = mask.float().unsqueeze(1)
        new = m * new + (1 - m) * (z0.float() + sig[step + 1] * eps.float())
    return new, D, factor


# ---- counter-based noise: the host restatement of csrc/philox.h ----
PHILOX_M = (0xD2511F53, 0xCD9E8D57)  # round multipliers
PHILOX_W = (0x9E3779B9, 0xBB67AE85)  # Weyl key increments


def philox4x32(counter, key, rounds: int = 10) -> np.ndarray:
    """Philox4x32-10 (Salmon et al. 2011; the Random123 constants) in exact integer numpy: counter (..., 4) and key
    (..., 2) words (broadcast against each other) -> uint32 (..., 4)."""
    mask = np.uint64(0xFFFFFFFF)
    c = np.asarray(counter, dtype=np.uint64) & mask
    k = np.asarray(key, dtype=np.uint64) & mask
    x = [c[..., i] for i in range(4)]
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(rounds):
        p0, p1 = np.uint64(PHILOX_M[0]) * x[0], np.uint64(PHILOX_M[1]) * x[2]  # 32 x 32 bits: no overflow in 64
        x = [(p1 >> np.uint64(32)) ^ x[1] ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ x[3] ^ k1, p0 & mask]
        k0, k1 = (k0 + np.uint64(PHILOX_W[0])) & mask, (k1 + np.uint64(PHILOX_W[1])) & mask
    return np.stack(np.broadcast_arrays(*x), axis=-1).astype(np.uint32)


def noise_reference(seed: int, step: int, stream_id: int, shape, F_total=None, f0: int = 0):
    """What vst_noise_bits and vst_noise_normal define for a tensor of `shape` (B, Cl, F, H, W) holding frames
    [f0, f0 + F) of clips of F_total frames (default: whole clips): (uint32 words, float64 normals), both of `shape`.
    For element (b, c, f, p), with P = (b * F_total + f0 + f) * HW + p,
        x = philox4x32((lo32 P, hi32 P, step, stream_id << 16 | c >> 2), (lo32 seed, hi32 seed)),  word x[c & 3],
        u_k = ((x_k >> 9) + 0.5) * 2^-23,  (n0, n1) = sqrt(-2 ln u0) * (cos, sin)(2 pi u1),  (n2, n3) from (u2, u3)."""
    B, Cl, F, H, W = (int(v) for v in shape)
    HW = H * W
    F_total = F if F_total is None else int(F_total)
    if not (0 <= stream_id < 1 << 16 and 0 < Cl <= 1 << 18 and 0 <= f0 and f0 + F <= F_total):
        raise ValueError(f"noise_reference: stream_id {stream_id}, Cl {Cl} or frames [{f0}, {f0 + F}) of {F_total}")
    seed = int(seed) & (2 ** 64 - 1)
    G = (Cl + 3) // 4
    b, g, f, p = np.meshgrid(np.arange(B, dtype=np.uint64), np.arange(G, dtype=np.uint64),
                             np.arange(F, dtype=np.uint64), np.arange(HW, dtype=np.uint64), indexing="ij")
    P = (b * np.uint64(F_total) + np.uint64(f0) + f) * np.uint64(HW) + p
    counter = np.stack([P & np.uint64(0xFFFFFFFF), P >> np.uint64(32), np.full_like(P, int(step) & 0xFFFFFFFF),
                        np.uint64(stream_id << 16) | g], axis=-1)
    x = philox4x32(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))  # (B, G, F, HW, 4)
    u = ((x >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    r = np.sqrt(-2.0 * np.log(u[..., 0::2]))
    a = 2.0 * np.pi * u[..., 1::2]
    n = np.stack([r * np.cos(a), r * np.sin(a)], axis=-1).reshape(x.shape)  # (r0 c, r0 s, r1 c, r1 s)

    def planes(t):  # (B, G, F, HW, 4) -> (B, Cl, F, H, W): channel c = 4 g + lane
        return np.ascontiguousarray(t.transpose(0, 1, 4, 2, 3).reshape(B, 4 * G, F, H, W)[:, :Cl])
    return torch.from_numpy(planes(x)), torch.from_numpy(planes(n))
