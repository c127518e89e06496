"""FreeInit: iterative noise re-initialisation with a 3-D frequency mix.

Wu et al., "FreeInit: Bridging Initialization Gap in Video Diffusion Models" (ECCV 2024); in diffusers
`FreeInitMixin.enable_free_init`, carried by the AnimateDiff pipelines.  The denoise loop runs `num_iters` times.
Between two passes the result x of the last one is re-noised to the top of the schedule with the noise z_init the run
was entered with, z_T = x + z_init, and only its low spatio-temporal frequencies are kept; the high ones come from fresh
noise r = init_noise_sigma * xi:
  out = Re IDFT3(M . DFT3(z_T) + (1 - M) . DFT3(r)) = r + L(z_T - r),   L = IDFT3 o (M~ .) o DFT3
over the (F, h, w) axes of every (clip, channel) volume.  M is the low-pass mask with frequency 0 at the centre
(`freq_filter`, as diffusers builds it); M~ = `dft_order(M)` is the same mask in unshifted DFT order, symmetrised under
k -> -k, which makes L a real operator for every size: r + L(z_T - r) is then exactly the real part diffusers keeps,
odd sizes included (tests/test_free_init.py).  The kernel (`kernels.free_init_mix`, csrc/free_init.hip) takes M~.

`FreeInit` is the option of AnimateDiffDenoiser(free_init=...) / enable_free_init(...).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

METHODS = ("butterworth", "gaussian", "ideal")


@dataclass(frozen=True)
class FreeInit:
    """diffusers' enable_free_init arguments (its defaults).  `use_fast_sampling` is not taken: the step count is part
    of the captured step."""
    num_iters: int = 3
    method: str = "butterworth"
    order: int = 4
    spatial_stop_frequency: float = 0.25
    temporal_stop_frequency: float = 0.25

    def __post_init__(self):
        check_free_init(self.num_iters, self.method, self.order, self.spatial_stop_frequency,
                        self.temporal_stop_frequency)


def check_free_init(num_iters, method, order, spatial_stop_frequency, temporal_stop_frequency) -> None:
    """ValueError unless num_iters and order are integers >= 1, the method is known and both stop frequencies are finite
    numbers >= 0."""
    for name, v in (("num_iters", num_iters), ("order", order)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"free_init {name} {v!r} must be an integer >= 1")
    if method not in METHODS:
        raise ValueError(f"free_init method {method!r}: one of {METHODS}")
    for name, v in (("spatial_stop_frequency", spatial_stop_frequency),
                    ("temporal_stop_frequency", temporal_stop_frequency)):
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"free_init {name} {v!r} is not a number") from None
        if isinstance(v, bool) or not (math.isfinite(f) and f >= 0.0):
            raise ValueError(f"free_init {name} {v} must be a finite value >= 0")


def check_free_init_arg(free_init) -> None:
    """Validate a `free_init=` argument (None | FreeInit | a dict of its fields | its positional tuple) without
    allocating anything."""
    if free_init is None or isinstance(free_init, FreeInit):
        return
    try:
        if isinstance(free_init, dict):
            FreeInit(**free_init)
        elif isinstance(free_init, (tuple, list)):
            FreeInit(*free_init)
        else:
            raise TypeError
    except TypeError:
        raise ValueError(f"free_init {free_init!r}: None, a FreeInit, a dict of its fields or its tuple") from None


def as_free_init(free_init):
    """None, a FreeInit, a dict of its fields or its tuple -> None or a FreeInit; ValueError on bad values."""
    check_free_init_arg(free_init)
    if free_init is None or isinstance(free_init, FreeInit):
        return free_init
    return FreeInit(**free_init) if isinstance(free_init, dict) else FreeInit(*free_init)


def check_free_init_run(free_init, shard=None, source=False) -> None:
    """What a FreeInit run cannot be combined with, each with its reason."""
    if free_init is None:
        return
    if shard is not None and shard.world > 1:
        raise ValueError("free_init transforms whole clips along the frame axis; under a frame shard of world "
                         f"{shard.world} the other ranks hold part of every clip")
    if source:
        raise ValueError("free_init re-noises to the top of the schedule and keeps only the low frequencies, which "
                         "would throw away the source clip's high frequencies: not together with a source run")


def freq_filter(F: int, H: int, W: int, fi: FreeInit) -> torch.Tensor:
    """The low-pass mask M, fp64 [F, H, W], frequency 0 at index (F / 2, H / 2, W / 2) (the fftshift order): with
    d_s / d_t the spatial / temporal stop frequencies and n the order,
      d2 = ((d_s / d_t)(2 t / F - 1))^2 + (2 h / H - 1)^2 + (2 w / W - 1)^2
      butterworth 1 / (1 + (d2 / d_s^2)^n);  gaussian exp(-d2 / (2 d_s^2));  ideal 1 where d2 <= 2 d_s, else 0;
    all zeros when d_s or d_t is 0."""
    if min(F, H, W) < 1:
        raise ValueError(f"freq_filter: sizes ({F}, {H}, {W}) must be positive")
    d_s, d_t = float(fi.spatial_stop_frequency), float(fi.temporal_stop_frequency)
    if d_s == 0.0 or d_t == 0.0:
        return torch.zeros(F, H, W, dtype=torch.float64)

    def axis(n):
        return 2.0 * torch.arange(n, dtype=torch.float64) / n - 1.0
    t, h, w = (d_s / d_t) * axis(F), axis(H), axis(W)
    d2 = t[:, None, None] ** 2 + h[None, :, None] ** 2 + w[None, None, :] ** 2
    if fi.method == "butterworth":
        return 1.0 / (1.0 + (d2 / d_s ** 2) ** fi.order)
    if fi.method == "gaussian":
        return torch.exp(-d2 / (2.0 * d_s ** 2))
    return (d2 <= 2.0 * d_s).to(torch.float64)


def dft_order(M: torch.Tensor) -> torch.Tensor:
    """M~ of a shifted mask M [F, H, W]: u = ifftshift(M), M~(k) = (u(k) + u(-k mod N)) / 2.  For real z,
    IDFT3(M~ . DFT3(z)) is real and equals Re IDFT3(u . DFT3(z))."""
    if M.dim() != 3:
        raise ValueError(f"dft_order: a [F, H, W] mask, got {tuple(M.shape)}")
    u = torch.fft.ifftshift(M, dim=(0, 1, 2))
    mirrored = torch.roll(torch.flip(u, dims=(0, 1, 2)), shifts=(1, 1, 1), dims=(0, 1, 2))
    return (u + mirrored) / 2


def mix_reference(x, init, noise, filt, scale, dtype=torch.float64) -> torch.Tensor:
    """out = r + L(x + init - r), r = scale * noise, on (..., F, H, W) tensors with torch.fft in `dtype`; filt is M~
    [F, H, W]; init may be None."""
    ctype = torch.complex128 if dtype == torch.float64 else torch.complex64
    r = scale * noise.to(dtype)
    z = x.to(dtype) - r if init is None else x.to(dtype) + init.to(dtype) - r
    low = torch.fft.ifftn(torch.fft.fftn(z.to(ctype), dim=(-3, -2, -1)) * filt.to(dtype), dim=(-3, -2, -1)).real
    return r + low
