"""FreeU in the up path.

The reference's up blocks call diffusers' `apply_freeu(resolution_idx, hidden, skip, s1, s2, b1, b2)` before every skip
concatenation of their first two stages (animatediff/unet_block.py:399-417, unziplora_unet/unet_block.py:853-867;
switched by `enable_freeu` / `disable_freeu` of unziplora_unet/unet_2d_condition.py):
  stage 0 (the first up block): hidden[:, :C_h // 2] *= b1, skip = fourier_filter(skip, threshold=1, scale=s1);
  stage 1: the same with b2, s2; later stages untouched.
C_h is the channel count of the hidden states at that resnet.  `fourier_filter` casts to fp32, takes the 2-D FFT,
fftshifts, multiplies the 2 x 2 block [H//2 - 1 : H//2 + 1, W//2 - 1 : W//2 + 1] by the scale, shifts back, inverts,
keeps the real part and casts back.  After the shift index H//2 is frequency 0, so the scaled bins are {-1, 0} x {-1, 0}
and the filter is a rank-4 correction of the map with a closed form (`fourier_filter_reference`); the kernel
(`kernels.freeu`, csrc/freeu.hip) evaluates the same form on NHWC bf16 rows.

`FreeU` holds the four values as a static fp32 [2, 2] device table ((s, b) per stage) that the kernel reads on the
device: `set` rewrites it in place, so a captured denoise step replays with the new values.
"""
from __future__ import annotations

import math

import torch

SDXL = dict(s1=0.9, s2=0.2, b1=1.3, b2=1.4)  # the FreeU authors' values for SDXL


def check_freeu(s1, s2, b1, b2) -> tuple:
    """The four FreeU values as floats; ValueError unless every one is a finite number > 0."""
    out = []
    for name, v in (("s1", s1), ("s2", s2), ("b1", b1), ("b2", b2)):
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"freeu {name} {v!r} is not a number") from None
        if not (math.isfinite(f) and f > 0.0):
            raise ValueError(f"freeu {name} {v} must be a finite value > 0")
        out.append(f)
    return tuple(out)


class FreeU:
    def __init__(self, s1, s2, b1, b2, device=None):
        self.values = check_freeu(s1, s2, b1, b2)  # refused before anything is allocated
        self.table = torch.empty(2, 2, dtype=torch.float32, device=device if device is not None else "cuda")
        self._write()

    def _write(self):
        s1, s2, b1, b2 = self.values
        self.table.copy_(torch.tensor([[s1, b1], [s2, b2]], dtype=torch.float32))

    def set(self, s1, s2, b1, b2):
        """New values, validated before the table is rewritten in place."""
        self.values = check_freeu(s1, s2, b1, b2)
        self._write()
        return self

    @property
    def device(self):
        return self.table.device

    def __repr__(self):
        s1, s2, b1, b2 = self.values
        return f"FreeU(s1={s1}, s2={s2}, b1={b1}, b2={b2})"


def as_freeu(freeu, device=None):
    """None, a FreeU, or its (s1, s2, b1, b2) -> None or a FreeU on `device`; ValueError on bad values."""
    check_freeu_arg(freeu)
    return freeu if freeu is None or isinstance(freeu, FreeU) else FreeU(*freeu, device=device)


def check_freeu_arg(freeu) -> None:
    """Validate a `freeu=` argument (None | FreeU | (s1, s2, b1, b2)) without allocating anything."""
    if freeu is None or isinstance(freeu, FreeU):
        return
    try:
        s1, s2, b1, b2 = freeu
    except (TypeError, ValueError):
        raise ValueError(f"freeu {freeu!r}: None, a FreeU or (s1, s2, b1, b2)") from None
    check_freeu(s1, s2, b1, b2)


def fourier_filter_reference(x: torch.Tensor, scale: float, dtype=torch.float64) -> torch.Tensor:
    """fourier_filter(x, threshold=1, scale) on [..., H, W] in closed form, evaluated in `dtype` (fp64 or fp32) and
    returned in it: with th = 2 pi h / H, ph = 2 pi w / W and, per map,
      m0 = S x, a = S x cos th, b = S x sin th, c = S x cos ph, d = S x sin ph, e = S x cos(th + ph),
      f = S x sin(th + ph),
      y = x + (scale - 1) / (H W) (m0 + a cos th + b sin th + c cos ph + d sin ph + e cos(th + ph) + f sin(th + ph)).
    H, W >= 2 (below that the definition's mask slice is empty or wraps)."""
    H, W = x.shape[-2:]
    if H < 2 or W < 2:
        raise ValueError(f"fourier_filter: a {H} x {W} map; H and W must be >= 2")
    x = x.to(dtype)
    th = (2 * math.pi / H) * torch.arange(H, dtype=torch.float64)[:, None]
    ph = (2 * math.pi / W) * torch.arange(W, dtype=torch.float64)[None, :]
    one = torch.ones(H, W, dtype=torch.float64)
    basis = torch.stack([one, torch.cos(th) * one, torch.sin(th) * one, torch.cos(ph) * one, torch.sin(ph) * one,
                         torch.cos(th + ph), torch.sin(th + ph)]).to(dtype=dtype, device=x.device)   # [7, H, W]
    sums = torch.einsum("...hw,jhw->...j", x, basis)
    return x + ((scale - 1.0) / (H * W)) * torch.einsum("...j,jhw->...hw", sums, basis)


def apply_freeu_reference(stage: int, hidden: torch.Tensor, skip: torch.Tensor, s1, s2, b1, b2,
                          dtype=torch.float64):
    """diffusers' apply_freeu on NCHW tensors: (hidden, skip) after the backbone scale of the first C_h // 2 channels
    of the tensor given and the skip filter, for stage 0 (b1, s1) and 1 (b2, s2); any other stage returns both
    unchanged.  The filter is the closed form evaluated in `dtype`, cast back to the skip's dtype."""
    if stage not in (0, 1):
        return hidden, skip
    s, b = ((s1, b1), (s2, b2))[stage]
    hidden = hidden.clone()
    half = hidden.shape[1] // 2
    hidden[:, :half] = hidden[:, :half] * b
    return hidden, fourier_filter_reference(skip, s, dtype).to(skip.dtype)
