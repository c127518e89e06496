"""Regional prompts: what text applies where (no line of the reference does this).

R <= 4 regions share the spatial attn2 layers.  Region 0 is the base prompt; region r has text states S_r [L, D] per
batch element and a raw weight map m_r >= 0 per (batch element, frame) at latent resolution h x w.  At a transformer
level of H x W tokens (h = s H, w = s W)

    p_r[Y, X] = mean of m_r over the s x s latent cell (fp32, avg_pool2d),     w_r = p_r / sum_r p_r,

and every query row blends the regions' attentions with its w (kernels.region_attention).  A row with w_r == 0 takes
nothing from region r; a region that is zero on a whole 128-query block is not even loaded there.

`RegionPrompts` owns static device buffers, in the manner of ip_adapter.ImagePrompt and lora_gate.LoraGate: the
states [B, R, L, D] and one fp32 [B*F*H*W, 4] table per attention level.  `set_weights` rewrites every table in
place, so a captured step that holds their addresses sees the new maps on its next replay; `set_states` writes in
place too, but the text K/V projected from the old states are stale afterwards (attention_processor._text_kv keys on
the tensor's version and projects again into a new buffer), so a captured step must be dropped.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
import torch.nn.functional as F

from . import kernels as K

BF16 = torch.bfloat16
F32 = torch.float32
MAX_REGIONS = K.REGION_MAX
MAX_MASKS = MAX_REGIONS - 1


def _err(msg):
    return K._lib.VstError(msg)


# ------------------------------------------------------------------------------------------ levels
def attention_levels(model, hw) -> list:
    """[(H, W)] at which the spatial transformers of `model` run for an hw = (h, w) latent, finest first, each once."""
    from .token_merge import spatial_levels
    out = []
    for lv, _ in spatial_levels(model, int(hw[0]), int(hw[1])):
        if lv not in out:
            out.append(lv)
    return out


def check_levels(levels: Sequence[tuple], hw) -> list:
    """[(H, W, s)] of the levels of an h x w latent; ValueError unless every level divides the latent into whole
    s x s cells (h, w divisible by the deepest level's factor)."""
    h, w = int(hw[0]), int(hw[1])
    out = []
    for H, W in levels:
        s = h // H if H else 0
        if H < 1 or W < 1 or s < 1 or s & (s - 1) or H * s != h or W * s != w:  # (levels halve: s is a power of 2)
            deepest = min(levels, key=lambda lv: lv[0] * lv[1])
            raise ValueError(f"region prompts: a {h} x {w} latent does not divide into the {deepest[0]} x {deepest[1]} "
                             f"tokens of the deepest attention level in whole square cells (level {H} x {W})")
        out.append((H, W, s))
    return out


# ------------------------------------------------------------------------------------------ weights
def _check_raw(t: torch.Tensor, what: str):
    if not bool(torch.isfinite(t).all()):
        raise ValueError(f"{what}: values must be finite")
    if bool((t < 0).any()):
        raise ValueError(f"{what}: values must be >= 0")


def region_weights(masks, frames: int, hw, base_mask=None) -> torch.Tensor:
    """Raw weights fp32 [frames, n + 1, h, w] (CPU) of one clip from n <= 3 user masks: masks [n, F or 1, h, w] (or a
    sequence of [F or 1, h, w]), bool or float in [0, 1]; region 0, the base prompt, gets max(1 - sum of the masks, 0),
    or `base_mask` [F or 1, h, w] when given.  ValueError for more than 3 masks, a shape that does not fit, a value
    that is not finite or outside [0, 1], or a pixel that no region covers (possible only with a base_mask)."""
    h, w = int(hw[0]), int(hw[1])
    frames = int(frames)
    if not torch.is_tensor(masks):
        masks = list(masks)
        masks = torch.stack([torch.as_tensor(m) for m in masks]) if masks else torch.zeros(0, 1, h, w)
    n = masks.shape[0] if masks.dim() else -1
    if masks.dim() != 4:
        raise ValueError(f"region masks: shape {tuple(masks.shape)}, expected (n, {frames} or 1, {h}, {w})")
    if n > MAX_MASKS:
        raise ValueError(f"region masks: {n} masks; at most {MAX_MASKS} beside the base prompt")

    def fit(t, what):
        t = torch.as_tensor(t).detach().to("cpu", F32)
        if t.shape[-3] not in (1, frames) or tuple(t.shape[-2:]) != (h, w):
            raise ValueError(f"{what}: shape {tuple(t.shape)}, expected (.., {frames} or 1, {h}, {w})")
        _check_raw(t, what)
        if bool((t > 1).any()):
            raise ValueError(f"{what}: values must be in [0, 1]")
        return t.expand(*t.shape[:-3], frames, h, w)
    m = fit(masks, "region masks")
    if base_mask is None:
        base = (1.0 - m.sum(0)).clamp_min(0.0)
    else:
        base = torch.as_tensor(base_mask)
        if base.dim() != 3:
            raise ValueError(f"region base_mask: shape {tuple(base.shape)}, expected ({frames} or 1, {h}, {w})")
        base = fit(base, "region base_mask")
    raw = torch.cat([base.unsqueeze(0), m], 0).permute(1, 0, 2, 3).contiguous()
    if bool((raw.sum(1) <= 0).any()):
        raise ValueError("region masks: some latent pixel has no weight in any region (sum of the weights is 0)")
    return raw


def pooled_weights(raw: torch.Tensor, s: int) -> torch.Tensor:
    """The definition at one level: fp32 [rows, R, h/s, w/s] = avg_pool2d(raw, s) normalised over the regions."""
    p = F.avg_pool2d(raw.to(F32), s) if s > 1 else raw.to(F32)
    return p / p.sum(1, keepdim=True)


# ------------------------------------------------------------------------------------------ the object
class RegionPrompts:
    """states: [B, R, L, D] text states, B token batches in UNet batch order, each serving `frames` consecutive
    frames; raw: [B * frames, R, h, w] raw weights; levels: the (H, W) of every attention level (attention_levels).
    Refused (ValueError): R outside 1..4, shapes that do not fit, weights that are not finite, negative, or zero in
    every region at some latent pixel, and a latent that the deepest level does not divide."""

    def __init__(self, states, raw, frames: int, levels: Sequence[tuple], device=None):
        st = torch.as_tensor(states)
        raw = torch.as_tensor(raw)
        if st.dim() != 4 or 0 in st.shape:
            raise ValueError(f"region prompts: states {tuple(st.shape)}, expected (batches, regions, tokens, dim)")
        B, R, L, D = st.shape
        if not 1 <= R <= MAX_REGIONS:
            raise ValueError(f"region prompts: {R} regions; the kernel blends 1 to {MAX_REGIONS}")
        if int(frames) < 1:
            raise ValueError(f"region prompts: {frames} frames per token batch")
        if raw.dim() != 4:
            raise ValueError(f"region prompts: weights {tuple(raw.shape)}, expected (rows, regions, h, w)")
        device = torch.device(device) if device is not None else st.device
        self.frames = int(frames)
        self.rows = B * self.frames
        self.R, self.L, self.D = R, L, D
        self.hw = tuple(int(v) for v in raw.shape[-2:])
        self.levels = check_levels(list(levels), self.hw)
        self._check_weights(raw)
        self.states = st.detach().to(device, BF16).contiguous().clone()
        # (the text K/V cache is keyed on the tensor object: one view for the life of the prompts)
        self.states_rows = self.states.view(B * R, L, D)
        self.tables = {(H, W): torch.zeros(self.rows * H * W, MAX_REGIONS, dtype=F32, device=device)
                       for H, W, _ in self.levels}
        self.version = 0
        self.set_weights(raw)
        self.version = 0

    @property
    def device(self):
        return self.states.device

    def _check_weights(self, raw):
        want = (self.rows, self.R) + self.hw
        if tuple(raw.shape) != want:
            raise ValueError(f"region prompts: weights {tuple(raw.shape)}, expected {want}")
        _check_raw(raw, "region prompts: weights")
        if bool((raw.sum(1) <= 0).any()):
            raise ValueError("region prompts: some latent pixel has no weight in any region (sum of the weights is 0)")

    def set_weights(self, raw):
        """New raw weights [rows, R, h, w], validated before anything is written: every level's table is re-pooled and
        re-normalised in place."""
        raw = torch.as_tensor(raw).detach()
        self._check_weights(raw)
        raw = raw.to(self.device, F32)
        for H, W, s in self.levels:
            wts = pooled_weights(raw, s)
            self.tables[(H, W)].view(self.rows, H, W, MAX_REGIONS)[..., :self.R].copy_(wts.permute(0, 2, 3, 1))
        self.version += 1
        return self

    def set_states(self, states):
        """New text states of the same shape, in place.  The K/V projected from the old ones no longer apply: a
        captured step that reads them must be dropped (AnimateDiffDenoiser does)."""
        st = torch.as_tensor(states)
        if tuple(st.shape) != tuple(self.states.shape):
            raise ValueError(f"region prompts: states {tuple(st.shape)}, expected {tuple(self.states.shape)}")
        self.states.copy_(st.detach())
        self.version += 1
        return self

    def table(self, hw) -> Optional[torch.Tensor]:
        return self.tables.get((int(hw[0]), int(hw[1])))


# ------------------------------------------------------------------------------------------ checks
def refuse_lora_gate(region_prompts, lora_gate):
    """The one rule between two options: regional prompts and a LoRA gate do not go together (per-frame text K/V times
    regions is out of scope).  Stated here only (ForwardOptions.resolve through check_forward, the denoiser's two
    setters, a direct processor call)."""
    if region_prompts is not None and lora_gate is not None:
        raise _err("region_prompts: not together with a lora_gate (the gated text K/V are per frame)")


def check_forward(model, rp, rows: int, hw, enc, lora_gate=None):
    """Refuse, before any launch, regional prompts the call cannot honour (ForwardOptions.resolve)."""
    if rp is None:
        return
    if not isinstance(rp, RegionPrompts):
        raise _err(f"region_prompts: expected a region_prompts.RegionPrompts, got {type(rp).__name__}")
    refuse_lora_gate(rp, lora_gate)
    if rp.rows != rows:
        raise _err(f"region_prompts: {rp.rows} rows, expected B * F = {rows}")
    for lv in attention_levels(model, hw):
        t = rp.table(lv)
        if t is None or t.shape[0] != rows * lv[0] * lv[1]:
            raise _err(f"region_prompts: no weight table for the {lv[0]} x {lv[1]} attention level of a "
                       f"{hw[0]} x {hw[1]} latent (tables: {sorted(rp.tables)})")
    if enc is None:
        raise _err("region_prompts: the call has no encoder_hidden_states; attn2 would run as self-attention")
    if tuple(enc.shape[1:]) != (rp.L, rp.D):
        raise _err(f"region_prompts: states of {rp.L} x {rp.D} per region, encoder_hidden_states of "
                   f"{enc.shape[1]} x {enc.shape[2]}")
    if rows % enc.shape[0] or rows // enc.shape[0] != rp.frames:
        raise _err(f"region_prompts: {rp.frames} frames per token batch, encoder_hidden_states of {enc.shape[0]} "
                   f"batches for {rows} images")
