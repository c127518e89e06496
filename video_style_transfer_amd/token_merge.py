"""Token merging for the spatial transformer blocks.

Bolya & Hoffman, "Token Merging for Fast Stable Diffusion" (CVPR-W 2023), the `tomesd` package: before attn1 (and
optionally before the feed-forward) of a spatial BasicTransformerBlock the r most redundant tokens of every image are
merged into their most similar destination token, the module runs on N - r rows per image, and every token takes the
result of the row it went to.  `TokenMerging` mirrors the arguments of `tomesd.apply_patch`; the kernels are
kernels.tome_match / tome_merge / tome_unmerge_add (csrc/token_merge.hip, include/vst.h).

A block computes ONE plan from its input hidden states and uses it for attn1 and for the feed-forward, as tomesd does
(its compute_merge runs once per block).  The plan, the scores and the merged rows live in static buffers per layer, so
a captured denoise step replays; with `use_rand` the destination of every 2 x 2 cell is drawn on the device from the
Philox counters at (seed, step counter, layer, cell), so the pattern still changes from step to step under replay, is
the same for every image of the batch (as in tomesd) and for every frame shard of a clip.

Image quality at a given ratio is not evaluated in this project.
"""
from __future__ import annotations

import dataclasses
import math
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from . import kernels as K
from ._lib import VstError
from .scheduler import philox4x32

TOME_STREAM = 2  # stream id of the destination draw in the noise counters (0: sampler step, 1: FreeInit)


@dataclass
class TokenMerging:
    """tomesd.apply_patch's arguments.  `ratio` of the tokens of an image are merged (at most all sources: with 2 x 2
    cells 0.75); `max_downsample` 1, 2, 4 or 8: blocks whose tokens are down-sampled more than that against the latent
    run as without the option (SDXL's first attention level is 2, the next 4); `sx`, `sy`: the cell; `use_rand`: a
    random destination per cell instead of its top-left token; `merge_attn` / `merge_mlp`: around attn1 / the
    feed-forward.  `merge_crossattn` is refused.  An instance owns the static device buffers of the layers it has run
    (`layers`: layer id -> LayerPlan, also the hook the tests read the recorded plans through), so use one per model."""
    ratio: float = 0.5
    max_downsample: int = 2
    sx: int = 2
    sy: int = 2
    use_rand: bool = True
    merge_attn: bool = True
    merge_crossattn: bool = False
    merge_mlp: bool = False
    # device state, never compared: the seed and the step counter the destination draw reads (bind), the buffers
    seed: Optional[torch.Tensor] = field(default=None, compare=False, repr=False)
    step_idx: Optional[torch.Tensor] = field(default=None, compare=False, repr=False)
    layers: dict = field(default_factory=dict, compare=False, repr=False)
    _merged: dict = field(default_factory=dict, compare=False, repr=False)

    def __post_init__(self):
        check_token_merging_values(self)

    # ---- what is merged where ----
    @property
    def enabled(self) -> bool:
        return self.ratio > 0.0 and (self.merge_attn or self.merge_mlp)

    def active(self, latent_tokens: int, N: int) -> bool:
        """A block of N tokens per image, in a model whose latent has latent_tokens, merges."""
        return self.enabled and downsample_of(latent_tokens, N) <= self.max_downsample

    def sizes(self, H: int, W: int):
        """(N, Nd, Ns, r) at an H x W level."""
        return K.tome_sizes(H, W, self.sy, self.sx, self.ratio)

    # ---- device state ----
    def bind(self, seed: torch.Tensor, step_idx: torch.Tensor):
        """The device seed (int64 [1]) and step counter (int32 [1]) the destination draw reads; a denoiser binds its
        own, so the pattern follows its step counter under graph replay."""
        self.seed, self.step_idx = seed, step_idx
        return self

    def _counters(self, device):
        if not self.use_rand:
            return None, None
        if self.seed is None or self.seed.device != device:
            self.seed = torch.zeros(1, dtype=torch.int64, device=device)
            self.step_idx = torch.zeros(1, dtype=torch.int32, device=device)
        return self.seed, self.step_idx

    def layer(self, layer_id: int, x: torch.Tensor, nimg: int, H: int, W: int) -> "LayerPlan":
        """The static buffers of one layer at this batch and level (allocated at the first call, outside capture)."""
        N, Nd, Ns, r = self.sizes(H, W)
        key = (nimg, H, W, x.shape[1], r, x.device)
        st = self.layers.get(layer_id)
        if st is None or st.key != key:
            st = LayerPlan(key, nimg, H, W, N, Nd, Ns, r, K.tome_plan(nimg, N, x.device),
                           torch.zeros((nimg, Ns), dtype=torch.float32, device=x.device))
            self.layers[layer_id] = st
        return st

    def merged_buffer(self, rows: int, C: int, device) -> torch.Tensor:
        """One bf16 [rows, C] buffer per shape, shared by the layers (they run one after the other on one stream)."""
        key = (rows, C, device)
        buf = self._merged.get(key)
        if buf is None:
            buf = self._merged[key] = torch.empty((rows, C), dtype=torch.bfloat16, device=device)
        return buf

    def match(self, layer_id: int, x: torch.Tensor, nimg: int, H: int, W: int) -> "LayerPlan":
        """Compute the layer's plan from the block's input hidden states x [nimg * H * W, C]."""
        st = self.layer(layer_id, x, nimg, H, W)
        seed, step = self._counters(x.device)
        K.tome_match(x, nimg, H, W, st.r, st.plan, sy=self.sy, sx=self.sx, seed=seed, step_idx=step, layer=layer_id,
                     best=st.best)
        return st

    def merge(self, st: "LayerPlan", x: torch.Tensor) -> torch.Tensor:
        out = self.merged_buffer(st.nimg * (st.N - st.r), x.shape[1], x.device)
        return K.tome_merge(x, st.nimg, st.H, st.W, st.r, st.plan, sy=self.sy, sx=self.sx, out=out)

    def unmerge_add(self, st: "LayerPlan", o: torch.Tensor, residual: Optional[torch.Tensor]) -> torch.Tensor:
        return K.tome_unmerge_add(o, st.nimg, st.N, st.r, st.plan, residual=residual)


@dataclass
class LayerPlan:
    key: tuple
    nimg: int
    H: int
    W: int
    N: int
    Nd: int
    Ns: int
    r: int
    plan: torch.Tensor   # int32 [nimg, 6 N + 4], the layout of include/vst.h
    best: torch.Tensor   # fp32 [nimg, Ns]

    def slot(self) -> torch.Tensor:
        """int32 [nimg, N]: the merged row of every token, as the last match wrote it."""
        return self.plan[:, :self.N]


def check_token_merging_values(tm: TokenMerging) -> None:
    """The option's values, refused before anything is allocated."""
    try:
        ratio = float(tm.ratio)
    except (TypeError, ValueError):
        raise VstError(f"token_merging: ratio {tm.ratio!r} is not a number") from None
    if not (math.isfinite(ratio) and 0.0 <= ratio <= 1.0):
        raise VstError(f"token_merging: ratio {tm.ratio} must lie in [0, 1]")
    if tm.max_downsample not in (1, 2, 4, 8):
        raise VstError(f"token_merging: max_downsample {tm.max_downsample!r}; one of 1, 2, 4, 8")
    for name in ("sx", "sy"):
        v = getattr(tm, name)
        if not isinstance(v, int) or isinstance(v, bool) or v < 1:
            raise VstError(f"token_merging: {name} {v!r} must be a positive integer")
    if tm.sx * tm.sy > 65536:
        raise VstError(f"token_merging: cells of {tm.sy} x {tm.sx} tokens; at most 65536 per cell")
    if tm.merge_crossattn:
        raise VstError("token_merging: merge_crossattn is not supported (attn2 runs on every token)")


def as_token_merging(tm) -> Optional[TokenMerging]:
    """None, a TokenMerging, a dict of its fields or a ratio."""
    if tm is None or isinstance(tm, TokenMerging):
        return tm
    if isinstance(tm, dict):
        return TokenMerging(**tm)
    if isinstance(tm, (int, float)) and not isinstance(tm, bool):
        return TokenMerging(ratio=float(tm))
    raise VstError(f"token_merging: {tm!r}; None, a TokenMerging, a dict of its fields or a ratio")


def downsample_of(latent_tokens: int, N: int) -> int:
    """tomesd's level of a block: ceil(sqrt(latent tokens / the block's tokens))."""
    return int(math.ceil(math.sqrt(latent_tokens / N)))


def active_levels(tm: Optional[TokenMerging], latent_hw, levels) -> list:
    """Which of the (H, W) levels merge for a latent of latent_hw."""
    h, w = latent_hw
    return [tm is not None and tm.active(h * w, H * W) for H, W in levels]


def check_token_merging(model, tm: Optional[TokenMerging], latent_hw, x=None) -> None:
    """Refuse, before any launch (and so before a capture), what the merged blocks cannot honour: the training path, a
    level outside the kernels' sizes, another processor than AnimateDiffAttnProcessor2_0 on a merged attn1."""
    if tm is None or not tm.enabled:
        return
    check_token_merging_values(tm)
    from .attention_processor import AnimateDiffAttnProcessor2_0
    from .unet_motion import BasicTransformerBlock, Transformer2DModel
    if torch.is_grad_enabled() and ((x is not None and x.requires_grad) or
                                    any(p.requires_grad for p in model.parameters())):
        raise VstError("token_merging: inference only; the training path (autograd) has no merged backward")
    h, w = latent_hw
    for (H, W), C in spatial_levels(model, h, w):
        if not tm.active(h * w, H * W):
            continue
        if H * W > K.TOME_MAX_TOKENS or C % 64 or C > K.TOME_MAX_CHANNELS:
            raise VstError(f"token_merging: a level of {H} x {W} tokens of {C} channels; the matching takes up to "
                           f"{K.TOME_MAX_TOKENS} tokens per image and a multiple of 64 channels up to "
                           f"{K.TOME_MAX_CHANNELS} (lower max_downsample, or a smaller latent)")
        if tm.sy > H or tm.sx > W:
            raise VstError(f"token_merging: cells of {tm.sy} x {tm.sx} on a level of {H} x {W} tokens")
    if tm.merge_attn:
        for name, m in model.named_modules():
            if isinstance(m, BasicTransformerBlock) and not m.temporal and \
                    not isinstance(m.attn1.processor, AnimateDiffAttnProcessor2_0):
                raise VstError(f"token_merging: {name}.attn1 has a {type(m.attn1.processor).__name__}; the merged "
                               f"attention runs through AnimateDiffAttnProcessor2_0")
    assign_layer_ids(model)


def assign_layer_ids(model) -> None:
    """Number the spatial transformer blocks in module order (the layer word of the destination draw)."""
    from .unet_motion import BasicTransformerBlock
    if model.__dict__.get("_vst_tome_numbered"):
        return
    i = 0
    for m in model.modules():
        if isinstance(m, BasicTransformerBlock) and not m.temporal:
            m.__dict__["_vst_tome_layer"] = i
            i += 1
    model.__dict__["_vst_tome_numbered"] = True


def spatial_levels(model, h: int, w: int) -> list:
    """((H, W), channels) of every level of `model` that has spatial transformer blocks, for an h x w latent."""
    out = []
    ch = model.config.block_out_channels
    for i, blk in enumerate(model.down_blocks):
        if blk.attentions is not None:
            out.append(((h, w), ch[i]))
        if blk.downsamplers is not None:
            h, w = (h + 1) // 2, (w + 1) // 2
    out.append(((h, w), ch[-1]))
    return out


# ---- host restatement of the destination draw (tests, tools) ----
def destination_offsets(H: int, W: int, sy: int, sx: int, seed: Optional[int], step: int = 0, layer: int = 0):
    """int64 [hc, wc]: the in-cell offset o of every whole cell, (oy, ox) = (o // sx, o % sx); seed None: zeros."""
    hc, wc = H // sy, W // sx
    if seed is None:
        return torch.zeros(hc, wc, dtype=torch.int64)
    seed = int(seed) & (2 ** 64 - 1)
    cell = np.arange(hc * wc, dtype=np.uint64)
    counter = np.stack([cell, np.zeros_like(cell), np.full_like(cell, int(step) & 0xFFFFFFFF),
                        np.full_like(cell, (TOME_STREAM << 16) | int(layer))], axis=-1)
    x = philox4x32(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
    return torch.from_numpy((x[:, 0].astype(np.int64) % (sy * sx)).reshape(hc, wc))


def destination_tokens(H: int, W: int, sy: int, sx: int, offsets: torch.Tensor) -> torch.Tensor:
    """int64 [Nd]: the token p = y * W + x of every cell's destination, in raster order of the cells."""
    hc, wc = H // sy, W // sx
    cy, cx = torch.meshgrid(torch.arange(hc), torch.arange(wc), indexing="ij")
    y = cy * sy + offsets // sx
    x = cx * sx + offsets % sx
    return (y * W + x).reshape(-1)


def replace(tm: TokenMerging, **kw) -> TokenMerging:
    """A copy with other values and no device state."""
    vals = {f.name: getattr(tm, f.name) for f in dataclasses.fields(tm) if f.compare}
    vals.update(kw)
    return TokenMerging(**vals)
