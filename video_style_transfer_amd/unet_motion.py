"""UNetMotionModel (SDXL + AnimateDiff motion modules), MI355X-native.

Module tree and parameter names follow diffusers' UNetMotionModel, which the reference builds with
`UNetMotionModel.from_unet2d` (animatediff/utils.py:13-45) and then patches with UnZipLoRA
(unziplora_unet/utils.py:388-484) and AnimateDiffAttnProcessor2_0 (inference_animatediff.py:209-215).
So `load_state_dict` of a reference/diffusers checkpoint (plus Stage-1 LoRA keys) drops in.

Execution is MI355X-first: activations never leave the token-major NHWC layout
[(b*F + f)*H*W + p, C] (bf16); every conv is an implicit GEMM, every projection a fused MFMA
GEMM with bias / residual / GEGLU / temb epilogues, GroupNorm+SiLU and LayerNorm(+PE) are single
passes, the skip concatenation of the up path is read from two sources instead of copied, and the
motion modules read the frame axis in place (no permutes).  The public forward keeps the
reference signature and 5-D (B, C, F, h, w) in/out.

Block semantics (diffusers ~0.30, restated in oracle/unet.py with citations):
  ResnetBlock2D:        GN+SiLU -> conv3x3 (+ time_emb_proj(SiLU(emb))) -> GN+SiLU -> conv3x3 (+ shortcut)
  Transformer2DModel:   GN(eps 1e-6) -> proj_in -> BasicTransformerBlock* -> proj_out -> + residual
  BasicTransformerBlock: LN -> attn1 -> +res ; LN -> attn2(text) -> +res ; LN -> GEGLU FF -> +res
  motion module:        GN over (C-group, F, H, W) -> proj_in -> block(self, self, PE before each attn)
                        -> proj_out -> + residual
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass
from typing import Optional

import torch
from torch import nn

from . import kernels as K
from .attention_processor import AnimateDiffAttnProcessor2_0, AttnCall, Attention, input_lora_ops
from .config import UNetMotionConfig
from .freeu import FreeU, as_freeu
from .lora_linear import LoRACompatibleLinear, build_ops, lora_in_gemm, run_ops
from .token_merge import TokenMerging, as_token_merging, check_token_merging, spatial_levels
from .weights import sinusoid_table

BF16 = torch.bfloat16


class _F32Cache:
    """fp32 device copies of bf16 params (norm affine, conv/linear bias) keyed by tensor version."""

    @staticmethod
    def get(p: torch.Tensor) -> torch.Tensor:
        if p.requires_grad:  # trained parameters change under graph replay without a version bump: no cache
            return p.detach().float().contiguous()
        key = (p.data_ptr(), p._version)
        c = p.__dict__.get("_vst_f32")
        if c is None or c[0] != key:
            c = (key, p.detach().float().contiguous())
            p.__dict__["_vst_f32"] = c
        return c[1]


f32 = _F32Cache.get


class GroupNorm(nn.GroupNorm):
    def run(self, x1, nsamples, rows_per_sample, *, silu=False, x2=None, out=None):
        return K.group_norm(x1, nsamples, rows_per_sample, self.num_groups, self.eps, f32(self.weight), f32(self.bias),
                            silu=silu, x2=x2, out=out)


class LayerNorm(nn.LayerNorm):
    def run(self, x, *, pe=None, pe_div=1, pe_mod=1, out=None):
        return K.layer_norm(x, f32(self.weight), f32(self.bias), self.eps, pe=pe, pe_div=pe_div, pe_mod=pe_mod,
                            out=out)

    def run_lora(self, x, ops):
        """(LN(x), LN(x) @ ops.a^T or None): the LoRA down-projection fused into the normalisation pass when
        the consuming projections carry one and the shapes suit the fused kernel."""
        C = x.shape[1]
        if ops is None or ops.a is None or ops.a.shape[0] > 64 or C % 32 or C > 1280 or lora_in_gemm(ops, x.shape[0]):
            return self.run(x), None
        return K.layer_norm_lora(x, f32(self.weight), f32(self.bias), self.eps, ops.a, r_alg=ops.r)


class Conv3x3(nn.Conv2d):
    """nn.Conv2d(k=3, pad=1) whose device weight is re-laid out once to [Cout, (ky,kx,ci)]."""

    def __init__(self, cin, cout, stride=1):
        super().__init__(cin, cout, 3, stride=stride, padding=1)

    def kernel_weight(self):
        key = (self.weight.data_ptr(), self.weight._version)
        c = self.__dict__.get("_vst_w")
        if c is None or c[0] != key:
            co, ci = self.weight.shape[:2]
            w = self.weight.detach().permute(0, 2, 3, 1).reshape(co, 9 * ci)
            kp = (9 * ci + 7) & ~7
            if kp != 9 * ci:
                w = torch.cat([w, w.new_zeros(co, kp - 9 * ci)], 1)
            c = (key, w.to(BF16).contiguous())
            self.__dict__["_vst_w"] = c
        return c[1]

    def folded_weight(self):
        """kernel_weight() folded for the upsample conv (K.fold_upsample_weight), cached per weight version like it.  A
        weight that trains is re-folded on every call (GEGLU.geglu_ops: graph replay updates it without a version
        bump); a frozen one is folded once, at the first eager call."""
        if self.weight.requires_grad:
            return K.fold_upsample_weight(self.kernel_weight())
        key = (self.weight.data_ptr(), self.weight._version)
        c = self.__dict__.get("_vst_wfold")
        if c is None or c[0] != key:
            c = (key, K.fold_upsample_weight(self.kernel_weight()))
            self.__dict__["_vst_wfold"] = c
        return c[1]

    def run(self, x1, nimg, H, W, *, x2=None, upsample=False, row_bias=None, row_bias_div=1, residual=None):
        # the upsample conv as four 2x2 convs on folded weights wherever the shape allows (never a question of nimg)
        if (upsample and x2 is None and row_bias is None and residual is None and self.stride[0] == 1
                and K.conv3x3_up_folded_applies(self.in_channels, self.out_channels)):
            return K.conv3x3_up_folded(x1, nimg, H, W, self.folded_weight(), f32(self.bias))
        return K.conv3x3(x1, nimg, H, W, self.kernel_weight(), f32(self.bias), x2=x2, stride=self.stride[0],
                         upsample=upsample, row_bias=row_bias, row_bias_div=row_bias_div, residual=residual)


class Conv1x1(nn.Conv2d):
    def __init__(self, cin, cout):
        super().__init__(cin, cout, 1)

    def kernel_weight(self):
        key = (self.weight.data_ptr(), self.weight._version)
        c = self.__dict__.get("_vst_w")
        if c is None or c[0] != key:
            c = (key, self.weight.detach().reshape(self.weight.shape[0], -1).to(BF16).contiguous())
            self.__dict__["_vst_w"] = c
        return c[1]

    def run(self, x1, x2=None):
        return K.linear(x1, self.kernel_weight(), f32(self.bias), x2=x2)


class Linear(LoRACompatibleLinear):
    """Plain projection (proj_in/out, FF, embeddings) — LoRACompatibleLinear without a lora layer."""

    def run(self, x, *, residual=None, out=None):
        return run_ops(x, build_ops([self], 1.0), residual=residual, out=out)


@dataclass(frozen=True)
class TemporalContext:
    """Sliding-window frame attention for clips longer than the motion modules' trained length (DESIGN.md "Long
    clips"): windows of `length` frames every `stride` frames, blended `flat` or `pyramid`.  Active when a clip has more
    than `length` frames; shorter clips run exactly as without it."""
    length: int
    stride: int = 4
    weighting: str = "pyramid"

    def __post_init__(self):
        K.context_windows(self.length, self.length, self.stride)  # 1 <= length <= 32, 1 <= stride <= length
        K.context_weights(self.length, self.weighting)

    def active(self, F: int) -> bool:
        return F > self.length


def check_clip_length(F: int, max_seq_length: int, tc: Optional[TemporalContext]):
    """Refuse, before any launch, a clip the motion modules cannot attend over: more frames than positional rows with
    no context windows, or windows longer than the table."""
    if tc is not None and tc.length > max_seq_length:
        raise K._lib.VstError(f"context_length {tc.length} exceeds the motion modules' {max_seq_length} positions")
    if F > max_seq_length and (tc is None or not tc.active(F)):
        raise K._lib.VstError(f"a clip of {F} frames exceeds the motion modules' {max_seq_length} positions: pass "
                              f"context_length (<= {max_seq_length}) to attend inside sliding windows")


@dataclass(frozen=True)
class CrossFrameAttention:
    """Cross-frame (extended) spatial self-attention (DESIGN.md "Cross-frame spatial self-attention"): attn1 of every
    spatial transformer block attends to its own frame's tokens plus those of the `sources` frames of the same clip,
    under one softmax.  One or two distinct sources, each "first" (frame 0), "prev" (frame max(f - 1, 0)) or a frame
    index.  Inactive on single-frame clips, which run exactly as without it.
    `adain` "qk" or "qkv" (StyleAligned): before that attention, the queries and keys (and values) of
    every frame are AdaIN-normalised, per column, to the statistics of the anchor frame, the first source that is a
    fixed frame ("first" or an index).  None: no such step.  Its values and its need of a fixed-frame source are
    checked by check_cross_frame."""
    sources: tuple = ("first",)
    adain: Optional[str] = None

    def __post_init__(self):
        src = (self.sources,) if isinstance(self.sources, (str, int)) else tuple(self.sources)
        object.__setattr__(self, "sources", src)
        if not 1 <= len(src) <= 2:
            raise ValueError(f"cross_frame: {len(src)} sources; one or two")
        if len({K.frame_source(s) for s in src}) != len(src):
            raise ValueError(f"cross_frame: sources {src} are not distinct")

    def active(self, F: int) -> bool:
        return F > 1

    @property
    def anchor(self) -> Optional[int]:
        """The frame the AdaIN normalises to: the first source that is a fixed frame, None when there is none."""
        return next((s for s in map(K.frame_source, self.sources) if s >= 0), None)

    @property
    def adain_blocks(self) -> int:
        """How many of the q | k | v column blocks the AdaIN covers (0: no AdaIN)."""
        return {None: 0, "qk": 2, "qkv": 3}[self.adain]


def as_cross_frame(cf) -> Optional[CrossFrameAttention]:
    """None, a CrossFrameAttention, or its sources (("first",), "prev", 3, ...)."""
    return cf if cf is None or isinstance(cf, CrossFrameAttention) else CrossFrameAttention(cf)


def check_cross_frame(model, F: int, cf: Optional[CrossFrameAttention], shard=None, hw=None):
    """Refuse, before any launch, a cross_frame option the spatial self-attention cannot honour on a clip of F
    frames (all ranks' frames together).  `hw`: the latent's (h, w), where the caller knows it; the AdaIN's unbiased
    variance needs two tokens per frame at every level."""
    if cf is None:
        return
    if cf.adain not in (None, "qk", "qkv"):
        raise K._lib.VstError(f"cross_frame: adain {cf.adain!r}; expected None, \"qk\" or \"qkv\"")
    if cf.adain is not None and cf.anchor is None:
        raise K._lib.VstError(f"cross_frame: adain={cf.adain!r} normalises to a fixed anchor frame, and sources "
                              f"{cf.sources} name none (\"first\" or a frame index)")
    if not cf.active(F):
        return
    # (the fewest tokens are at the deepest level of the down path; the up path's levels are never smaller)
    if cf.adain is not None and hw is not None and min(H * W for (H, W), _ in spatial_levels(model, *hw)) < 2:
        raise K._lib.VstError(f"cross_frame: adain={cf.adain!r} takes a variance over each frame's tokens, and a "
                              f"{hw[0]} x {hw[1]} latent leaves a level of this model fewer than 2 per frame")
    if shard is not None and shard.world > 1:
        raise K._lib.VstError("cross_frame: a source frame's keys/values live on another rank under frame sharding "
                              f"(world {shard.world}); run the clip unsharded")
    for s in cf.sources:
        if isinstance(s, int) and s >= F:
            raise K._lib.VstError(f"cross_frame: source frame {s} >= F = {F}")
    bad = model.__dict__.get("_vst_xframe_bad_heads")
    if bad is None:  # head sizes are fixed at construction: scanned once per model
        bad = [n for n, m in model.named_modules()
               if isinstance(m, BasicTransformerBlock) and not m.temporal and m.attn1.dim_head != 64]
        model.__dict__["_vst_xframe_bad_heads"] = bad
    if bad:
        raise K._lib.VstError(f"cross_frame: the cross-frame attention kernel is specialised for head_dim 64; "
                              f"{bad[0]}.attn1 has another")


@dataclass(frozen=True)
class ForwardOptions:
    """The per-call options of the UNet forward, normalised and checked.  `resolve` is the way to one
    for a model call: holding an instance means the checks have run, so nothing below looks again.  (Built directly,
    from the option objects themselves, only to run a block on its own.)  None: the option is off, the plain launches.
    `temporal_context`: the motion modules attend inside sliding windows when the clip is longer than its length.
    `cross_frame` (given as a CrossFrameAttention or its sources, e.g. ("first",)): attn1 of the spatial transformer
    blocks also attends to the source frames of the same clip.  `lora_gate` (lora_gate.LoraGate with B * F rows, one
    per (batch element, frame) in row order; under a shard this rank's frames): the content / style strength of the
    UnZipLoRA delta of the spatial transformer blocks' projections, per row; the motion modules are not gated.
    `freeu` (given as a freeu.FreeU or its (s1, s2, b1, b2)): FreeU in the first two up blocks (§17).  `image_prompt`
    (ip_adapter.ImagePrompt with B * F rows): the image tokens of the IP-Adapter attn2 layers (load_ip_adapter, §20);
    required when they are installed, refused when they are not.  `token_merging` (given as a TokenMerging, a dict of
    its fields or a ratio; §22): the spatial blocks up to its max_downsample merge tokens around attn1 (and the
    feed-forward).  `region_prompts` (region_prompts.RegionPrompts with B * F rows; §24): regional prompts, every
    spatial attn2 attends to the regions' own text states, blended per pixel by their weight maps, and does not read
    encoder_hidden_states (whose L and D they must share); not together with a lora_gate."""
    temporal_context: Optional[TemporalContext] = None
    cross_frame: Optional[CrossFrameAttention] = None
    lora_gate: Optional[object] = None
    freeu: Optional[FreeU] = None
    image_prompt: Optional[object] = None
    token_merging: Optional[TokenMerging] = None
    region_prompts: Optional[object] = None

    @classmethod
    def resolve(cls, model, B: int, F: int, hw, shard=None, x=None, *, use_model_defaults: bool, enc=None, **given):
        """The options `given` (by field name, in the forms forward() takes) for a call of `model` on B clips of F
        frames (this rank's, under `shard`) of an hw = (h, w) latent; `x`: the call's input, for its device and
        whether it asks for gradients.  `use_model_defaults`: freeu / token_merging not given are what enable_freeu /
        enable_token_merging set (forward()); else None means off (forward_tokens()).  `enc`: the call's
        encoder_hidden_states, which regional prompts are checked against.
        Every refusal is raised here, before any launch, each check once and in this order: the image prompt against
        the model (and against a lora_gate), cross_frame, the freeu values, token_merging, the clip length against
        the motion modules' positions, the lora_gate's rows, the regional prompts (rows, a table per attention level,
        the text shape, and against a lora_gate)."""
        from .ip_adapter import check_forward  # (local import: ip_adapter imports the attention processors)
        from .region_prompts import check_forward as check_regions
        o = cls(**given)  # (an option that does not exist is a TypeError here)
        F_clip = F * (shard.world if shard is not None else 1)
        check_forward(model, o.image_prompt, B * F, o.lora_gate)
        cross_frame = as_cross_frame(o.cross_frame)
        check_cross_frame(model, F_clip, cross_frame, shard, hw)
        freeu, token_merging = o.freeu, o.token_merging
        if use_model_defaults:
            freeu = model.freeu if freeu is None else freeu
            token_merging = model.token_merging if token_merging is None else token_merging
        freeu = as_freeu(freeu, x.device if x is not None else model.conv_in.weight.device)
        token_merging = as_token_merging(token_merging)
        check_token_merging(model, token_merging, hw, x)
        if model.config.motion_modules:
            check_clip_length(F_clip, model.config.motion_max_seq_length, o.temporal_context)
        if o.lora_gate is not None and o.lora_gate.rows != B * F:
            raise K._lib.VstError(f"lora_gate: {o.lora_gate.rows} rows, expected B * F = {B * F}")
        check_regions(model, o.region_prompts, B * F, hw, enc, o.lora_gate)
        return dataclasses.replace(o, cross_frame=cross_frame, freeu=freeu, token_merging=token_merging)


@dataclass
class FwdCtx:
    B: int                 # clips in the batch (CFG-batched: 2x)
    F: int                 # frames per clip
    emb_silu: torch.Tensor  # [B, T] bf16, SiLU(time + add embedding)
    enc: Optional[torch.Tensor]  # [B, L, D] bf16 text states
    cross_kwargs: dict
    opts: ForwardOptions = ForwardOptions()
    shard: Optional[object] = None  # frame_shard.FrameShard when the clip's frames span ranks (F is per rank)
    temb: Optional[dict] = None     # ResnetBlock2D -> fp32 [B, Cout] view of the batched time_emb_proj output
    latent_hw: Optional[tuple] = None   # the latent's (h, w): a block's down-sampling level is measured against it
    spatial_hw: Optional[tuple] = None  # the (H, W) of the tokens of the Transformer2DModel being run (the cells' grid)


# --------------------------------------------------------------------------------------- blocks
class GEGLU(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.proj = Linear(dim_in, dim_out * 2)

    def geglu_ops(self):
        """proj weight with hidden/gate rows interleaved per 32-output block (GEMM GEGLU epilogue).  Cached per
        parameter version while the weights are frozen; trained weights are re-interleaved on every call (a cache
        keyed on the version would go stale under HIP-graph replay, which updates parameters without Python)."""
        w, b = self.proj.weight, self.proj.bias
        if w.requires_grad or b.requires_grad:
            return self._interleaved(w, b)
        key = (w.data_ptr(), w._version, b.data_ptr(), b._version)
        c = self.__dict__.get("_vst_geglu")
        if c is None or c[0] != key:
            c = (key, self._interleaved(w, b))
            self.__dict__["_vst_geglu"] = c
        return c[1]

    @staticmethod
    def _interleaved(w, b):
        inner = w.shape[0] // 2
        idx = torch.arange(inner, device=w.device).view(-1, 32)
        idx = torch.cat([idx, idx + inner], 1).reshape(-1)
        return w.detach()[idx].to(BF16).contiguous(), b.detach()[idx].float().contiguous()


class FeedForward(nn.Module):
    """diffusers FeedForward(activation_fn="geglu"): net = [GEGLU, Dropout, Linear]."""

    def __init__(self, dim, mult=4):
        super().__init__()
        inner = dim * mult
        self.net = nn.ModuleList([GEGLU(dim, inner), nn.Dropout(0.0), Linear(inner, dim)])

    def run(self, x, residual):
        w, b = self.net[0].geglu_ops()
        h = K.linear(x, w, b, geglu=True)
        return self.net[2].run(h, residual=residual)


class BasicTransformerBlock(nn.Module):
    """unziplora_unet/unzip_attention.py:13-239 / diffusers BasicTransformerBlock (norm_type layer_norm)."""

    def __init__(self, dim, heads, head_dim, cross_attention_dim=None, temporal=False, max_seq_length=32):
        super().__init__()
        self.temporal = temporal
        self.norm1 = LayerNorm(dim)
        self.attn1 = Attention(dim, None, heads, head_dim, temporal=temporal)
        self.norm2 = LayerNorm(dim)
        self.attn2 = Attention(dim, None if temporal else cross_attention_dim, heads, head_dim, temporal=temporal)
        self.norm3 = LayerNorm(dim)
        self.ff = FeedForward(dim)
        if temporal:
            self.pos_embed = _SinusoidalPE(dim, max_seq_length)

    def run(self, x, nimg, N, ctx: FwdCtx):
        """x: [nimg*N, C] -> same.  A spatial block merges tokens (ctx.opts.token_merging) only where ctx.spatial_hw
        gives the (H, W) of its N tokens: the cells are cut on that grid."""
        C = x.shape[1]
        opts = ctx.opts
        if self.temporal:
            pe = f32(self.pos_embed.pe).view(-1, C)
            tc = opts.temporal_context
            if tc is not None and tc.active(ctx.F):
                # LayerNorm WITHOUT the positional term: the windowed kernel adds pe[position in window] . Wqkv^T per
                # window behind one projection per frame; the fused q/k/v GEMM steps aside
                pe_kw, context = {}, (tc, pe)
            else:
                pe_kw, context = dict(pe=pe, pe_div=N, pe_mod=ctx.F), None
            for norm, attn in ((self.norm1, self.attn1), (self.norm2, self.attn2)):
                n = norm.run(x, **pe_kw)
                x = attn(n.view(nimg, N, C), _vst=AttnCall(residual=x, frames=ctx.F, context=context)).view(-1, C)
        else:
            scale = ctx.cross_kwargs.get("scale", 1.0)
            gate = opts.lora_gate
            cf = opts.cross_frame if opts.cross_frame is not None and opts.cross_frame.active(ctx.F) else None
            frames = ctx.F if cf is not None else None
            tm, plan = self._token_merging(x, nimg, N, ctx)
            if plan is not None and tm.merge_attn:
                # attn1 on the merged rows (no fused residual, the LoRA down-projection inside the GEMM); every token
                # then takes the row it went to, on top of the block's residual
                m = tm.merge(plan, self.norm1.run(x))
                call = AttnCall(frames=frames, cross_frame=cf, lora_gate=gate)
                o = self.attn1(m.view(nimg, N - plan.r, C), _vst=call, **ctx.cross_kwargs).view(-1, C)
                x = tm.unmerge_add(plan, o, x)
            else:
                n, u = self.norm1.run_lora(x, input_lora_ops(self.attn1, True, scale))
                call = AttnCall(residual=x, lora_u=u, frames=frames, cross_frame=cf, lora_gate=gate)
                x = self.attn1(n.view(nimg, N, C), _vst=call, **ctx.cross_kwargs).view(-1, C)
            n, u = self.norm2.run_lora(x, input_lora_ops(self.attn2, False, scale))
            call = AttnCall(residual=x, lora_u=u, lora_gate=gate, image_prompt=opts.image_prompt,
                            regions=self._regions(ctx, nimg, N))
            x = self.attn2(n.view(nimg, N, C), encoder_hidden_states=ctx.enc, _vst=call, **ctx.cross_kwargs).view(-1, C)
            if plan is not None and tm.merge_mlp:
                m = tm.merge(plan, self.norm3.run(x))
                return tm.unmerge_add(plan, self.ff.run(m, residual=None), x)
        n = self.norm3.run(x)
        return self.ff.run(n, residual=x)

    @staticmethod
    def _regions(ctx: FwdCtx, nimg, N):
        """(the regional prompts, the weight table of this block's level), or None without the option."""
        rp = ctx.opts.region_prompts
        if rp is None:
            return None
        wts = None if ctx.spatial_hw is None else rp.table(ctx.spatial_hw)
        if wts is None or wts.shape[0] != nimg * N:
            raise K._lib.VstError(f"region_prompts: no weight table for a block of {nimg} x {N} tokens at level "
                                  f"{ctx.spatial_hw}")
        return rp, wts

    def _token_merging(self, x, nimg, N, ctx: FwdCtx):
        """(the option, this block's plan computed from its input x), or (None, None) where the block runs as without
        the option: off, ratio 0, no tokens to merge, or a level above max_downsample."""
        tm, hw = ctx.opts.token_merging, ctx.spatial_hw
        if tm is None or hw is None or hw[0] * hw[1] != N or not tm.enabled:
            return None, None
        H, W = hw
        lat = ctx.latent_hw or hw
        if not tm.active(lat[0] * lat[1], N) or tm.sizes(H, W)[3] == 0:
            return None, None
        if torch.is_grad_enabled() and x.requires_grad:
            raise K._lib.VstError("token_merging: inference only; the training path (autograd) has no merged backward")
        if tm.merge_attn and not isinstance(self.attn1.processor, AnimateDiffAttnProcessor2_0):
            raise K._lib.VstError(f"token_merging: attn1 has a {type(self.attn1.processor).__name__}; the merged "
                                  f"attention runs through AnimateDiffAttnProcessor2_0")
        return tm, tm.match(self.__dict__.get("_vst_tome_layer", 0), x, nimg, H, W)


class _SinusoidalPE(nn.Module):
    def __init__(self, dim, max_len=32):
        super().__init__()
        self.register_buffer("pe", sinusoid_table(dim, max_len))


class Transformer2DModel(nn.Module):
    """unziplora_unet/transformer_2d.py:137-352 (continuous input, use_linear_projection=True)."""

    def __init__(self, heads, head_dim, C, layers, cross_attention_dim, groups=32):
        super().__init__()
        self.norm = GroupNorm(groups, C, eps=1e-6)
        self.proj_in = Linear(C, C)
        self.transformer_blocks = nn.ModuleList(
            [BasicTransformerBlock(C, heads, head_dim, cross_attention_dim) for _ in range(layers)])
        self.proj_out = Linear(C, C)

    def run(self, x, nimg, H, W, ctx):
        h = self.norm.run(x, nimg, H * W)
        h = self.proj_in.run(h)
        if ctx.opts.token_merging is not None or ctx.opts.region_prompts is not None:
            ctx = dataclasses.replace(ctx, spatial_hw=(H, W))
        for blk in self.transformer_blocks:
            h = blk.run(h, nimg, H * W, ctx)
        return self.proj_out.run(h, residual=x)


class MotionModule(nn.Module):
    """diffusers AnimateDiffTransformer3D (motion module built by UNetMotionModel.from_unet2d)."""

    def __init__(self, C, heads=8, groups=32, max_seq_length=32):
        super().__init__()
        self.norm = GroupNorm(groups, C, eps=1e-6)
        self.proj_in = Linear(C, C)
        self.transformer_blocks = nn.ModuleList(
            [BasicTransformerBlock(C, heads, C // heads, None, temporal=True, max_seq_length=max_seq_length)])
        self.proj_out = Linear(C, C)

    def run(self, x, nimg, H, W, ctx):
        HW = H * W
        shard = ctx.shard
        B, G = nimg // ctx.F, self.norm.num_groups
        if shard is not None and shard.world > 1 and shard.exchange == "all_gather":
            # north-star exchange (frame_shard.py): the whole clip on every rank, this rank's frames kept at the end.
            # With overlap, the batch's two halves (the CFG pair) are gathered by two async all-gathers issued up front,
            # so half 1's gather runs under half 0's module (the gather overlapped with compute)
            Fl, P = ctx.F, shard.world
            F = Fl * P
            tctx = dataclasses.replace(ctx, F=F)
            halves = 2 if shard.overlap and B % 2 == 0 else 1
            nb, rows = B // halves, (B // halves) * Fl * HW
            ends = [shard.gather_frames_begin(x[i * rows:(i + 1) * rows], nb, Fl, HW) for i in range(halves)]
            out = torch.empty_like(x) if halves > 1 else None
            for i in range(halves):
                end, _src = ends[i]
                xf = end()
                part = K.group_norm_frame_partials(xf, nb * F, HW, G)
                h = K.group_norm_apply_partials(xf, nb, F, HW, G, self.norm.eps, f32(self.norm.weight),
                                                f32(self.norm.bias), part, 1)
                h = self.proj_in.run(h)
                for blk in self.transformer_blocks:
                    h = blk.run(h, nb * F, HW, tctx)
                ends[i] = None
                if halves == 1:
                    return self.proj_out.run(shard.local_frames_of(h, nb, Fl, HW), residual=x)
                self.proj_out.run(shard.local_frames_of(h, nb, Fl, HW), residual=x[i * rows:(i + 1) * rows],
                                  out=out[i * rows:(i + 1) * rows])
            return out
        # GroupNorm statistics over every frame of a clip, from per-frame partials merged in one fixed frame order:
        # the same bits whether this process holds the whole clip or a frame shard of it
        part = K.group_norm_frame_partials(x, nimg, HW, G)
        P = 1 if shard is None else shard.world
        if P > 1:
            part = shard.all_gather(part)
            if shard.overlap and B % 2 == 0 and HW % P == 0:
                return self._run_overlapped(x, B, ctx.F, HW, P, ctx, part)
        h = K.group_norm_apply_partials(x, B, ctx.F, HW, G, self.norm.eps, f32(self.norm.weight), f32(self.norm.bias),
                                        part, P)
        h = self.proj_in.run(h)
        if P == 1:
            for blk in self.transformer_blocks:
                h = blk.run(h, nimg, HW, ctx)
            return self.proj_out.run(h, residual=x)
        # frames of each clip spread over ranks (frame_shard.py): frame-axis work on a pixel shard holding every frame
        Fl = ctx.F
        h = shard.to_pixels(h, B, Fl, HW)
        tctx = dataclasses.replace(ctx, F=Fl * P)
        with K.fusion_world(1):  # (these HW // P pixels are this rank's share already)
            for blk in self.transformer_blocks:
                h = blk.run(h, B * Fl * P, HW // P, tctx)
        h = shard.to_frames(h, B, Fl, HW)
        return self.proj_out.run(h, residual=x)

    def _run_overlapped(self, x, B, Fl, HW, P, ctx, part):
        """The all-to-all branch with the batch in two halves (the CFG pair's uncond / cond clips), so each half's
        exchange runs while the other half computes (FrameShard.pipelined): GroupNorm + proj_in of half 1 under half
        0's frame -> pixel exchange, half 0's transformer block under half 1's, and so on.  Every op is row-wise on
        its half's rows (the GroupNorm statistics are per clip, from the all-gathered partials), so the output is the
        one-half schedule's bits (tests/test_frame_shard.py)."""
        G, nb = self.norm.num_groups, B // 2
        rows = nb * Fl * HW
        out = torch.empty_like(x)
        tctx = dataclasses.replace(ctx, F=Fl * P)
        w, bias = f32(self.norm.weight), f32(self.norm.bias)

        def pre(i):
            xs = x[i * rows:(i + 1) * rows]
            ps = part[:, i * nb * Fl:(i + 1) * nb * Fl].contiguous()  # [P, nb*Fl, chunks, G, 2]: this half's clips
            h = K.group_norm_apply_partials(xs, nb, Fl, HW, G, self.norm.eps, w, bias, ps, P)
            return self.proj_in.run(h)

        def mid(i, h):
            with K.fusion_world(1):  # (these HW // P pixels are this rank's share already)
                for blk in self.transformer_blocks:
                    h = blk.run(h, nb * Fl * P, HW // P, tctx)
            return h

        def post(i, h):
            self.proj_out.run(h, residual=x[i * rows:(i + 1) * rows], out=out[i * rows:(i + 1) * rows])

        ctx.shard.pipelined(2, pre, mid, post, nb, Fl, HW)
        return out


class ResnetBlock2D(nn.Module):
    def __init__(self, cin, cout, temb, groups=32, eps=1e-5):
        super().__init__()
        self.in_channels, self.out_channels = cin, cout
        self.norm1 = GroupNorm(groups, cin, eps=eps)
        self.conv1 = Conv3x3(cin, cout)
        self.time_emb_proj = Linear(temb, cout)
        self.norm2 = GroupNorm(groups, cout, eps=eps)
        self.dropout = nn.Dropout(0.0)
        self.conv2 = Conv3x3(cout, cout)
        self.conv_shortcut = Conv1x1(cin, cout) if cin != cout else None

    def run(self, x1, nimg, H, W, ctx, x2=None):
        HW = H * W
        h = self.norm1.run(x1, nimg, HW, silu=True, x2=x2)
        if ctx.temb is not None and self in ctx.temb:
            temb = ctx.temb[self]  # view of the one batched projection (UNetMotionModel.batched_temb)
        else:
            temb = self.time_emb_proj.run(ctx.emb_silu).float()  # [B, cout]; bf16-rounded like the reference
        h = self.conv1.run(h, nimg, H, W, row_bias=temb, row_bias_div=ctx.F * HW)
        h = self.norm2.run(h, nimg, HW, silu=True)
        sc = self.conv_shortcut.run(x1, x2) if self.conv_shortcut is not None else x1
        return self.conv2.run(h, nimg, H, W, residual=sc)


class Downsample2D(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.conv = Conv3x3(C, C, stride=2)

    def run(self, x, nimg, H, W):
        return self.conv.run(x, nimg, H, W), (H + 1) // 2, (W + 1) // 2


class Upsample2D(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.conv = Conv3x3(C, C)

    def run(self, x, nimg, H, W):
        return self.conv.run(x, nimg, H, W, upsample=True), 2 * H, 2 * W


class DownBlock(nn.Module):
    """DownBlockMotion / CrossAttnDownBlockMotion."""

    def __init__(self, cin, cout, temb, layers, cross, t_layers, heads, cross_dim, add_down, motion_heads, motion=True):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(cin if j == 0 else cout, cout, temb) for j in range(layers)])
        self.attentions = nn.ModuleList(
            [Transformer2DModel(heads, cout // heads, cout, t_layers, cross_dim) for _ in range(layers)]) if cross else None
        self.motion_modules = nn.ModuleList([MotionModule(cout, motion_heads) for _ in range(layers)]) if motion else None
        self.downsamplers = nn.ModuleList([Downsample2D(cout)]) if add_down else None

    def run(self, x, nimg, H, W, ctx):
        outs = []
        for j, res in enumerate(self.resnets):
            x = res.run(x, nimg, H, W, ctx)
            if self.attentions is not None:
                x = self.attentions[j].run(x, nimg, H, W, ctx)
            if self.motion_modules is not None:
                x = self.motion_modules[j].run(x, nimg, H, W, ctx)
            outs.append((x, H, W))
        if self.downsamplers is not None:
            x, H, W = self.downsamplers[0].run(x, nimg, H, W)
            outs.append((x, H, W))
        return x, H, W, outs


class UpBlock(nn.Module):
    """UpBlockMotion / CrossAttnUpBlockMotion."""

    def __init__(self, prev_c, cout, skip_in, temb, layers, cross, t_layers, heads, cross_dim, add_up, motion_heads,
                 motion=True):
        super().__init__()
        n = layers + 1
        self.resnets = nn.ModuleList([
            ResnetBlock2D((prev_c if j == 0 else cout) + (skip_in if j == n - 1 else cout), cout, temb)
            for j in range(n)])
        self.attentions = nn.ModuleList(
            [Transformer2DModel(heads, cout // heads, cout, t_layers, cross_dim) for _ in range(n)]) if cross else None
        self.motion_modules = nn.ModuleList([MotionModule(cout, motion_heads) for _ in range(n)]) if motion else None
        self.upsamplers = nn.ModuleList([Upsample2D(cout)]) if add_up else None

    def run(self, x, nimg, H, W, ctx, skips, stage=None):
        """`stage`: this block's index in the up path; with ctx.opts.freeu, stages 0 and 1 run apply_freeu before each
        resnet (x scaled in place: it is this path's own tensor; the skip filtered into a new one)."""
        freeu = ctx.opts.freeu if stage in (0, 1) else None
        for j, res in enumerate(self.resnets):
            s, sh, sw = skips.pop()
            assert (sh, sw) == (H, W)
            if freeu is not None:
                x, s = K.freeu(x, s, nimg, H, W, freeu.table, stage, x_out=x)
            x = res.run(x, nimg, H, W, ctx, x2=s)  # channel concat [x, skip] read from two sources
            if self.attentions is not None:
                x = self.attentions[j].run(x, nimg, H, W, ctx)
            if self.motion_modules is not None:
                x = self.motion_modules[j].run(x, nimg, H, W, ctx)
        if self.upsamplers is not None:
            x, H, W = self.upsamplers[0].run(x, nimg, H, W)
        return x, H, W


class MidBlock(nn.Module):
    """UNetMidBlockCrossAttnMotion (no motion module for the SDXL-beta adapter)."""

    def __init__(self, C, temb, t_layers, heads, cross_dim, motion, motion_heads):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(C, C, temb), ResnetBlock2D(C, C, temb)])
        self.attentions = nn.ModuleList([Transformer2DModel(heads, C // heads, C, t_layers, cross_dim)])
        self.motion_modules = nn.ModuleList([MotionModule(C, motion_heads)]) if motion else None

    def run(self, x, nimg, H, W, ctx):
        x = self.resnets[0].run(x, nimg, H, W, ctx)
        x = self.attentions[0].run(x, nimg, H, W, ctx)
        if self.motion_modules is not None:
            x = self.motion_modules[0].run(x, nimg, H, W, ctx)
        return self.resnets[1].run(x, nimg, H, W, ctx)


class TimestepEmbedding(nn.Module):
    def __init__(self, cin, T):
        super().__init__()
        self.linear_1 = Linear(cin, T)
        self.linear_2 = Linear(T, T)

    def run(self, x, residual=None):
        h = self.linear_1.run(x)
        h = K.silu(h)
        return self.linear_2.run(h, residual=residual)


@dataclass
class UNetMotionOutput:
    sample: torch.Tensor


class UNetMotionModel(nn.Module):
    def __init__(self, config: Optional[UNetMotionConfig] = None):
        super().__init__()
        cfg = config or UNetMotionConfig.sdxl()
        self.config = cfg
        ch = cfg.block_out_channels
        T = cfg.time_embed_dim
        self.conv_in = Conv3x3(cfg.in_channels, ch[0])
        self.time_embedding = TimestepEmbedding(ch[0], T)
        self.add_embedding = TimestepEmbedding(cfg.projection_class_embeddings_input_dim, T)
        self.down_blocks = nn.ModuleList()
        out_c = ch[0]
        for i, bt in enumerate(cfg.down_block_types):
            in_c, out_c = out_c, ch[i]
            self.down_blocks.append(DownBlock(in_c, out_c, T, cfg.layers_per_block, bt.startswith("CrossAttn"),
                                              cfg.transformer_layers_per_block[i], cfg.num_attention_heads[i],
                                              cfg.cross_attention_dim, i < len(ch) - 1, cfg.motion_num_attention_heads,
                                              cfg.motion_modules))
        self.mid_block = MidBlock(ch[-1], T, cfg.transformer_layers_per_block[-1], cfg.num_attention_heads[-1],
                                  cfg.cross_attention_dim, cfg.use_motion_mid_block and cfg.motion_modules,
                                  cfg.motion_num_attention_heads)
        rch = list(reversed(ch))
        rtl = list(reversed(cfg.transformer_layers_per_block))
        rheads = list(reversed(cfg.num_attention_heads))
        self.up_blocks = nn.ModuleList()
        out_c = rch[0]
        for i, bt in enumerate(cfg.up_block_types):
            prev_c, out_c = out_c, rch[i]
            skip_in = rch[min(i + 1, len(ch) - 1)]
            self.up_blocks.append(UpBlock(prev_c, out_c, skip_in, T, cfg.layers_per_block, bt.startswith("CrossAttn"),
                                          rtl[i], rheads[i], cfg.cross_attention_dim, i < len(ch) - 1,
                                          cfg.motion_num_attention_heads, cfg.motion_modules))
        self.conv_norm_out = GroupNorm(cfg.norm_num_groups, ch[0], eps=cfg.norm_eps)
        self.conv_out = Conv3x3(ch[0], cfg.out_channels)
        self.freeu = None  # enable_freeu: the default of forward()
        self.token_merging = None  # enable_token_merging: the default of forward()

    # ---- diffusers surface ----------------------------------------------------------------
    @property
    def dtype(self):
        return self.conv_in.weight.dtype

    @property
    def attn_processors(self):
        return {f"{n}.processor": m.processor for n, m in self.named_modules() if isinstance(m, Attention)}

    def set_attn_processor(self, processor):
        mods = {f"{n}.processor": m for n, m in self.named_modules() if isinstance(m, Attention)}
        if isinstance(processor, dict):
            if set(processor) != set(mods):
                raise ValueError("processor dict keys must match attn_processors")
            for k, p in processor.items():
                mods[k].set_processor(p)
        else:
            for m in mods.values():
                m.set_processor(processor)

    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float):
        """FreeU for every later forward() that is given no `freeu=` (the reference's
        unziplora_unet/unet_2d_condition.py method; the FreeU authors' SDXL values are s1=0.9, s2=0.2, b1=1.3,
        b2=1.4).  Inference only.  A second call rewrites the same device table."""
        if self.freeu is None:
            self.freeu = FreeU(s1, s2, b1, b2, device=self.conv_in.weight.device)
        else:
            self.freeu.set(s1, s2, b1, b2)

    def disable_freeu(self):
        self.freeu = None

    def enable_token_merging(self, ratio: float = 0.5, max_downsample: int = 2, sx: int = 2, sy: int = 2,
                             use_rand: bool = True, merge_attn: bool = True, merge_crossattn: bool = False,
                             merge_mlp: bool = False):
        """Token merging (tomesd.apply_patch's arguments; token_merge.TokenMerging) for every later
        forward() that is given no `token_merging=`.  Inference only."""
        self.token_merging = TokenMerging(ratio, max_downsample, sx, sy, use_rand, merge_attn, merge_crossattn,
                                          merge_mlp)

    def disable_token_merging(self):
        self.token_merging = None

    def set_ip_adapter_scale(self, scale):
        """The weight of the image term of the IP-Adapter layers (ip_adapter.load_ip_adapter): a float, or
        {attention name prefix: float} with 0 for the layers under no prefix (InstantStyle-like block selection).  A
        layer at 0 launches nothing, so a captured step must be captured again after a change."""
        from .ip_adapter import set_ip_adapter_scale
        set_ip_adapter_scale(self, scale)

    # ---- embeddings -----------------------------------------------------------------------
    def embed(self, timestep, text_embeds, time_ids, B, step_idx=None, out=None):
        """SiLU(time_embedding(Timesteps(t)) + add_embedding([text_embeds, Timesteps(time_ids)])) -> [B, T].
        `timestep`: fp32 device tensor [B] (or a schedule table with step_idx)."""
        cfg = self.config
        ch0 = cfg.block_out_channels[0]
        dev = text_embeds.device
        t_in = torch.empty(B, ch0, dtype=BF16, device=dev)
        K.timestep_embedding(timestep, B, ch0, t_in, step_idx=step_idx)
        add_in = torch.empty(B, cfg.projection_class_embeddings_input_dim, dtype=BF16, device=dev)
        K.copy2d(text_embeds, add_in[:, : cfg.text_embed_dim])
        tid = time_ids.float().reshape(-1).contiguous()
        K.timestep_embedding(tid, B * cfg.num_time_ids, cfg.addition_time_embed_dim, add_in,
                             col0=cfg.text_embed_dim, per_row=cfg.num_time_ids)
        temb = self.time_embedding.run(t_in)
        emb = self.add_embedding.run(add_in, residual=temb)  # emb = temb + aug_emb
        return K.silu(emb, out=out)

    def batched_temb(self, emb_silu):
        """time_emb_proj(SiLU(emb)) of EVERY ResnetBlock2D as one GEMM over the concatenated weights
        ([B, sum Cout], bf16-rounded like the reference's per-block Linear, then fp32 once): 17 M=2
        projections become one launch.  Returns {resnet: fp32 [B, Cout] view}."""
        res = [m for m in self.modules() if isinstance(m, ResnetBlock2D)]
        ops = build_ops([m.time_emb_proj for m in res], 1.0)
        allt = run_ops(emb_silu, ops).float()
        out, o = {}, 0
        for m in res:
            c = m.out_channels
            out[m] = allt[:, o:o + c]
            o += c
        return out

    # ---- core (NHWC tokens) -----------------------------------------------------------------
    def forward_tokens(self, x, B, F, h, w, emb_silu, enc, cross_kwargs=None, shard=None, fusion_world=None,
                       temporal_context=None, cross_frame=None, lora_gate=None, freeu=None, image_prompt=None,
                       token_merging=None, region_prompts=None, options: Optional[ForwardOptions] = None):
        """x: [B*F*h*w, in_channels] bf16 -> noise prediction [B*F*h*w, out_channels] bf16.
        With `shard` (frame_shard.FrameShard), F is this rank's frames of each clip.  `fusion_world` P (default: the
        shard's world size, else 1): take the shape-dependent fusion decisions a P-way frame-sharded rank takes
        (kernels.fusion_world), so an unsharded forward equals a P-way sharded one bit for bit.  The seven option
        keywords are ForwardOptions' fields, resolved (checked) here; None means off: the enable_freeu /
        enable_token_merging defaults are applied by forward().  Or `options`: a ForwardOptions already resolved for
        this call, in their place; it is taken as it is, nothing is checked again."""
        given = dict(temporal_context=temporal_context, cross_frame=cross_frame, lora_gate=lora_gate, freeu=freeu,
                     image_prompt=image_prompt, token_merging=token_merging, region_prompts=region_prompts)
        if options is None:
            options = ForwardOptions.resolve(self, B, F, (h, w), shard, x, use_model_defaults=False, enc=enc, **given)
        elif any(v is not None for v in given.values()):
            raise TypeError("forward_tokens: `options` holds every option of the call; no option keyword beside it")
        return self._run_tokens(x, B, F, h, w, emb_silu, enc, cross_kwargs, shard, fusion_world, options)

    def _run_tokens(self, x, B, F, h, w, emb_silu, enc, cross_kwargs, shard, fusion_world, opts: ForwardOptions):
        """forward_tokens under resolved options: launches only."""
        if fusion_world is None:
            fusion_world = shard.world if shard is not None else 1
        # no split-K: a row's bits do not depend on the launch's row count (frame shards)
        with K.row_invariant(), K.fusion_world(fusion_world):
            ctx = FwdCtx(B=B, F=F, emb_silu=emb_silu, enc=enc, cross_kwargs=cross_kwargs or {}, opts=opts, shard=shard,
                         temb=self.batched_temb(emb_silu), latent_hw=(h, w))
            nimg = B * F
            H, W = h, w
            x = self.conv_in.run(x, nimg, H, W)
            skips = [(x, H, W)]
            for blk in self.down_blocks:
                x, H, W, outs = blk.run(x, nimg, H, W, ctx)
                skips.extend(outs)
            x = self.mid_block.run(x, nimg, H, W, ctx)
            for i, blk in enumerate(self.up_blocks):
                x, H, W = blk.run(x, nimg, H, W, ctx, skips, stage=i)
            x = self.conv_norm_out.run(x, nimg, H * W, silu=True)
            return self.conv_out.run(x, nimg, H, W)

    def forward(self, sample, timestep, encoder_hidden_states, timestep_cond=None, attention_mask=None,
                cross_attention_kwargs=None, added_cond_kwargs=None, return_dict=True, frame_shard=None,
                fusion_world=None, temporal_context=None, cross_frame=None, lora_gate=None, freeu=None,
                image_prompt=None, token_merging=None, region_prompts=None, **kwargs):
        """diffusers UNetMotionModel.forward signature (inference_animatediff.py:110-121).  With
        `frame_shard` (frame_shard.FrameShard) `sample` holds this rank's frames of each clip; `fusion_world`: see
        forward_tokens; `temporal_context`, `cross_frame`, `lora_gate`, `freeu`, `image_prompt`, `token_merging`,
        `region_prompts`: the options of this call (ForwardOptions), every one refused before any launch if it cannot
        be honoured; `freeu` and `token_merging` default to what enable_freeu / enable_token_merging set.  With
        regional prompts the spatial attn2 layers attend to the regions' own text states:
        `encoder_hidden_states` gives only the shape they must share and is not read by them."""
        if not sample.is_cuda:
            raise K._lib.VstError("UNetMotionModel: sample is on CPU; the HIP path has no CPU fallback")
        B, Cin, F, h, w = sample.shape
        opts = ForwardOptions.resolve(self, B, F, (h, w), frame_shard, sample, use_model_defaults=True,
                                      temporal_context=temporal_context, cross_frame=cross_frame, lora_gate=lora_gate,
                                      freeu=freeu, image_prompt=image_prompt, token_merging=token_merging,
                                      region_prompts=region_prompts, enc=encoder_hidden_states)
        dev = sample.device
        t = timestep if torch.is_tensor(timestep) else torch.tensor([timestep])
        t = t.to(device=dev, dtype=torch.float32).reshape(-1)
        if t.numel() == 1:
            t = t.expand(B)
        t = t.contiguous()
        text_embeds = added_cond_kwargs["text_embeds"].to(dev, BF16).reshape(B, -1).contiguous()
        time_ids = added_cond_kwargs["time_ids"].to(dev).reshape(B, -1)
        emb_silu = self.embed(t, text_embeds, time_ids, B)
        enc = encoder_hidden_states.to(dev, BF16).contiguous()
        x = torch.empty(B * F * h * w, Cin, dtype=BF16, device=dev)
        K.pack_latents(sample.float().contiguous(), x)
        y = self._run_tokens(x, B, F, h, w, emb_silu, enc, cross_attention_kwargs, frame_shard, fusion_world, opts)
        out = y.view(B, F, h, w, -1).permute(0, 4, 1, 2, 3).contiguous().to(sample.dtype)
        return UNetMotionOutput(out) if return_dict else (out,)
