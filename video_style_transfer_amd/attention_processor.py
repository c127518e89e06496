"""Attention module + processors — the plug-in surface the reference swaps.

* `Attention`: the attributes/methods diffusers' Attention exposes to processors
  (heads, to_q/to_k/to_v/to_out, norm_cross, spatial_norm, group_norm, residual_connection,
  rescale_output_factor, prepare_attention_mask, set_processor/processor).
* `AnimateDiffAttnProcessor2_0`: same call signature and semantics as
  animatediff/attention_processor.py:18-96 (spatial self/cross attention of UNetMotionModel,
  text states repeat_interleave'd to B*F, LoRA `scale` forwarded to the projections only when
  to_q has a lora_layer).  Kernel mapping: self-attn q/k/v -> ONE fused GEMM (UnZipLoRA delta
  as augmented K), SDPA -> vst_spatial_attention, to_out -> GEMM with the block residual fused
  in the epilogue.  Cross-attn K/V are projected once per clip (not per frame) and indexed by
  frame // F inside the attention kernel.
* `AttnProcessor2_0`: the default processor the reference leaves on motion modules
  (inference_animatediff.py:211-215): frame-axis self-attention -> vst_temporal_attention.

Hidden-state layout.  Spatial: (B*F, H*W, C).  Motion: the reference/diffusers permute to
(B*H*W, F, C); our blocks keep (B*F, H*W, C) and pass the frame count (`AttnCall.frames`; a caller
without an AttnCall passes `num_frames=F`), the kernel reads the frame axis with stride H*W.  Both
layouts are accepted by AttnProcessor2_0 (given neither, the input is taken as (batch, seq=F, C),
the diffusers layout).
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn

from . import kernels as K
from .lora_linear import LoRACompatibleLinear, build_ops, gate_operands, run_ops
from .region_prompts import refuse_lora_gate as refuse_region_gate


@dataclass
class AttnCall:
    """What the UNet's blocks hand a processor beside diffusers' arguments, as the one keyword `_vst` (DESIGN.md
    §23).  A processor called without it is being called the diffusers way: ip_adapter's then finds the image tokens
    at the end of encoder_hidden_states, AttnProcessor2_0 takes the (B*HW, F, C) layout unless given `num_frames`."""
    residual: Optional[torch.Tensor] = None  # the block's residual, added in to_out's epilogue
    lora_u: Optional[torch.Tensor] = None    # x @ Acat^T of the q(/k/v) ops, from K.layer_norm_lora
    frames: Optional[int] = None             # frames per clip, where the attention reads the frame axis
    cross_frame: Optional[object] = None     # attn1 only: an active unet_motion.CrossFrameAttention (needs `frames`)
    lora_gate: Optional[object] = None       # lora_gate.LoraGate, one row per image of the batch
    image_prompt: Optional[object] = None    # attn2 only: ip_adapter.ImagePrompt
    regions: Optional[tuple] = None          # attn2 only: (region_prompts.RegionPrompts, this level's fp32 weight table)
    context: Optional[tuple] = None          # motion modules: (TemporalContext, fp32 PE table); the input carries no PE


_NO_CALL = AttnCall()

class Attention(nn.Module):
    def __init__(self, query_dim: int, cross_attention_dim: Optional[int] = None, heads: int = 8,
                 dim_head: int = 64, bias: bool = False, out_bias: bool = True, processor=None,
                 temporal: bool = False):
        super().__init__()
        inner = heads * dim_head
        kv_dim = cross_attention_dim if cross_attention_dim is not None else query_dim
        self.heads = heads
        self.dim_head = dim_head
        self.inner_dim = inner
        self.is_cross_attention = cross_attention_dim is not None
        self.scale = dim_head ** -0.5
        self.to_q = LoRACompatibleLinear(query_dim, inner, bias=bias)
        self.to_k = LoRACompatibleLinear(kv_dim, inner, bias=bias)
        self.to_v = LoRACompatibleLinear(kv_dim, inner, bias=bias)
        self.to_out = nn.ModuleList([LoRACompatibleLinear(inner, query_dim, bias=out_bias), nn.Dropout(0.0)])
        self.norm_cross = None
        self.spatial_norm = None
        self.group_norm = None
        self.residual_connection = False
        self.rescale_output_factor = 1.0
        self.temporal = temporal
        self.processor = processor if processor is not None else (
            AttnProcessor2_0() if temporal else AnimateDiffAttnProcessor2_0())

    def set_processor(self, processor):
        # (a processor that is an nn.Module, ip_adapter's, registers as a child; a plain one replacing it must not)
        if "processor" in self._modules and not isinstance(processor, nn.Module):
            del self._modules["processor"]
        self.processor = processor

    def get_processor(self):
        return self.processor

    def prepare_attention_mask(self, attention_mask, target_length, batch_size, out_dim=3):
        raise NotImplementedError("attention masks are not used on the AnimateDiff-XL denoise path")

    def norm_encoder_hidden_states(self, encoder_hidden_states):
        raise NotImplementedError("norm_cross is None for SDXL attention")

    def forward(self, hidden_states, encoder_hidden_states=None, attention_mask=None, **cross_attention_kwargs):
        return self.processor(self, hidden_states, encoder_hidden_states=encoder_hidden_states,
                              attention_mask=attention_mask, **cross_attention_kwargs)


def _proj_scale(attn, scale):
    # attention_processor.py:54 — LoRA scale only reaches layers that have a lora_layer
    return scale if hasattr(attn.to_q, "lora_layer") else 1.0


def _finish(attn, out, residual_for_flag):
    if attn.residual_connection:
        out = out + residual_for_flag
    if attn.rescale_output_factor != 1.0:
        out = out / attn.rescale_output_factor
    return out


class AnimateDiffAttnProcessor2_0:
    """animatediff/attention_processor.py:6-96, kernel-backed.  With `_vst.regions` (regional prompts, DESIGN.md
    §24) attn2 attends to the regions' own text states and does not read encoder_hidden_states (it must still be
    given: it is what makes the call a cross-attention)."""

    def __init__(self):
        if not hasattr(F, "scaled_dot_product_attention"):
            raise ImportError("AnimateDiffAttnProcessor2_0 requires PyTorch 2.0+.")

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None, scale=1.0,
                 _vst: Optional[AttnCall] = None, **kwargs):
        call = _vst if _vst is not None else _NO_CALL
        lora_u, cf, gate = call.lora_u, call.cross_frame, call.lora_gate
        if gate is not None and gate.rows != hidden_states.shape[0]:
            raise K._lib.VstError(f"LoRA gate: {gate.rows} rows for a batch of {hidden_states.shape[0]} images")
        if attn.spatial_norm is not None or attn.group_norm is not None or attn.norm_cross:
            raise NotImplementedError("spatial_norm/group_norm/norm_cross are inert for SDXL (attention_processor.py:30-60)")
        if attention_mask is not None:
            raise NotImplementedError("attention_mask is None on the reference path (attention_processor.py:46-48)")
        input_ndim = hidden_states.ndim
        if input_ndim == 4:  # (B, C, H, W) -> tokens (attention_processor.py:34-36)
            b4, c4, h4, w4 = hidden_states.shape
            hidden_states = hidden_states.reshape(b4, c4, h4 * w4).transpose(1, 2).contiguous()
        batch, N, C = hidden_states.shape
        s = _proj_scale(attn, scale)
        heads, inner = attn.heads, attn.to_q.out_features
        hd = inner // heads
        x = hidden_states.reshape(batch * N, C)
        if encoder_hidden_states is None:
            if cf is not None and hd != 64:
                raise K._lib.VstError("cross_frame: the cross-frame attention kernel is specialised for head_dim 64")
            qkv = run_ops(x, build_ops([attn.to_q, attn.to_k, attn.to_v], s), u=lora_u, gate=gate)
            if cf is not None:
                # the frame's own tokens plus those of the source frames of the same clip, read in place
                Fr = call.frames
                if cf.adain is not None:
                    # StyleAligned: q | k (| v) normalised per column to the anchor frame's statistics, in place
                    K.frame_adain(qkv[:, :cf.adain_blocks * inner], batch // Fr, Fr, N, cf.anchor)
                o = K.spatial_attention_frames(qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:],
                                               batch // Fr, Fr, heads, N, cf.sources, scale=hd ** -0.5)
            elif hd == 64:
                o = K.spatial_attention(qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:], batch, heads, N,
                                        N, 1, scale=hd ** -0.5)
            else:
                o = _generic_attention(qkv, batch, heads, N)
        else:
            enc = encoder_hidden_states
            be, L, D = enc.shape
            if batch % be:
                raise ValueError(f"encoder batch {be} does not divide hidden batch {batch}")
            q_ops = build_ops([attn.to_q], s)
            regions = call.regions
            if regions is not None:
                # regional prompts: the text K/V are those of the regions' own states, projected once
                # per clip through the same cache; encoder_hidden_states is not read
                refuse_region_gate(regions[0], gate)
                kv, L, kv_div = _text_kv(attn, regions[0].states_rows, s), regions[0].L, regions[0].frames
            else:
                # (with a gate the text K/V carry each frame's own gates: one block per image, kv_div 1)
                kv = _text_kv(attn, enc, s, gate)
                kv_div = batch // (kv.shape[0] // L)
            if hd != 64:
                raise NotImplementedError("spatial cross-attention kernel is specialised for head_dim 64 (SDXL)")
            if regions is not None:
                # q is its own launch (the fused q + cross-attention steps aside), then one attention per live region,
                # blended per row with this level's weights
                q = run_ops(x, q_ops, u=lora_u)
                o = K.region_attention(q, kv[:, :inner], kv[:, inner:], regions[1], nimg=batch, heads=heads, Nq=N,
                                       Nk=L, R=regions[0].R, kv_div=kv_div, scale=hd ** -0.5)
            elif lora_u is None and _cross_fusable(q_ops, batch * N, N, L):
                # q projection (+ in-GEMM UnZipLoRA) and the text cross-attention as one launch: q stays on chip
                g, gdiv = gate_operands(q_ops, gate, batch * N)
                o = K.linear_cross_attention(x, q_ops.w, q_ops.a, q_ops.gn, q_ops.gr, q_ops.bias, kv[:, :inner],
                                             kv[:, inner:], Nq=N, Nk=L, kv_div=kv_div, scale=hd ** -0.5,
                                             r_alg=q_ops.r, gate=g, gate_div=gdiv)
            else:
                q = run_ops(x, q_ops, u=lora_u, gate=gate)
                o = K.spatial_attention(q, kv[:, :inner], kv[:, inner:], batch, heads, N, L, kv_div,
                                        scale=hd ** -0.5)
            o = self._image_attention(attn, x, o, q_ops, batch, N, call.image_prompt, gate)
        res2d = None if call.residual is None else call.residual.reshape(batch * N, -1)
        out = run_ops(o, build_ops([attn.to_out[0]], s), residual=res2d, gate=gate)
        out = out.view(batch, N, -1)
        if input_ndim == 4:
            out = out.transpose(-1, -2).reshape(b4, c4, h4, w4)
        return _finish(attn, out, hidden_states)

    def _image_attention(self, attn, x, o, q_ops, batch, N, image_prompt, gate):
        """What a processor adds to the text attention's output o ahead of to_out (ip_adapter's processor: the image
        attention); here nothing, and an image prompt has no projections to go through."""
        if image_prompt is not None:
            raise K._lib.VstError("image_prompt: this attention has no IP-Adapter processor (load_ip_adapter)")
        return o


def _cross_fusable(ops, M: int, Nq: int, Nk: int) -> bool:
    """attn2's q projection ops (as build_ops made them) and the cross-attention fit vst_gemm_cross_attention."""
    lora = ops.a is not None
    if lora and ops.gn <= 0:
        return False
    return K.cross_attention_fusable(M, ops.n, ops.k1, lora, 0 if not lora else ops.a.shape[0], ops.gn, ops.gr, Nq, Nk)


def input_lora_ops(attn, self_attention: bool, scale: float = 1.0):
    """The projection operands AnimateDiffAttnProcessor2_0 will apply to this attention's hidden states
    (q/k/v for self-attention, q for cross-attention), or None when another processor is installed.
    Lets the producer of the hidden states (the block's LayerNorm) emit the LoRA down-projection."""
    if not isinstance(attn.processor, AnimateDiffAttnProcessor2_0):
        return None
    s = _proj_scale(attn, scale)
    return build_ops([attn.to_q, attn.to_k, attn.to_v] if self_attention else [attn.to_q], s)


def _text_kv_gated(attn, enc, ops, gate):
    """_text_kv under a LoRA gate: every image's text K/V ([gate.rows * L, 2 inner], gate row per L text rows), from
    the repeated text rows the gate keeps for all layers.  Cached per (text, operands, gate object); when the gate's
    values have changed since, the projection is redone into the SAME buffer (a captured step holds it)."""
    import weakref
    cache = attn.__dict__.setdefault("_vst_text_kv_gated", [])
    for c in cache:
        ref, ver, ops_c, gref, kv = c[:5]
        if ref() is enc and ver == enc._version and ops_c is ops and gref() is gate:
            if c[5] != gate.version:
                run_ops(gate.text_rows(enc), ops, out=kv, gate=gate)
                c[5] = gate.version
            return kv
    kv = run_ops(gate.text_rows(enc), ops, gate=gate)
    # (entries go when their text or their gate object does: a captured step of a live denoiser reads kv)
    live = [c for c in cache if c[0]() is not None and c[3]() is not None]
    cache[:] = live + [[weakref.ref(enc), enc._version, ops, weakref.ref(gate), kv, gate.version]]
    return kv


def refresh_text_kv(model, gate):
    """Re-project, into their existing buffers, the gated text K/V that the attn2 layers of `model` cached under
    older values of `gate` (AnimateDiffDenoiser.set_lora_gates: before a captured step is replayed).  Under
    K.row_invariant, as the forward that first projected them ran: without it these small GEMMs may split K and
    round differently."""
    with K.row_invariant():
        for m in model.modules():
            for c in m.__dict__.get("_vst_text_kv_gated", ()):
                enc = c[0]()
                if enc is not None and c[3]() is gate and c[5] != gate.version and c[1] == enc._version:
                    run_ops(gate.text_rows(enc), c[2], out=c[4], gate=gate)
                    c[5] = gate.version


def _text_kv(attn, enc, s, gate=None):
    """Cross-attention K/V of the text states (to_k/to_v + LoRA on encoder_hidden_states).

    They depend only on the prompt and the weights, not on the latents, so across the 50 denoise
    steps of a clip they are projected once: cached on the module and keyed on the text tensor
    object (weakref + in-place version) and on the projection operands (build_ops is itself keyed
    on the parameter versions, LoRA scale and mode).  Inside a captured step graph the cached
    buffer is simply read.  A few texts are kept (the two CFG branches run as separate calls on two streams,
    pipeline.py), oldest dropped first."""
    import weakref
    ops = build_ops([attn.to_k, attn.to_v], s)
    if gate is not None and (ops.gated or ops.folded):  # (folded: run_ops refuses the gate)
        return _text_kv_gated(attn, enc, ops, gate)
    cache = attn.__dict__.setdefault("_vst_text_kv", [])
    for ref, ver, ops_c, kv in cache:
        if ref() is enc and ver == enc._version and ops_c is ops:
            return kv
    be, L, D = enc.shape
    kv = run_ops(enc.reshape(be * L, D), ops)
    cache[:] = [c for c in cache if c[0]() is not None][-3:] + [(weakref.ref(enc), enc._version, ops, kv)]
    return kv


def _generic_attention(qkv, batch, heads, N):
    raise NotImplementedError("spatial self-attention kernel is specialised for head_dim 64 (SDXL)")


def _tattn_enabled() -> bool:
    """VST_TATTN=0 keeps the motion attention as q/k/v GEMM + vst_temporal_attention (A/B)."""
    return os.environ.get("VST_TATTN", "1") != "0"


def _tattn_operands(attn, ops, heads, head_dim):
    """The fused q/k/v weight re-laid out per pair of heads for vst_gemm_temporal_attention, cached on the module
    against the fused operand it was made from (build_ops caches that one per parameter version; trained weights get
    a fresh operand, hence a fresh layout, every call)."""
    c = attn.__dict__.get("_vst_tattn")
    if c is None or c[0] is not ops:
        c = (ops,) + K.temporal_qkv_layout(ops.w, ops.bias, heads, head_dim)
        attn.__dict__["_vst_tattn"] = c
    return c[1], c[2]


def _context_table(attn, ops, pe, length):
    """fp32 [length, 3C] = pe[:length] @ Wqkv^T (LoRA factors included, bias not): what the positional term adds to
    q/k/v by linearity, so the windowed kernel adds it per window position behind ONE projection per frame.  Cached on
    the module against the fused operand it was made from, like _tattn_operands."""
    c = attn.__dict__.get("_vst_window_pos")
    if c is None or c[0] is not ops or c[1] != length or c[2] != pe.data_ptr():
        with torch.no_grad():
            w = ops.w.float()
            p = pe[:length].float()
            t = p @ w[:, :ops.k1].t()
            if ops.a is not None:
                t = t + (p @ ops.a.float().t()) @ w[:, ops.k1:].t()
        c = (ops, length, pe.data_ptr(), t.contiguous())
        attn.__dict__["_vst_window_pos"] = c
    return c[3]


class AttnProcessor2_0:
    """Default (motion-module) processor: self-attention along the frame axis."""

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None,
                 num_frames: Optional[int] = None, _vst: Optional[AttnCall] = None, **kwargs):
        call = _vst if _vst is not None else AttnCall(frames=num_frames)
        num_frames, context = call.frames, call.context
        if encoder_hidden_states is not None or attention_mask is not None:
            raise NotImplementedError("motion-module attention is self-attention without mask")
        batch, N, C = hidden_states.shape
        if num_frames is not None:  # our layout: (B*F, HW, C)
            nclip, Fr, HW = batch // num_frames, num_frames, N
        else:  # diffusers layout: (B*HW, F, C)
            nclip, Fr, HW = batch, N, 1
        heads = attn.heads
        inner = attn.to_q.out_features
        D = inner // heads
        x = hidden_states.reshape(batch * N, C)
        ops = build_ops([attn.to_q, attn.to_k, attn.to_v], 1.0)
        # (HW % (16 P) under K.fusion_world(P): a P-way all-to-all rank holds HW / P pixels and fuses only when that
        # is a multiple of 16, so the unsharded forward it is compared with decides the same way)
        if context is not None:
            # a clip longer than the context: one projection per frame, then the frame attention inside sliding
            # windows with the positional term added per window position (vst_temporal_attention_windowed); the fused
            # q/k/v + attention GEMM steps aside (its epilogue attends over whole 16-frame clips)
            tc, pe = context
            qkv = run_ops(x, ops)
            o = K.temporal_attention_windowed(qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:],
                                              _context_table(attn, ops, pe, tc.length), nclip, Fr, HW, heads, D,
                                              tc.length, tc.stride, tc.weighting)
        elif num_frames is not None and _tattn_enabled() and ops.a is None and ops.w.shape[1] == C and \
                HW % (16 * K.fusion_pixel_div()) == 0 and \
                K.temporal_attention_fusable(batch * N, C, nclip, Fr, HW, heads, D):
            # q/k/v projection + frame attention in one launch (vst_gemm_temporal_attention; 16 frames, heads of 40)
            w_t, b_t = _tattn_operands(attn, ops, heads, D)
            o = K.linear_temporal_attention(x, w_t, b_t, nclip=nclip, F=Fr, HW=HW, heads=heads, head_dim=D,
                                            scale=D ** -0.5)
        else:
            qkv = run_ops(x, ops)
            o = K.temporal_attention(qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:], nclip, Fr, HW,
                                     heads, D)
        res2d = None if call.residual is None else call.residual.reshape(batch * N, -1)
        out = run_ops(o, build_ops([attn.to_out[0]], 1.0), residual=res2d).view(batch, N, -1)
        return _finish(attn, out, hidden_states)
