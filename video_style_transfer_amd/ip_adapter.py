"""IP-Adapter image prompts: decoupled attn2 over a few image tokens.

The reference carries the processor (unziplora_unet/unzip_attention_processor.py:1693-1822,
IPAdapterAttnProcessor2_0): every spatial attn2 gets a second pair of projections, to_k_ip / to_v_ip, over num_tokens
image tokens, and the image attention is added to the text attention with a scale (:1793-1809).

Here the text attention runs as it always did (the fused q + cross-attention launch, or the two-launch path) and the
image term is ONE more launch per layer, vst_ip_attention_add, which needs no q: the image keys are constants of a
clip, so they fold into the query projection,

    s[m,h,t] = scale * (q_h[m] . k_ip[b,t,h]) = scale * (x[m] . G[b,h,t] + c[b,h,t]),
    G[b,h,t,:] = k_ip[b,t,64h:64h+64] . W_eff[64h:64h+64, :],  c[b,h,t] = k_ip[b,t,64h:64h+64] . bias_q[64h:64h+64],
    W_eff = W_q + V_up . A_cat   (the UnZipLoRA delta of to_q, folded in fp32),

with x the norm2 output that attn2 reads.  G, c and the image values live in static per-layer buffers, folded outside
the step with torch; new tokens are re-folded into the same buffers (refresh_image_kv), so a captured step replays
them.  Inference only; head size 64; not together with a LoRA gate (the fold would differ per frame).
"""
from __future__ import annotations

import weakref
from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn

from . import kernels as K
from .attention_processor import AnimateDiffAttnProcessor2_0, AttnCall, Attention
from .lora_linear import build_ops, run_ops

BF16 = torch.bfloat16
F32 = torch.float32
KEY_ROWS = 16  # image-token rows per (token batch, head) of the kernel's operands


def _err(msg):
    return K._lib.VstError(msg)


# ------------------------------------------------------------------------------------------ definition
def decoupled_attention_reference(query, key, value, ip_key, ip_value, heads: int, scale: float = 1.0,
                                  round_to=None):
    """unzip_attention_processor.py:1779-1809 on plain tensors, in the dtype given (fp32 for the definition):
    query [B, N, C]; key / value [B, L, C] or None (the image term alone); ip_key / ip_value [B, T, C].  Returns
    SDPA(q, k, v) + scale * SDPA(q, k_ip, v_ip) as [B, N, C], heads of C // heads.  `round_to` (a dtype): each SDPA
    output is rounded to it and back, the reference's `.to(query.dtype)` under bf16."""
    B, N, C = query.shape
    d = C // heads

    def split(t):
        return t.reshape(B, -1, heads, d).transpose(1, 2)

    def sdpa(k, v):
        o = F.scaled_dot_product_attention(split(query), split(k), split(v), attn_mask=None, dropout_p=0.0,
                                           is_causal=False)
        o = o.transpose(1, 2).reshape(B, N, C)
        return o if round_to is None else o.to(round_to).to(o.dtype)

    ip = sdpa(ip_key, ip_value)
    if key is None:
        return scale * ip
    return sdpa(key, value) + scale * ip


def effective_query_weight(ops, dtype=F32) -> torch.Tensor:
    """[N, K1] in `dtype` (fp32): W_q plus the low-rank delta V_up . A_cat of a ProjOps, as _context_table folds
    them."""
    w = ops.w.to(dtype)
    if ops.a is None:
        return w[:, :ops.k1]
    return w[:, :ops.k1] + w[:, ops.k1:] @ ops.a.to(dtype)


def fold_image_keys(k_ip: torch.Tensor, w_eff: torch.Tensor, bias: Optional[torch.Tensor], heads: int):
    """(G [B, heads, T, K], c [B, heads, T] or None) from k_ip [B, T, heads*d], W_eff [heads*d, K] and to_q's bias
    [heads*d] or None, in k_ip's dtype: q_h . k_ip_h = x . G + c for q = x W_eff^T + bias."""
    B, T, inner = k_ip.shape
    d = inner // heads
    k = k_ip.reshape(B, T, heads, d)
    G = torch.einsum("bthd,hdk->bhtk", k, w_eff.to(k.dtype).reshape(heads, d, -1))
    c = None if bias is None else torch.einsum("bthd,hd->bht", k, bias.to(k.dtype).reshape(heads, d))
    return G, c


# ------------------------------------------------------------------------------------------ image prompt
class ImagePrompt:
    """The image tokens of a batch and their per-frame strength, in static device buffers (like lora_gate.LoraGate).
    tokens: [B, T, D] (B token batches in UNet batch order, each serving `frames` consecutive frames); strength: fp32
    [B * frames], what the image term of each frame is multiplied by (0: the frame is left alone).  set_tokens /
    set_strength write in place and bump `version`; a captured step holds the buffers' addresses."""

    def __init__(self, tokens, frames: int, strength=1.0):
        t = torch.as_tensor(tokens)
        if t.dim() != 3 or 0 in t.shape:
            raise ValueError(f"image tokens: shape {tuple(t.shape)}, expected (batches, tokens, dim)")
        if not 1 <= t.shape[1] <= KEY_ROWS:
            raise ValueError(f"image tokens: {t.shape[1]} tokens; the kernel holds 1 to {KEY_ROWS}")
        if int(frames) < 1:
            raise ValueError(f"image prompt: {frames} frames per token batch")
        self.frames = int(frames)
        self.tokens = t.detach().to(BF16).contiguous().clone()
        self.rows = t.shape[0] * self.frames
        self.strength = torch.ones(self.rows, dtype=F32, device=self.tokens.device)
        self.version = 0
        self.set_strength(strength)
        self.version = 0

    @property
    def device(self):
        return self.tokens.device

    @property
    def num_tokens(self) -> int:
        return self.tokens.shape[1]

    def set_tokens(self, tokens):
        t = torch.as_tensor(tokens)
        if tuple(t.shape) != tuple(self.tokens.shape):
            raise ValueError(f"image tokens: shape {tuple(t.shape)}, expected {tuple(self.tokens.shape)}")
        self.tokens.copy_(t.detach())
        self.version += 1
        return self

    def set_strength(self, value):
        """A scalar, (frames,) or (batches, frames); finite values."""
        B = self.tokens.shape[0]
        t = torch.as_tensor(value, dtype=F32).detach().cpu()
        if t.dim() == 0:
            t = t.expand(B, self.frames)
        elif t.dim() == 1 and t.shape[0] == self.frames:
            t = t.unsqueeze(0).expand(B, self.frames)
        elif not (t.dim() == 2 and tuple(t.shape) == (B, self.frames)):
            raise ValueError(f"image prompt strength: shape {tuple(t.shape)}, expected a scalar, ({self.frames},) or "
                             f"({B}, {self.frames})")
        if not bool(torch.isfinite(t).all()):
            raise ValueError("image prompt strength: values must be finite")
        self.strength.copy_(t.reshape(-1))
        self.version += 1
        return self


# ------------------------------------------------------------------------------------------ processor
class IPAdapterAttnProcessor2_0(nn.Module, AnimateDiffAttnProcessor2_0):
    """unzip_attention_processor.py:1693-1822 on the kernels: AnimateDiffAttnProcessor2_0's attn2 (text K/V cached per
    clip, q + cross-attention in one launch where it fits) plus vst_ip_attention_add for the image tokens.
    Called by the UNet (with an AttnCall) it takes the tokens from its `image_prompt` (ImagePrompt) and plain text
    states; called without one, as the reference is, the last num_tokens rows of encoder_hidden_states are the image
    tokens (:1767-1771).
    `scale` is the layer's weight of the image term (unet.set_ip_adapter_scale); 0 launches nothing."""

    def __init__(self, hidden_size, cross_attention_dim=None, num_tokens=4, scale=1.0):
        nn.Module.__init__(self)
        AnimateDiffAttnProcessor2_0.__init__(self)
        if not 1 <= int(num_tokens) <= KEY_ROWS:
            raise ValueError(f"IPAdapterAttnProcessor2_0: num_tokens {num_tokens}; the kernel holds 1 to {KEY_ROWS}")
        self.hidden_size = hidden_size
        self.cross_attention_dim = cross_attention_dim
        self.num_tokens = int(num_tokens)
        self.scale = scale
        self.to_k_ip = nn.Linear(cross_attention_dim or hidden_size, hidden_size, bias=False)
        self.to_v_ip = nn.Linear(cross_attention_dim or hidden_size, hidden_size, bias=False)

    def forward(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None, scale=1.0,
                _vst: Optional[AttnCall] = None, **kwargs):
        if encoder_hidden_states is None:
            raise _err("image_prompt: IPAdapterAttnProcessor2_0 is a cross-attention (attn2) processor")
        if _vst is None:
            encoder_hidden_states, prompt = self._split(encoder_hidden_states, hidden_states.shape[0])
            _vst = AttnCall(image_prompt=prompt)
        elif _vst.image_prompt is None:
            raise _err("image_prompt: IP-Adapter processors are installed and no image prompt was given")
        return AnimateDiffAttnProcessor2_0.__call__(self, attn, hidden_states, encoder_hidden_states, attention_mask,
                                                    temb, scale, _vst, **kwargs)

    def _split(self, enc, batch):
        """(text states, ImagePrompt) of concatenated states [be, L + num_tokens, D], kept per tensor object: the
        text K/V cache is keyed on tensor identity, and a fresh slice per call would never hit it."""
        if enc.dim() != 3 or enc.shape[1] <= self.num_tokens or batch % enc.shape[0]:
            raise _err(f"image_prompt: encoder_hidden_states {tuple(enc.shape)} for {self.num_tokens} image tokens "
                       f"and a batch of {batch}")
        cache = self.__dict__.setdefault("_vst_split", [])
        for ref, ver, text, prompt in cache:
            if ref() is enc and ver == enc._version:
                return text, prompt
        end = enc.shape[1] - self.num_tokens
        text = enc[:, :end].to(BF16).contiguous()
        prompt = ImagePrompt(enc[:, end:], batch // enc.shape[0])
        cache[:] = [c for c in cache if c[0]() is not None][-3:] + [(weakref.ref(enc), enc._version, text, prompt)]
        return text, prompt

    # ---- per-clip operands -------------------------------------------------------------------
    def _fold(self, prompt, q_ops, heads, bufs):
        """Project the tokens and fold the keys into the query projection, into the static buffers."""
        G, c, V = bufs
        B, T, D = prompt.tokens.shape
        inner = self.to_k_ip.out_features
        kv = run_ops(prompt.tokens.reshape(B * T, D), build_ops([self.to_k_ip, self.to_v_ip], 1.0))  # bf16
        with torch.no_grad():
            Gf, cf = fold_image_keys(kv[:, :inner].float().reshape(B, T, inner), effective_query_weight(q_ops),
                                     q_ops.bias, heads)
            G.view(B, heads, KEY_ROWS, -1)[:, :, :T].copy_(Gf)
            if c is not None:
                c.view(B, heads, KEY_ROWS)[:, :, :T].copy_(cf)
            V.view(B, KEY_ROWS, inner)[:, :T].copy_(kv[:, inner:].reshape(B, T, inner))

    def image_operands(self, prompt, q_ops, heads):
        """(G, c or None, V) of this layer for `prompt` under the query operands `q_ops`: cached on the module,
        keyed on the prompt object and its version and on the ProjOps object; a newer version is folded into the
        same buffers."""
        cache = self.__dict__.setdefault("_vst_ip_ops", [])
        for c in cache:
            if c[0]() is prompt and c[2] is q_ops:
                if c[1] != prompt.version:
                    self._fold(prompt, q_ops, heads, c[3])
                    c[1] = prompt.version
                return c[3]
        B = prompt.tokens.shape[0]
        dev = prompt.device
        bufs = (torch.zeros(B * heads * KEY_ROWS, q_ops.k1, dtype=BF16, device=dev),
                None if q_ops.bias is None else torch.zeros(B * heads * KEY_ROWS, dtype=F32, device=dev),
                torch.zeros(B * KEY_ROWS, self.to_k_ip.out_features, dtype=BF16, device=dev))
        self._fold(prompt, q_ops, heads, bufs)
        # (entries go when their prompt object does: a captured step of a live denoiser reads the buffers)
        cache[:] = [c for c in cache if c[0]() is not None] + [[weakref.ref(prompt), prompt.version, q_ops, bufs]]
        return bufs

    def _image_attention(self, attn, x, o, q_ops, batch, N, image_prompt, gate):
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            # (no backward pass of vst_ip_attention_add, and the fold is made outside autograd)
            raise NotImplementedError("image_prompt: the IP-Adapter path is inference only")
        refuse_lora_gate(image_prompt, gate)
        if image_prompt is None:
            raise _err("image_prompt: IP-Adapter processors are installed and no image prompt was given")
        heads = attn.heads
        check_image_prompt(image_prompt, batch, self.num_tokens)
        if attn.to_q.out_features != 64 * heads or self.to_k_ip.out_features != 64 * heads:
            raise _err("image_prompt: the image attention kernel is specialised for head_dim 64")
        if self.scale == 0:
            return o
        G, c, V = self.image_operands(image_prompt, q_ops, heads)
        K.ip_attention_add(x, G, c, V, o, Nq=N, heads=heads, T=self.num_tokens, kv_div=image_prompt.frames,
                           scale=64 ** -0.5, layer_scale=float(self.scale), row_scale=image_prompt.strength)
        return o


def check_image_prompt(prompt, rows: int, num_tokens: Optional[int] = None):
    if not isinstance(prompt, ImagePrompt):
        raise _err(f"image_prompt: expected an ip_adapter.ImagePrompt, got {type(prompt).__name__}")
    if prompt.rows != rows:
        raise _err(f"image_prompt: {prompt.rows} rows for a batch of {rows} images")
    if num_tokens is not None and prompt.num_tokens != num_tokens:
        raise _err(f"image_prompt: {prompt.num_tokens} image tokens; the processors were built for {num_tokens}")


def ip_processors(model) -> list:
    """[(attention name, Attention)] of the attn2 layers of `model` that carry an IP-Adapter processor."""
    return [(n, m) for n, m in model.named_modules()
            if isinstance(m, Attention) and isinstance(m.processor, IPAdapterAttnProcessor2_0)]


def refuse_lora_gate(image_prompt, lora_gate):
    """The one rule between two options: an image prompt and a LoRA gate do not go together.  Stated here only
    (ForwardOptions.resolve through check_forward, the denoiser's two setters, a direct processor call)."""
    if image_prompt is not None and lora_gate is not None:
        raise _err("image_prompt: not together with a lora_gate (the folded keys would differ per frame)")


def check_forward(model, image_prompt, rows: int, lora_gate=None):
    """Refuse, before any launch, an image prompt the model cannot honour (ForwardOptions.resolve)."""
    layers = ip_processors(model)
    if image_prompt is None:
        if layers:
            raise _err("image_prompt: IP-Adapter processors are installed and no image prompt was given")
        return
    if not layers:
        raise _err("image_prompt: the model has no IP-Adapter processors (load_ip_adapter)")
    refuse_lora_gate(image_prompt, lora_gate)
    check_image_prompt(image_prompt, rows)
    for n, m in layers:
        if m.processor.num_tokens != image_prompt.num_tokens:
            raise _err(f"image_prompt: {image_prompt.num_tokens} image tokens; {n} was built for "
                       f"{m.processor.num_tokens}")
        if m.dim_head != 64:
            raise _err(f"image_prompt: the image attention kernel is specialised for head_dim 64; {n} has "
                       f"{m.dim_head}")


def refuse_training(model):
    """The IP-Adapter path is inference only (no backward pass of vst_ip_attention_add): a training forward of a
    model that carries the processors is refused before any launch (autograd.unet_train_tokens)."""
    if ip_processors(model):
        raise NotImplementedError("image_prompt: training with IP-Adapter processors installed; the image attention "
                                  "is inference only (no backward pass)")


def refresh_image_kv(model, prompt):
    """Re-project and re-fold, into their existing buffers, the image operands that the IP-Adapter layers of `model`
    cached under an older version of `prompt` (AnimateDiffDenoiser.set_image_prompt: before a captured step is
    replayed).  Under K.row_invariant, as the forward that first projected them ran."""
    with K.row_invariant():
        for _, m in ip_processors(model):
            for c in m.processor.__dict__.get("_vst_ip_ops", ()):
                if c[0]() is prompt and c[1] != prompt.version:
                    m.processor._fold(prompt, c[2], m.heads, c[3])
                    c[1] = prompt.version


# ------------------------------------------------------------------------------------------ image projection
class ImageProjection(nn.Module):
    """diffusers ImageProjection (the encoder_hid_proj of an IP-Adapter): image_embeds Linear -> reshape to
    num_tokens x cross_attention_dim -> LayerNorm, on the GEMM and LayerNorm kernels."""

    def __init__(self, image_embed_dim: int, cross_attention_dim: int, num_tokens: int = 4):
        super().__init__()
        self.num_image_text_embeds = int(num_tokens)
        self.cross_attention_dim = int(cross_attention_dim)
        self.image_embeds = nn.Linear(image_embed_dim, self.num_image_text_embeds * cross_attention_dim)
        self.norm = nn.LayerNorm(cross_attention_dim)

    def forward(self, image_embeds: torch.Tensor) -> torch.Tensor:
        """[B, image_embed_dim] -> bf16 [B, num_tokens, cross_attention_dim]."""
        if not image_embeds.is_cuda:
            raise _err("ImageProjection: image_embeds is on CPU; the HIP path has no CPU fallback")
        x = image_embeds.to(BF16).reshape(-1, self.image_embeds.in_features).contiguous()
        B = x.shape[0]
        with K.row_invariant():
            h = run_ops(x, build_ops([self.image_embeds], 1.0))
            h = h.reshape(B * self.num_image_text_embeds, self.cross_attention_dim)
            y = K.layer_norm(h, self.norm.weight.detach().float().contiguous(),
                             self.norm.bias.detach().float().contiguous(), self.norm.eps)
        return y.view(B, self.num_image_text_embeds, self.cross_attention_dim)


# ------------------------------------------------------------------------------------------ loading
def ip_adapter_layers(unet) -> list:
    """[(processor key, Attention)] of the spatial cross-attention (attn2) layers in unet.attn_processors order: the
    layers an IP-Adapter checkpoint numbers 1, 3, 5, ..."""
    mods = {n: m for n, m in unet.named_modules() if isinstance(m, Attention)}
    out = []
    for key in unet.attn_processors:
        m = mods[key[:-len(".processor")]]
        if m.is_cross_attention and not m.temporal:
            out.append((key, m))
    return out


def load_ip_adapter(unet, state_dict_or_path, scale: float = 1.0):
    """Install an IP-Adapter: an IPAdapterAttnProcessor2_0 on every spatial attn2 and unet.encoder_hid_proj.
    The layout is the public IP-Adapter one,
        {"image_proj": {"proj.weight", "proj.bias", "norm.weight", "norm.bias"},
         "ip_adapter": {"<id>.to_k_ip.weight", "<id>.to_v_ip.weight"}},
    with <id> = 1, 3, 5, ... over the non-motion attn2 layers in unet.attn_processors order (diffusers counts the
    same way over its own attn_processors).  That this module tree enumerates the layers in diffusers' order cannot
    be checked here without diffusers and a published checkpoint: the names follow diffusers' UNetMotionModel, the
    order is named_modules' order, and a mismatch would show as shape errors only between levels of different width.
    Returns the number of layers installed."""
    sd = state_dict_or_path
    if not isinstance(sd, dict):
        sd = torch.load(sd, map_location="cpu")
    if not isinstance(sd, dict) or "image_proj" not in sd or "ip_adapter" not in sd:
        raise ValueError("load_ip_adapter: expected {'image_proj': {...}, 'ip_adapter': {...}}")
    proj, ipa = sd["image_proj"], sd["ip_adapter"]
    for k in ("proj.weight", "proj.bias", "norm.weight", "norm.bias"):
        if k not in proj:
            raise ValueError(f"load_ip_adapter: image_proj lacks {k!r}")
    layers = ip_adapter_layers(unet)
    if not layers:
        raise ValueError("load_ip_adapter: the model has no spatial cross-attention layers")
    cross = proj["norm.weight"].shape[0]
    if proj["proj.weight"].shape[0] % cross:
        raise ValueError(f"load_ip_adapter: proj.weight {tuple(proj['proj.weight'].shape)} vs norm {cross}")
    T = proj["proj.weight"].shape[0] // cross
    want = {f"{2 * i + 1}.{w}.weight" for i in range(len(layers)) for w in ("to_k_ip", "to_v_ip")}
    if set(ipa) != want:
        odd = sorted(set(ipa) ^ want)[:4]
        raise ValueError(f"load_ip_adapter: ip_adapter keys do not match the model's {len(layers)} spatial attn2 "
                         f"layers (ids 1, 3, ..., {2 * len(layers) - 1}); first differences: {odd}")
    dev = unet.conv_in.weight.device
    dtype = unet.conv_in.weight.dtype
    procs = []
    for i, (key, m) in enumerate(layers):
        p = IPAdapterAttnProcessor2_0(m.inner_dim, cross, T, scale)
        for w in ("to_k_ip", "to_v_ip"):
            src = ipa[f"{2 * i + 1}.{w}.weight"]
            lin = getattr(p, w)
            if tuple(src.shape) != tuple(lin.weight.shape):
                raise ValueError(f"load_ip_adapter: {2 * i + 1}.{w}.weight {tuple(src.shape)} for {key} "
                                 f"{tuple(lin.weight.shape)}")
            with torch.no_grad():
                lin.weight.copy_(src)
        procs.append(p.to(dev, dtype).requires_grad_(False))
    hid = ImageProjection(proj["proj.weight"].shape[1], cross, T)
    with torch.no_grad():
        hid.image_embeds.weight.copy_(proj["proj.weight"])
        hid.image_embeds.bias.copy_(proj["proj.bias"])
        hid.norm.weight.copy_(proj["norm.weight"])
        hid.norm.bias.copy_(proj["norm.bias"])
    for (key, m), p in zip(layers, procs):  # nothing is installed unless everything fits
        m.set_processor(p)
    unet.encoder_hid_proj = hid.to(dev, dtype).requires_grad_(False)
    return len(layers)


def unload_ip_adapter(unet):
    """Take the IP-Adapter off: AnimateDiffAttnProcessor2_0 back on the layers that carry an IP processor, and no
    encoder_hid_proj.  Returns the number of layers restored."""
    layers = ip_processors(unet)
    for _, m in layers:
        m.set_processor(AnimateDiffAttnProcessor2_0())
    if isinstance(getattr(unet, "encoder_hid_proj", None), ImageProjection):
        del unet.encoder_hid_proj
    return len(layers)


def set_ip_adapter_scale(unet, scale):
    """The image term's weight per layer: a float for every layer, or {name prefix: float} (layers under no prefix get
    0): style-only block selection in the manner of InstantStyle, e.g. {"up_blocks.0.attentions.1": 1.0}."""
    layers = ip_processors(unet)
    if not layers:
        raise ValueError("set_ip_adapter_scale: the model has no IP-Adapter processors (load_ip_adapter)")
    if isinstance(scale, dict):
        for pre in scale:
            if not any(n.startswith(pre) for n, _ in layers):
                raise ValueError(f"set_ip_adapter_scale: no IP-Adapter layer under {pre!r}")
        vals = [next((float(v) for pre, v in scale.items() if n.startswith(pre)), 0.0) for n, _ in layers]
    else:
        vals = [float(scale)] * len(layers)
    if not all(v == v and abs(v) != float("inf") for v in vals):
        raise ValueError("set_ip_adapter_scale: scales must be finite")
    for (_, m), v in zip(layers, vals):
        m.processor.scale = v
