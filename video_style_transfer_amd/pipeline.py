"""The denoise loop of `generate_video` (inference_animatediff.py:53-151), MI355X-native.

Per step the reference does: scale_model_input -> unet(uncond) -> unet(cond) -> CFG combine ->
Euler step (two B=1 UNet calls, :109-121).  Here one step is:
  vst_pack_latents (scale_model_input, both CFG branches, NHWC bf16)
  -> embed (timestep read from the device schedule table)
  -> ONE UNet forward over the CFG-batched B=2 clip (results identical to two B=1 calls: no op mixes
     batch elements)
  -> vst_euler_cfg_step (CFG combine + Euler update of the fp32 latents)
  -> vst_step_advance (device step counter).
Because every per-step scalar lives in device tables indexed by the device counter, the whole step
is captured once into a HIP graph and replayed for all 50 steps (no per-launch host overhead).
Latents stay fp32 on the device (the reference keeps them in the UNet dtype between steps).
With sampler="dpmpp_2m" or guidance_rescale > 0 the update is vst_sampler_step instead, after
vst_cfg_rescale_factor when rescaling: its coefficients, its history and the rescale factor live on the device too.
The stochastic samplers ("euler_a", "dpmpp_2m_sde", "lcm") step with vst_sampler_step_noise: the fresh
noise of every step is counter-based, a function of a device seed and the device step counter, so the captured step
still replays unchanged.
With free_init= a call runs the loop num_iters times; between two passes vst_free_init_mix re-noises the
result with the run's initial noise, keeps its low spatio-temporal frequencies and takes the high ones from fresh
counter-based noise.  The mix runs between passes, outside the step, so the captured step replays untouched.
With token_merging= the spatial transformer blocks merge tokens around attn1 (and the feed-forward); the
plans live in static buffers and the destination draw reads the device seed and step counter, so the step still replays.
With set_region_prompts every spatial attn2 blends up to four prompts per pixel (vst_region_attention);
the states and the per-level weight tables are static buffers, so new masks replay the captured step.
"""
from __future__ import annotations

from typing import Optional

import math

import torch

from . import kernels as K
from .attention_processor import refresh_text_kv
from .free_init import FreeInit, as_free_init, check_free_init_arg, check_free_init_run, dft_order, freq_filter
from .freeu import FreeU, as_freeu, check_freeu_arg
from .ip_adapter import ImagePrompt, check_forward, refresh_image_kv, refuse_lora_gate
from .lora_gate import LoraGate
from .region_prompts import MAX_MASKS, RegionPrompts, attention_levels, region_weights
from .region_prompts import refuse_lora_gate as refuse_region_gate
from .token_merge import TokenMerging, as_token_merging, check_token_merging
from .scheduler import (SAMPLERS, STOCHASTIC_SAMPLERS, EulerDiscreteScheduler, check_eta, sampler_coefficients,
                        start_index)
from .unet_motion import TemporalContext, UNetMotionModel, as_cross_frame, check_clip_length, check_cross_frame

BF16 = torch.bfloat16


def check_sampler(sampler, guidance_scale, guidance_rescale, shard=None, eta=1.0, scheduler=None) -> float:
    """The sampler arguments of AnimateDiffDenoiser, refused here before anything is allocated.  Returns
    guidance_rescale as a float.  `eta` must be finite and >= 0; "lcm" steps on the LCM timesteps, so a `scheduler`
    given with it must have timestep_spacing "lcm"."""
    if sampler not in SAMPLERS:
        raise ValueError(f"sampler {sampler!r}: one of {SAMPLERS}")
    check_eta(eta)
    if sampler == "lcm" and scheduler is not None and scheduler.timestep_spacing != "lcm":
        raise ValueError(f"sampler 'lcm' needs EulerDiscreteScheduler(timestep_spacing='lcm'), got spacing "
                         f"{scheduler.timestep_spacing!r}")
    try:
        phi = float(guidance_rescale)
    except (TypeError, ValueError):
        raise ValueError(f"guidance_rescale {guidance_rescale!r} is not a number") from None
    if not (math.isfinite(phi) and 0.0 <= phi <= 1.0):
        raise ValueError(f"guidance_rescale {guidance_rescale} must be a finite value in [0, 1]")
    if phi > 0.0:
        if not guidance_scale > 1.0:
            raise ValueError(f"guidance_rescale {phi} rescales the guided noise against the cond branch: it needs "
                             f"classifier-free guidance (guidance_scale > 1, got {guidance_scale})")
        if shard is not None and shard.world > 1:
            raise ValueError("guidance_rescale takes the std over whole clips; under a frame shard of world "
                             f"{shard.world} the other ranks hold part of every clip")
    return phi


class AnimateDiffDenoiser:
    def __init__(self, unet: UNetMotionModel, num_frames: int, height: int, width: int, *,
                 num_inference_steps: int = 50, guidance_scale: float = 7.5, device=None,
                 scheduler: Optional[EulerDiscreteScheduler] = None, use_graph: bool = True, shard=None,
                 num_clips: int = 1, context_length: Optional[int] = None, context_stride: int = 4,
                 context_weighting: str = "pyramid", cross_frame=None, sampler: str = "euler",
                 guidance_rescale: float = 0.0, eta: float = 1.0, freeu=None, free_init=None,
                 token_merging=None):
        """`num_clips` clips are denoised together (the reference loop is one clip, B=1).
        `shard` (frame_shard.FrameShard): this process denoises frames [f0, f0 + F/P) of every clip and
        exchanges with the other ranks inside every motion module.
        The CFG branches always run as ONE batched B=2 forward on one stream (running them as two B=1 chains on two
        forked streams measured slower, 76.6 vs 72.8 ms per step, profiles/r3_ab_cfg_streams.txt; removed).
        `context_length` (with `context_stride`, `context_weighting`): clips of more than context_length frames run
        their motion modules inside sliding windows of that many frames (unet_motion.TemporalContext, DESIGN.md "Long
        clips"); without it a clip longer than the motion modules' positional table is refused here.
        `cross_frame` (e.g. ("first",) or ("first", "prev"); unet_motion.CrossFrameAttention, DESIGN.md "Cross-frame
        spatial self-attention"): every frame's spatial self-attention also attends to those frames of its clip.  It
        is static, so a captured step replays it unchanged.
        `sampler` "euler" or "dpmpp_2m" (second-order multistep, DPM-Solver++ 2M; meant for 20-25 steps on
        EulerDiscreteScheduler(sigma_schedule="karras")) and `guidance_rescale` in [0, 1] (rescale_noise_cfg of the
        reference's pipeline; needs CFG and whole clips on this rank) are fixed at construction.
        With "euler" and 0 the step is the one it always was.
        `sampler` "euler_a", "dpmpp_2m_sde" or "lcm"  adds fresh noise at every step, scaled by `eta`
        (finite, >= 0; 0 is the deterministic sampler; "lcm" ignores it).  The noise is a function of the noise seed
        (set_noise_seed, or the `seed` of a call), the step and the element's place in the whole clip, so a frame
        shard draws what the whole clip draws.  "lcm" (4-8 steps, guidance_scale 1) needs a scheduler with
        timestep_spacing "lcm" and builds one when none is given.
        `freeu` (a freeu.FreeU or its (s1, s2, b1, b2), each finite and > 0): FreeU in the UNet's first
        two up blocks, the reference's enable_freeu.  None takes what unet.enable_freeu set, if anything, as it stands
        now.  It is per frame and per channel, so it composes with every other option, a frame shard included; the
        values live in a device table, so set_freeu keeps a captured step.
        `free_init` (a free_init.FreeInit, a dict of its fields or its tuple): FreeInit, diffusers'
        enable_free_init.  A call (`__call__`) then runs the whole loop num_iters times, with the frequency mix of
        kernels.free_init_mix between two passes.  It transforms whole clips, so a frame shard of more than one rank
        is refused, and so is a source run; num_iters 1 or None is the plain run, launch for launch.
        `token_merging` (a token_merge.TokenMerging, a dict of its fields or a ratio): token merging in
        the spatial transformer blocks, tomesd's apply_patch.  None takes what unet.enable_token_merging set, if
        anything.  With use_rand the destination pattern is drawn from the noise seed (set_noise_seed, or the `seed` of
        a call) and the device step counter, so it changes per step under replay; ratio 0 is the plain step."""
        self.guidance_rescale = check_sampler(sampler, guidance_scale, guidance_rescale, shard, eta, scheduler)
        check_freeu_arg(freeu)
        check_free_init_arg(free_init)
        check_free_init_run(free_init, shard)
        if unet is None:  # refused with the other arguments, before anything is allocated
            raise ValueError("AnimateDiffDenoiser needs a UNetMotionModel, got None")
        self.sampler = sampler
        self.eta = float(eta)
        self.noise_step = sampler in STOCHASTIC_SAMPLERS
        self.context = None if context_length is None else TemporalContext(int(context_length), int(context_stride),
                                                                           context_weighting)
        if unet.config.motion_modules:
            check_clip_length(num_frames, unet.config.motion_max_seq_length, self.context)
        self.cross_frame = as_cross_frame(cross_frame)
        check_cross_frame(unet, num_frames, self.cross_frame, shard, (height // 8, width // 8))
        self.unet = unet
        self.nclips = num_clips
        self.shard = shard
        self.F_total = num_frames
        self.F, self.f0 = shard.local_frames(num_frames) if shard is not None else (num_frames, 0)
        self.h, self.w = height // 8, width // 8
        self.height, self.width = height, width
        self.guidance = guidance_scale
        self.cfg = guidance_scale > 1.0
        self.ncopy = 2 if self.cfg else 1
        self.device = torch.device(device or "cuda")
        self.freeu = getattr(unet, "freeu", None) if freeu is None else as_freeu(freeu, self.device)
        self.scheduler = scheduler or EulerDiscreteScheduler(**({"timestep_spacing": "lcm"} if sampler == "lcm"
                                                                else {}))
        self.scheduler.set_timesteps(num_inference_steps, device=self.device)
        self.num_steps = num_inference_steps
        self.use_graph = use_graph
        cfg = unet.config
        dev = self.device
        self.lat = torch.zeros(num_clips, cfg.in_channels, self.F, self.h, self.w, dtype=torch.float32, device=dev)
        self.x = torch.empty(self.ncopy * num_clips * self.F * self.h * self.w, cfg.in_channels, dtype=BF16,
                             device=dev)
        self.step_idx = torch.zeros(1, dtype=torch.int32, device=dev)
        self.timesteps = self.scheduler.timesteps.to(dev, torch.float32).contiguous()
        self.sigmas = self.scheduler.sigmas.to(dev, torch.float32).contiguous()
        self.enc = None
        self.graph = None
        # video-to-video state (set_source): the first step of the run, and the static device buffers of the source
        # latents, their noise and the keep mask (allocated on first use, never reallocated: a captured step holds
        # their pointers)
        self.t_start = 0
        self.steps_run = 0  # steps since the run was entered (host side; run_steps' default finishes the schedule)
        self.src = self.eps = self.mask = None
        self.masked = False
        # per-frame content / style strength (set_lora_gates): None = the plain step
        self.lora_gate = None
        # IP-Adapter image prompt (set_image_prompt): None = the plain step
        self.image_prompt = None
        # regional prompts (set_region_prompts): None = the plain step; the regions' embeds as given, for a later
        # set_prompt_embeds
        self.region_prompts = None
        self._region_embeds = None
        # table-driven sampler step: the previous step's denoised estimate, the (a, b, c) rows, the
        # per-clip rescale factor and its workspace; allocated here once, a captured step holds their pointers.  A
        # stochastic sampler (§16) has (a, b, c, d) rows and the seed of its noise, rewritten in place.
        self.table_step = sampler != "euler" or self.guidance_rescale > 0.0
        self.hist = self.coef = self.factor = self.rescale_ws = self.noise_seed = None
        if self.table_step:
            self.hist = torch.zeros_like(self.lat)
            self.coef = torch.empty(num_inference_steps, 4 if self.noise_step else 3, dtype=torch.float32, device=dev)
            if self.noise_step:
                self.noise_seed = torch.zeros(1, dtype=torch.int64, device=dev)
            self._write_coef(0)
            if self.guidance_rescale > 0.0:
                self.factor = torch.ones(num_clips, dtype=torch.float32, device=dev)
                self.rescale_ws = K.cfg_rescale_workspace(self.lat.shape, dev)
        # token merging: refused here, before anything is captured; its destination draw reads the
        # sampler's noise seed where there is one, else a seed of its own, and this denoiser's step counter
        self.token_merging = self.tm_seed = None
        self._set_token_merging(getattr(unet, "token_merging", None) if token_merging is None
                                else as_token_merging(token_merging))
        # FreeInit: the latents the run was entered with, the mask in DFT order, the seed and the
        # counter of the fresh noise and the spectrum workspace; static device buffers, allocated when it is turned on
        self.free_init = None
        self.fi_init = self.fi_filt = self.fi_seed = self.fi_iter = self.fi_ws = None
        if free_init is not None:
            self._set_free_init(as_free_init(free_init))

    def set_prompt_embeds(self, cond_embeds, cond_pooled, uncond_embeds=None, uncond_pooled=None):
        """(1 or num_clips, L, D) text states and (1 or num_clips, P) pooled embeds per branch
        (encode_prompt output).  UNet batch order: [uncond clips..., cond clips...]."""
        dev = self.device
        n = self.nclips

        def per_clip(t):
            return t if t is None or t.shape[0] == n else t.expand(n, *t.shape[1:])
        cond_embeds, cond_pooled = per_clip(cond_embeds), per_clip(cond_pooled)
        uncond_embeds, uncond_pooled = per_clip(uncond_embeds), per_clip(uncond_pooled)
        if self.cfg:
            enc = torch.cat([uncond_embeds, cond_embeds], 0)
            pooled = torch.cat([uncond_pooled, cond_pooled], 0)
        else:
            enc, pooled = cond_embeds, cond_pooled
        enc = enc.to(dev, BF16).contiguous()
        if self.region_prompts is not None:  # region 0 is this prompt: refused before anything is replaced
            self.region_prompts.set_states(self._region_states(enc, self._region_embeds))
        self.enc = enc
        self.pooled = pooled.to(dev, BF16).contiguous()
        # SDXL time ids (inference_animatediff.py:81-85)
        tid = torch.tensor([self.height, self.width, 0, 0, self.height, self.width], dtype=torch.float32)
        self.time_ids = tid.unsqueeze(0).repeat(self.ncopy * n, 1).to(dev).contiguous()
        self.graph = None

    def _options(self) -> dict:
        """The per-call options as they stand now, by ForwardOptions' field names: the one place that maps this
        object's attributes to them.  The forward resolves (and so checks) them, once per call."""
        return dict(temporal_context=self.context, cross_frame=self.cross_frame, lora_gate=self.lora_gate,
                    freeu=self.freeu, image_prompt=self.image_prompt, token_merging=self.token_merging,
                    region_prompts=self.region_prompts)

    def _step(self):
        B = self.ncopy * self.nclips
        K.pack_latents(self.lat, self.x, sigmas=self.sigmas, step_idx=self.step_idx, ncopy=self.ncopy)
        emb = self.unet.embed(self.timesteps, self.pooled, self.time_ids, B, step_idx=self.step_idx)
        noise = self.unet.forward_tokens(self.x, B, self.F, self.h, self.w, emb, self.enc, shard=self.shard,
                                         **self._options())
        if self.table_step:
            if self.factor is not None:
                K.cfg_rescale_factor(noise, self.lat.shape, guidance=self.guidance, phi=self.guidance_rescale,
                                     out=self.factor, workspace=self.rescale_ws)
            src, eps, mask = (self.src, self.eps, self.mask) if self.masked else (None, None, None)
            kw = dict(guidance=self.guidance, ncopy=self.ncopy, factor=self.factor, z0=src, eps=eps, mask=mask)
            if self.noise_step:
                K.sampler_step_noise(noise, self.lat, self.hist, self.sigmas, self.coef, self.step_idx,
                                     self.noise_seed, F_total=self.F_total, f0=self.f0, **kw)
            else:
                K.sampler_step(noise, self.lat, self.hist, self.sigmas, self.coef, self.step_idx, **kw)
        elif self.masked:
            K.euler_cfg_step_masked(noise, self.lat, self.sigmas, self.step_idx, self.src, self.eps, self.mask,
                                    guidance=self.guidance, ncopy=self.ncopy)
        else:
            K.euler_cfg_step(noise, self.lat, self.sigmas, self.step_idx, guidance=self.guidance, ncopy=self.ncopy)
        K.step_advance(self.step_idx, self.num_steps)

    def capture(self):
        """Warm up (fills every derived-weight cache), then capture one step into a HIP graph.  Frame-sharded over
        several ranks: piecewise (frame_shard.PiecewiseGraph), the graphs split at the collectives, which run between
        them.  The latents and the step counter are put back afterwards, so a run entered part-way (set_source)
        starts where it was set; so is the sampler's history, which the warm-up step overwrites (a run interrupted
        by run_steps(k) and recaptured goes on from the history it had)."""
        saved = self.lat.clone()
        saved_hist = None if self.hist is None else self.hist.clone()
        saved_step = self.step_idx.clone()
        s = torch.cuda.Stream(device=self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            self.step_idx.zero_()
            self._step()
        torch.cuda.current_stream(self.device).wait_stream(s)
        if self.shard is not None and self.shard.world > 1:
            from .frame_shard import PiecewiseGraph
            self.graph = PiecewiseGraph().capture(self._step, [self.shard], s)
        else:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._step()
            self.graph = g
        self.lat.copy_(saved)
        if saved_hist is not None:
            self.hist.copy_(saved_hist)
        self.step_idx.copy_(saved_step)

    def _write_coef(self, first_step: int):
        """Rewrite the coefficient table in place for a run entered at `first_step` (first order there: no history)."""
        if self.coef is not None:
            self.coef.copy_(sampler_coefficients(self.scheduler.sigmas, self.sampler, first_step, self.eta,
                                                 self.scheduler.timesteps).to(torch.float32))

    def set_noise_seed(self, seed: int):
        """The seed of a stochastic sampler's step noise (any integer, taken modulo 2^64), written in place on the
        device: a captured step replays with the new seed.  The noise has no other state, so the same seed from the
        same latents is the same run."""
        if self.noise_seed is None:
            raise ValueError(f"sampler {self.sampler!r} adds no noise: one of {STOCHASTIC_SAMPLERS} takes a seed")
        v = int(seed) & (2 ** 64 - 1)
        self.noise_seed.fill_(v - 2 ** 64 if v >= 2 ** 63 else v)  # the same 64 bits as an int64

    def _set_masked(self, on: bool):
        if on != self.masked:  # another Euler kernel: the captured step no longer fits
            self.masked = on
            self.graph = None

    def _local(self, t, axis, name):
        """Whole-clip or local-frame tensor -> this rank's frames along `axis`."""
        if t.shape[axis] == self.F_total and self.F != self.F_total:
            t = t.narrow(axis, self.f0, self.F)
        if t.shape[axis] != self.F:
            raise ValueError(f"{name}: {t.shape[axis]} frames, expected {self.F_total} (whole clip) or {self.F}")
        return t

    def _gate_rows(self, value, name):
        """A gate argument -> fp32 CPU [ncopy * num_clips * F_local] in UNet batch order (both CFG copies alike)."""
        t = torch.as_tensor(value, dtype=torch.float32).detach().cpu()
        if t.dim() == 0:
            t = t.expand(self.nclips, self.F)
        elif t.dim() == 1:
            t = self._local(t, 0, f"{name} gate").unsqueeze(0).expand(self.nclips, self.F)
        elif t.dim() == 2 and t.shape[0] == self.nclips:
            t = self._local(t, 1, f"{name} gate")
        else:
            raise ValueError(f"{name} gate: shape {tuple(t.shape)}, expected a scalar, ({self.F_total},), "
                             f"({self.nclips}, {self.F_total}) or ({self.nclips}, {self.F})")
        if not bool(torch.isfinite(t).all()):
            raise ValueError(f"{name} gate: values must be finite")
        return t.unsqueeze(0).expand(self.ncopy, self.nclips, self.F).reshape(-1)

    def set_lora_gates(self, content=1.0, style=1.0):
        """Per-frame strength of the content and the style term of the UnZipLoRA delta.  Each is a
        scalar, (F_total,), (num_clips, F_total) or this rank's (num_clips, F_local); any finite value (1 = as
        trained, 0 = the term removed, above 1 over-drives, negative subtracts).  Both CFG branches of a clip use the
        same gates.  Under forward type "both" the gated terms are the merger-weighted ones, so content 1 / style 0
        is not set_forward("content"), which drops the merger.
        The first call drops a captured step (the gated step runs other kernels); later calls rewrite the gate
        tables in place, re-project the text K/V of every attn2 into their buffers, and keep it, so a schedule can
        be driven from the host: run_steps(k), set_lora_gates(...), run_steps()."""
        refuse_lora_gate(self.image_prompt, True)  # (True: the gate this call would make)
        refuse_region_gate(self.region_prompts, True)
        c = self._gate_rows(content, "content")
        s = self._gate_rows(style, "style")
        if self.lora_gate is None:
            self.lora_gate = LoraGate(self.ncopy * self.nclips * self.F, self.device)
            self.graph = None
        self.lora_gate.set(c, s)
        refresh_text_kv(self.unet, self.lora_gate)

    def _image_tokens(self, embeds, tokens, name):
        """One branch's image tokens, bf16 [num_clips, T, D] on the device: `tokens` as given, else `embeds` through
        unet.encoder_hid_proj (ip_adapter.ImageProjection)."""
        if tokens is None:
            proj = getattr(self.unet, "encoder_hid_proj", None)
            if proj is None:
                raise ValueError(f"{name}: image embeds need unet.encoder_hid_proj (load_ip_adapter); pass tokens=")
            e = torch.as_tensor(embeds).to(self.device, BF16)
            if e.dim() != 2 or e.shape[0] not in (1, self.nclips):
                raise ValueError(f"{name}: image embeds {tuple(e.shape)}, expected (1 or {self.nclips}, dim)")
            tokens = proj(e)
        t = torch.as_tensor(tokens).to(self.device, BF16)
        if t.dim() != 3 or t.shape[0] not in (1, self.nclips):
            raise ValueError(f"{name}: image tokens {tuple(t.shape)}, expected (1 or {self.nclips}, tokens, dim)")
        return t.expand(self.nclips, *t.shape[1:])

    def set_image_prompt(self, image_embeds=None, *, tokens=None, negative_image_embeds=None, negative_tokens=None,
                         strength=1.0):
        """The image prompt of an IP-Adapter (ip_adapter.load_ip_adapter).  `image_embeds` (1 or
        num_clips, dim) go through unet.encoder_hid_proj; `tokens` (1 or num_clips, T, D) are taken as they are (the
        16 tokens of a "plus" Resampler, say).  The uncond branch of CFG takes `negative_tokens`, else
        `negative_image_embeds`, else zero embeds through the projection, as diffusers does; without the projection
        it needs `negative_tokens`.  Batch order [uncond clips..., cond clips...], like set_prompt_embeds.
        `strength`: what the image term of each frame is multiplied by, in the forms set_lora_gates takes (a scalar,
        (F_total,), (num_clips, F_total) or this rank's (num_clips, F_local)); 0 leaves a frame alone.
        The first call drops a captured step; later calls rewrite the token and strength buffers in place, re-fold
        the image keys of every layer into their buffers and keep it.  Not together with set_lora_gates."""
        if (image_embeds is None) == (tokens is None):
            raise ValueError("set_image_prompt: give image_embeds or tokens (one of them)")
        refuse_lora_gate(True, self.lora_gate)  # (True: the prompt this call would make)
        cond = self._image_tokens(image_embeds, tokens, "set_image_prompt")
        if self.cfg:
            if negative_tokens is None and negative_image_embeds is None:
                if getattr(self.unet, "encoder_hid_proj", None) is None:
                    raise ValueError("set_image_prompt: CFG needs negative_tokens when the model has no "
                                     "encoder_hid_proj")
                negative_image_embeds = torch.zeros(1, self.unet.encoder_hid_proj.image_embeds.in_features,
                                                    dtype=BF16, device=self.device)
            neg = self._image_tokens(negative_image_embeds, negative_tokens, "set_image_prompt (negative)")
            if neg.shape != cond.shape:
                raise ValueError(f"set_image_prompt: negative tokens {tuple(neg.shape)} vs {tuple(cond.shape)}")
            cond = torch.cat([neg, cond], 0)
        rows = self._gate_rows(strength, "image prompt strength")
        p = self.image_prompt
        if p is None or tuple(p.tokens.shape) != tuple(cond.shape):
            p = ImagePrompt(cond, self.F, rows.view(cond.shape[0], self.F))
            check_forward(self.unet, p, self.ncopy * self.nclips * self.F, None)  # before it replaces anything
            self.image_prompt = p
            self.graph = None
        else:
            p.set_tokens(cond)
            p.set_strength(rows.view(cond.shape[0], self.F))
            refresh_image_kv(self.unet, p)

    def clear_image_prompt(self):
        """Back to the plain step (drops a captured step with the image attention).  The IP-Adapter processors, if
        still installed, refuse a forward without a prompt: take them off with ip_adapter.unload_ip_adapter."""
        if self.image_prompt is not None:
            self.image_prompt = None
            self.graph = None

    def _region_states(self, enc, embeds):
        """[ncopy * num_clips, 1 + n, L, D] in UNet batch order from the prompt states `enc` and the regions' embeds
        [n, L, D]: a cond clip has its prompt in slot 0 and the regions' after it, an uncond clip its own (uncond)
        states in every slot."""
        n = self.nclips
        if tuple(embeds.shape[1:]) != tuple(enc.shape[1:]):
            raise ValueError(f"region prompts: embeds of {tuple(embeds.shape[1:])} per region, prompt states of "
                             f"{tuple(enc.shape[1:])}")
        R = 1 + embeds.shape[0]
        cond = torch.cat([enc[-n:].unsqueeze(1), embeds.to(enc).unsqueeze(0).expand(n, *embeds.shape)], 1)
        if not self.cfg:
            return cond
        return torch.cat([enc[:n].unsqueeze(1).expand(n, R, *enc.shape[1:]), cond], 0)

    def set_region_prompts(self, embeds, masks, *, base_mask=None):
        """Regional prompts: `embeds` (n, L, D), the text states of n <= 3 further prompts, and
        `masks` (n, F_total | F_local | 1, h, w), bool or float in [0, 1], where each applies, at latent resolution.
        Region 0 is the prompt of set_prompt_embeds (call it first) with weight max(1 - sum of the masks, 0), or
        `base_mask` (frames, h, w) when given; per pixel the weights are normalised, so overlapping masks share.  Maps
        that are constant in space and vary over the frames are a prompt schedule.  Every clip of the batch takes
        the same regions.  The pooled embeds and the time ids stay the global prompt's.  The uncond branch of CFG
        attends to the uncond states alone (weights (1, 0, 0, 0): the other slots are skipped).
        The first call, another n, or other embeds drop a captured step; new masks with the same embeds rewrite
        the weight tables in place and keep it.  Not together with set_lora_gates.  While regions are on, the spatial
        attn2 layers do not read the plain prompt states."""
        refuse_region_gate(True, self.lora_gate)  # (True: the prompts this call would make)
        if self.enc is None:
            raise ValueError("set_region_prompts: region 0 is the prompt of set_prompt_embeds; call that first")
        e = torch.as_tensor(embeds)
        if e.dim() != 3 or not 1 <= e.shape[0] <= MAX_MASKS:
            raise ValueError(f"set_region_prompts: embeds {tuple(e.shape)}, expected (1 to {MAX_MASKS}, L, D)")
        m = torch.as_tensor(masks)
        if m.dim() != 4 or m.shape[0] != e.shape[0]:
            raise ValueError(f"set_region_prompts: masks {tuple(m.shape)} for {e.shape[0]} embeds, expected "
                             f"({e.shape[0]}, frames, {self.h}, {self.w})")
        frames = max([self.F if t.shape[-3] == 1 else t.shape[-3]
                      for t in (m,) + (() if base_mask is None else (torch.as_tensor(base_mask),))])
        raw = self._local(region_weights(m, frames, (self.h, self.w), base_mask), 0, "region masks")
        states = self._region_states(self.enc, e.to(self.device, BF16))
        R, n = states.shape[1], self.nclips
        rows = raw.unsqueeze(0).expand(n, *raw.shape)
        if self.cfg:
            base_only = torch.zeros_like(rows)
            base_only[:, :, 0] = 1.0
            rows = torch.cat([base_only, rows], 0)
        rows = rows.reshape(-1, R, self.h, self.w)
        rp = self.region_prompts
        if rp is None or rp.R != R:
            self.region_prompts = RegionPrompts(states, rows, self.F, attention_levels(self.unet, (self.h, self.w)),
                                                self.device)
            self.graph = None
        else:
            rp.set_weights(rows)
            if not torch.equal(rp.states, states):
                rp.set_states(states)
                self.graph = None
        self._region_embeds = e.detach().to(self.device, BF16).clone()

    def clear_region_prompts(self):
        """Back to the plain step (drops a captured step with the regional attention)."""
        if self.region_prompts is not None:
            self.region_prompts = self._region_embeds = None
            self.graph = None

    def set_ip_adapter_scale(self, scale):
        """unet.set_ip_adapter_scale, dropping a captured step (the scales are launch arguments, and a layer at 0
        launches nothing)."""
        self.unet.set_ip_adapter_scale(scale)
        self.graph = None

    def set_freeu(self, s1: float, s2: float, b1: float, b2: float):
        """FreeU values for the steps that follow.  When FreeU is already on, its device table is rewritten in place
        and a captured step is kept (it replays with the new values); turning it on drops the captured step, which
        has no FreeU launches."""
        if self.freeu is None:
            self.freeu = FreeU(s1, s2, b1, b2, device=self.device)
            self.graph = None
        else:
            self.freeu.set(s1, s2, b1, b2)

    def clear_freeu(self):
        """Back to the plain step (drops a captured step with FreeU)."""
        if self.freeu is not None:
            self.freeu = None
            self.graph = None

    def _set_token_merging(self, tm: Optional[TokenMerging]):
        check_token_merging(self.unet, tm, (self.h, self.w))
        if tm is not None and tm.use_rand:
            if self.tm_seed is None:
                self.tm_seed = self.noise_seed if self.noise_seed is not None else torch.zeros(
                    1, dtype=torch.int64, device=self.device)
            tm.bind(self.tm_seed, self.step_idx)
        self.token_merging = tm
        self.graph = None

    def enable_token_merging(self, ratio: float = 0.5, max_downsample: int = 2, sx: int = 2, sy: int = 2,
                             use_rand: bool = True, merge_attn: bool = True, merge_crossattn: bool = False,
                             merge_mlp: bool = False):
        """tomesd.apply_patch's arguments for the steps that follow (token_merge.TokenMerging).  Drops a
        captured step: the merged blocks run other launches."""
        self._set_token_merging(TokenMerging(ratio, max_downsample, sx, sy, use_rand, merge_attn, merge_crossattn,
                                             merge_mlp))

    def disable_token_merging(self):
        """Back to the plain step (drops a captured step with merged blocks)."""
        if self.token_merging is not None:
            self._set_token_merging(None)

    def _set_free_init(self, fi: FreeInit):
        check_free_init_run(fi, self.shard)
        F, h, w = self.lat.shape[2:]
        if max(F, h, w) > K.FREE_INIT_MAX_AXIS:
            raise ValueError(f"free_init: a clip of {F} x {h} x {w} latents; the frequency mix takes at most "
                             f"{K.FREE_INIT_MAX_AXIS} per axis")
        filt = dft_order(freq_filter(F, h, w, fi)).to(torch.float32)
        if self.fi_init is None:
            dev = self.device
            self.fi_init = self.lat.clone()
            self.fi_filt = torch.empty(F, h, w, dtype=torch.float32, device=dev)
            self.fi_seed = torch.zeros(1, dtype=torch.int64, device=dev)
            self.fi_iter = torch.zeros(1, dtype=torch.int32, device=dev)
            self.fi_ws = K.free_init_workspace(self.lat.shape, dev)
        self.fi_filt.copy_(filt)
        self.free_init = fi

    def enable_free_init(self, num_iters: int = 3, use_fast_sampling: bool = False, method: str = "butterworth",
                         order: int = 4, spatial_stop_frequency: float = 0.25,
                         temporal_stop_frequency: float = 0.25):
        """diffusers' enable_free_init for the calls that follow (free_init.FreeInit).  The mix runs
        between the passes of a call, so a captured step is kept.  `use_fast_sampling` (fewer steps in the early
        passes) is refused: the step count is part of the captured step."""
        if use_fast_sampling:
            raise ValueError("free_init use_fast_sampling: the number of steps is fixed at construction (the captured "
                             "step wraps its counter at num_inference_steps)")
        self._set_free_init(FreeInit(num_iters, method, order, spatial_stop_frequency, temporal_stop_frequency))

    def disable_free_init(self):
        """Back to one pass per call (the buffers stay; a captured step is kept)."""
        self.free_init = None

    def clear_lora_gates(self):
        """Back to the plain step (drops a captured gated step)."""
        if self.lora_gate is not None:
            self.lora_gate = None
            self.graph = None

    def set_source(self, latents, strength: float, mask=None, seed: int = 42):
        """Start from a source clip instead of noise (SDEdit / img2img; DESIGN.md "Video-to-video").
        latents: the source z0, (num_clips, C, F_total, h, w) or this rank's (num_clips, C, F_local, h, w), already
        times scaling_factor (AutoencoderKL.encode_frames).  The run enters the schedule at
        t_start = scheduler.start_index(num_steps, strength) with lat = z0 + sigmas[t_start] * eps,
        eps = randn(whole clip, CPU generator(seed)) as init_latents draws it (no init_noise_sigma factor).
        mask: optional keep mask (1 or num_clips, F_total or F_local, h, w) in [0, 1] over the channels; 1 = free to
        change, 0 = keep the source: after every Euler update lat = m * lat + (1 - m) * (z0 + sigmas[i + 1] * eps).
        A new strength, source or mask values reuse a captured step; adding or removing the mask drops it."""
        check_free_init_run(self.free_init, source=True)
        t_start = start_index(self.num_steps, strength)
        C = self.lat.shape[1]
        z0 = torch.as_tensor(latents)
        if z0.dim() != 5 or z0.shape[0] != self.nclips or z0.shape[1] != C or tuple(z0.shape[3:]) != (self.h, self.w):
            raise ValueError(f"source latents {tuple(z0.shape)}, expected ({self.nclips}, {C}, {self.F_total} or "
                             f"{self.F}, {self.h}, {self.w})")
        z0 = self._local(z0, 2, "source latents").to(self.device, torch.float32)
        m = None
        if mask is not None:
            m = torch.as_tensor(mask)
            if m.dim() != 4 or m.shape[0] not in (1, self.nclips) or tuple(m.shape[2:]) != (self.h, self.w):
                raise ValueError(f"mask {tuple(m.shape)}, expected (1 or {self.nclips}, {self.F_total} or {self.F}, "
                                 f"{self.h}, {self.w})")
            m = self._local(m, 1, "mask").to(self.device, torch.float32)
            if not bool(((m >= 0) & (m <= 1)).all()):
                raise ValueError("mask values must lie in [0, 1]")
        g = torch.Generator(device="cpu").manual_seed(seed)
        eps = torch.randn((self.nclips, C, self.F_total, self.h, self.w), generator=g)
        eps = eps[:, :, self.f0:self.f0 + self.F]
        if self.src is None:
            self.src, self.eps = torch.empty_like(self.lat), torch.empty_like(self.lat)
        self.src.copy_(z0)
        self.eps.copy_(eps)
        if m is not None:
            if self.mask is None:
                self.mask = torch.empty(self.nclips, self.F, self.h, self.w, dtype=torch.float32, device=self.device)
            self.mask.copy_(m.expand_as(self.mask))
        self._set_masked(m is not None)
        self.t_start = t_start
        self.steps_run = 0
        self.step_idx.fill_(t_start)
        self._write_coef(t_start)
        K.noise_latents(self.src, self.eps, self.sigmas, self.step_idx, out=self.lat)

    def set_latents(self, latents):
        """latents: (num_clips, C, F_total, h, w) for whole clips (this rank keeps its frames) or
        (num_clips, C, F_local, h, w)."""
        lat = latents.to(self.device, torch.float32)
        if lat.dim() == 5 and lat.shape[2] == self.F_total and self.F != self.F_total:
            lat = lat[:, :, self.f0:self.f0 + self.F]
        self.lat.copy_(lat.reshape(self.lat.shape))
        if self.free_init is not None:
            self.fi_init.copy_(self.lat)  # z_init: what every later pass is re-noised with
        self._restart()
        self._set_masked(False)

    def _restart(self):
        """The step counter, the run bookkeeping and the coefficient table (first order at step 0, so the sampler's
        history is not read there) as a run from the top of the schedule finds them."""
        self.step_idx.zero_()
        self.t_start = 0
        self.steps_run = 0
        self._write_coef(0)

    def init_latents(self, seed: int = 42):
        """randn((1,4,F,h,w), generator=seed) * init_noise_sigma (inference_animatediff.py:88-95); with
        frame sharding every rank draws the whole clip and keeps its frames."""
        g = torch.Generator(device="cpu").manual_seed(seed)
        shape = (self.nclips, self.lat.shape[1], self.F_total, self.h, self.w)
        lat = torch.randn(shape, generator=g) * self.scheduler.init_noise_sigma
        self.set_latents(lat)
        return lat

    def run_steps(self, n: Optional[int] = None):
        """n steps from where the counter stands.  Default: to the end of the schedule, which is num_steps - t_start
        steps after set_latents / init_latents / set_source and what is left of them after run_steps(k) (so
        run_steps(k), set_lora_gates(...), run_steps() is one whole run)."""
        total = self.num_steps - self.t_start
        n = total - self.steps_run % total if n is None else n
        self.steps_run += n
        if self.use_graph and self.graph is None:
            self.capture()
        for _ in range(n):
            if self.graph is not None:
                self.graph.replay()
            else:
                self._step()
        return self.lat

    def __call__(self, latents=None, seed: int = 42, *, source=None, strength: Optional[float] = None, mask=None,
                 content_scale=None, style_scale=None):
        """Plain run from `latents` (or from noise drawn with `seed`), or, with `source` and `strength` (and an
        optional keep `mask`), a video-to-video run (set_source).  `content_scale` / `style_scale`: set_lora_gates
        for this and later runs (the one not given is 1).  `seed` is also the noise seed of a stochastic sampler, and
        of FreeInit's fresh noise (stream 1 of the same counters, so the two are independent).  With free_init on the
        loop runs num_iters times: before pass i >= 1 the latents become free_init_mix(lat, z_init, filter,
        init_noise_sigma) at noise counter i - 1 and the run restarts from the top of the schedule; the captured step
        is not recaptured."""
        fi = self.free_init
        check_free_init_run(fi, self.shard, source is not None)
        if self.noise_seed is not None:
            self.set_noise_seed(seed)
        elif self.tm_seed is not None:
            v = int(seed) & (2 ** 64 - 1)
            self.tm_seed.fill_(v - 2 ** 64 if v >= 2 ** 63 else v)  # the same 64 bits as an int64
        if content_scale is not None or style_scale is not None:
            self.set_lora_gates(1.0 if content_scale is None else content_scale,
                                1.0 if style_scale is None else style_scale)
        if source is not None:
            if latents is not None or strength is None:
                raise ValueError("a source run takes `source` and `strength`, and no `latents`")
            self.set_source(source, strength, mask, seed)
        elif strength is not None or mask is not None:
            raise ValueError("`strength` and `mask` need a `source`")
        elif latents is None:
            self.init_latents(seed)
        else:
            self.set_latents(latents)
        self.run_steps()
        if fi is not None and fi.num_iters > 1:
            v = int(seed) & (2 ** 64 - 1)
            self.fi_seed.fill_(v - 2 ** 64 if v >= 2 ** 63 else v)  # the same 64 bits as an int64
            for i in range(1, fi.num_iters):
                self.fi_iter.fill_(i - 1)
                K.free_init_mix(self.lat, self.fi_init, self.fi_filt, float(self.scheduler.init_noise_sigma),
                                seed=self.fi_seed, it=self.fi_iter, stream_id=1, out=self.lat, workspace=self.fi_ws)
                self._restart()
                if self.hist is not None:
                    self.hist.zero_()
                self.run_steps()
        return self.lat

    def decode(self, vae) -> torch.Tensor:
        """inference_animatediff.py:137-144 for the frames this rank holds: latents / scaling_factor -> VAE decode ->
        uint8 (clips * F_local, 8h, 8w, 3) on the device.  Frame-sharded runs decode their own frames (no exchange);
        the frames of a clip are decoded together instead of one vae.decode call per frame."""
        return torch.cat([vae.decode_to_frames(self.lat[c:c + 1]) for c in range(self.lat.shape[0])])
