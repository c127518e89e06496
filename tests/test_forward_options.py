"""ForwardOptions: the per-call options of the UNet forward, normalised and checked once (DESIGN.md "Forward
options").  CPU only: the model lives on the meta device, and everything asserted here happens before any launch.

The single-fault table's exception types and messages are those `forward_tokens` raised before ForwardOptions
existed, observed by running the same table there; `resolve` and `forward_tokens` must both still raise them."""
import dataclasses
import types

import pytest
import torch

B, FR, H, W = 2, 4, 8, 8
BF16 = torch.bfloat16


def _model(ip=False, **cfg_kw):
    from video_style_transfer_amd.config import UNetMotionConfig
    from video_style_transfer_amd.unet_motion import UNetMotionModel
    cfg = dataclasses.replace(UNetMotionConfig.tiny(), **cfg_kw)
    with torch.device("meta"):
        model = UNetMotionModel(cfg)
        if ip:
            from video_style_transfer_amd.ip_adapter import IPAdapterAttnProcessor2_0, ip_adapter_layers
            for _, m in ip_adapter_layers(model):
                m.set_processor(IPAdapterAttnProcessor2_0(m.inner_dim, cfg.cross_attention_dim, 4))
    return model.requires_grad_(False)


@pytest.fixture(scope="module")
def model():
    return _model()


def _x(F=FR):
    return torch.empty(B * F * H * W, 4, dtype=BF16, device="meta")


def _prompt(F=FR):
    from video_style_transfer_amd.ip_adapter import ImagePrompt
    return ImagePrompt(torch.zeros(B, 4, 256), F)


def _gate(rows):
    from video_style_transfer_amd.lora_gate import LoraGate
    return LoraGate(rows, "cpu")


def _cf(*a, **kw):
    from video_style_transfer_amd.unet_motion import CrossFrameAttention
    return CrossFrameAttention(*a, **kw)


def _tc(*a):
    from video_style_transfer_amd.unet_motion import TemporalContext
    return TemporalContext(*a)


def _vst_error():
    from video_style_transfer_amd._lib import VstError
    return VstError


# (name, model keywords, frames per rank, shard, the options given, exception type, message)
SINGLE_FAULTS = [
    ("cross_frame_source_past_F", {}, FR, None, lambda: dict(cross_frame=(5,)),
     _vst_error, r"cross_frame: source frame 5 >= F = 4"),
    ("cross_frame_adain_without_anchor", {}, FR, None, lambda: dict(cross_frame=_cf(("prev",), adain="qk")),
     _vst_error, r"cross_frame: adain='qk' normalises to a fixed anchor frame, and sources \('prev',\) name none"),
    ("cross_frame_sharded", {}, FR, types.SimpleNamespace(world=2), lambda: dict(cross_frame=("first",)),
     _vst_error, r"cross_frame: a source frame's keys/values live on another rank under frame sharding \(world 2\)"),
    ("clip_longer_than_table", {}, 40, None, lambda: {},
     _vst_error, r"a clip of 40 frames exceeds the motion modules' 32 positions: pass context_length"),
    ("context_longer_than_table", dict(motion_max_seq_length=16), 8, None,
     lambda: dict(temporal_context=_tc(24, 4)),
     _vst_error, r"context_length 24 exceeds the motion modules' 16 positions"),
    ("freeu_non_finite", {}, FR, None, lambda: dict(freeu=(0.9, float("inf"), 1.3, 1.4)),
     lambda: ValueError, r"freeu s2 inf must be a finite value > 0"),
    ("token_merging_not_an_option", {}, FR, None, lambda: dict(token_merging="half"),
     _vst_error, r"token_merging: 'half'; None, a TokenMerging, a dict of its fields or a ratio"),
    ("token_merging_crossattn", {}, FR, None, lambda: dict(token_merging=dict(merge_crossattn=True)),
     _vst_error, r"token_merging: merge_crossattn is not supported"),
    ("lora_gate_rows", {}, FR, None, lambda: dict(lora_gate=_gate(3)),
     _vst_error, r"lora_gate: 3 rows, expected B \* F = 8"),
    ("image_prompt_without_processors", {}, FR, None, lambda: dict(image_prompt=_prompt()),
     _vst_error, r"image_prompt: the model has no IP-Adapter processors"),
    ("image_prompt_with_lora_gate", dict(ip=True), FR, None,
     lambda: dict(image_prompt=_prompt(), lora_gate=_gate(B * FR)),
     _vst_error, r"image_prompt: not together with a lora_gate"),
]


@pytest.mark.parametrize("case", SINGLE_FAULTS, ids=[c[0] for c in SINGLE_FAULTS])
def test_single_fault_table(case):
    from video_style_transfer_amd.unet_motion import ForwardOptions
    name, model_kw, F, shard, given, exc, message = case
    model = _model(**model_kw)
    x = _x(F)
    with pytest.raises(exc(), match=message) as by_resolve:
        ForwardOptions.resolve(model, B, F, (H, W), shard, x, use_model_defaults=False, **given())
    with pytest.raises(exc(), match=message) as by_forward:
        model.forward_tokens(x, B, F, H, W, None, None, shard=shard, **given())
    assert type(by_resolve.value) is type(by_forward.value) and str(by_resolve.value) == str(by_forward.value)
    if name == "image_prompt_with_lora_gate":  # the one rule that names two options: one function states it
        assert by_resolve.traceback[-1].name == by_forward.traceback[-1].name == "refuse_lora_gate"


def test_direct_processor_call_with_both_refuses_through_the_shared_function():
    from video_style_transfer_amd.ip_adapter import IPAdapterAttnProcessor2_0
    proc = IPAdapterAttnProcessor2_0(64, 256, 4).requires_grad_(False)
    with pytest.raises(_vst_error(), match="image_prompt: not together with a lora_gate") as e:
        proc._image_attention(None, torch.zeros(1), None, None, B * FR, H * W, _prompt(), _gate(B * FR))
    assert e.traceback[-1].name == "refuse_lora_gate"


def test_model_defaults(model, monkeypatch):
    from video_style_transfer_amd.unet_motion import ForwardOptions, UNetMotionModel
    model.enable_freeu(0.9, 0.2, 1.3, 1.4)
    model.enable_token_merging(ratio=0.25, use_rand=False)
    try:
        def resolve(defaults, **given):
            return ForwardOptions.resolve(model, B, FR, (H, W), None, _x(), use_model_defaults=defaults, **given)
        on = resolve(True)
        assert on.freeu is model.freeu and on.token_merging is model.token_merging
        assert on == ForwardOptions(freeu=model.freeu, token_merging=model.token_merging)
        off = resolve(False)
        assert off == ForwardOptions() and off.freeu is None and off.token_merging is None
        explicit = resolve(True, freeu=(1.0, 1.0, 1.1, 1.2), token_merging=0.5)
        assert explicit.freeu is not model.freeu and explicit.freeu.values == (1.0, 1.0, 1.1, 1.2)
        assert explicit.token_merging is not model.token_merging and explicit.token_merging.ratio == 0.5
        # forward_tokens is the "None means off" caller
        seen = []
        monkeypatch.setattr(UNetMotionModel, "_run_tokens", lambda self, *a: seen.append(a[-1]))
        model.forward_tokens(_x(), B, FR, H, W, None, None)
        assert seen == [ForwardOptions()]
    finally:
        model.disable_freeu()
        model.disable_token_merging()


def test_resolve_normalises(model):
    from video_style_transfer_amd.freeu import FreeU
    from video_style_transfer_amd.token_merge import TokenMerging
    from video_style_transfer_amd.unet_motion import CrossFrameAttention, ForwardOptions
    tc, gate = _tc(2, 1), _gate(B * FR)
    o = ForwardOptions.resolve(model, B, FR, (H, W), None, _x(), use_model_defaults=False, temporal_context=tc,
                               cross_frame="first", lora_gate=gate, freeu=(0.9, 0.2, 1.3, 1.4),
                               token_merging=dict(ratio=0.5, use_rand=False))
    assert o.temporal_context is tc and o.lora_gate is gate and o.image_prompt is None
    assert o.cross_frame == CrossFrameAttention(("first",))
    assert isinstance(o.freeu, FreeU) and isinstance(o.token_merging, TokenMerging)
    with pytest.raises(dataclasses.FrozenInstanceError):
        o.freeu = None
    with pytest.raises(TypeError, match="cross_frames"):   # a misspelt option is not swallowed
        ForwardOptions.resolve(model, B, FR, (H, W), use_model_defaults=False, cross_frames="first")
    with pytest.raises(TypeError, match="options"):
        model.forward_tokens(_x(), B, FR, H, W, None, None, options=o, cross_frame="first")


def test_one_check_per_call(model, monkeypatch):
    from video_style_transfer_amd import ip_adapter, unet_motion
    from video_style_transfer_amd.unet_motion import ForwardOptions, UNetMotionModel
    counts = {}

    def counted(mod, name):
        inner = getattr(mod, name)

        def f(*a, **kw):
            counts[name] = counts.get(name, 0) + 1
            return inner(*a, **kw)
        monkeypatch.setattr(mod, name, f)

    checks = ("check_forward", "check_cross_frame", "as_freeu", "check_token_merging", "check_clip_length")
    counted(ip_adapter, "check_forward")
    for name in checks[1:]:
        counted(unet_motion, name)
    given = dict(cross_frame=("first",), freeu=(0.9, 0.2, 1.3, 1.4), token_merging=0.5, temporal_context=_tc(2, 1),
                 lora_gate=_gate(B * FR))
    opts = ForwardOptions.resolve(model, B, FR, (H, W), None, _x(), use_model_defaults=False, **given)
    assert counts == dict.fromkeys(checks, 1)
    ran = []
    monkeypatch.setattr(UNetMotionModel, "_run_tokens", lambda self, *a: ran.append(a[-1]))
    model.forward_tokens(_x(), B, FR, H, W, None, None, options=opts)
    assert ran == [opts] and ran[0] is opts
    assert counts == dict.fromkeys(checks, 1)          # an instance in hand is never checked again
    model.forward_tokens(_x(), B, FR, H, W, None, None, **given)
    assert counts == dict.fromkeys(checks, 2)          # without one: once per call
    assert ran[1].freeu.values == opts.freeu.values    # (each resolve of a tuple makes its own FreeU)
    assert dataclasses.replace(ran[1], freeu=None) == dataclasses.replace(opts, freeu=None)
