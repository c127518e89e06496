"""CPU tests: the wrappers of kernels.py refuse a bad operand on the host, before the library is touched.

Every pointer a wrapper hands to the library has passed a validator (DESIGN.md "Entry points").  Here the library call
is replaced by a recorder and the operands are CPU tensors that claim to be on the device (test_host.fake_device_tensor),
so nothing can launch: each bad operand must raise VstError naming the wrapper and the argument with the recorder
untouched, and the same call with the operand corrected must reach the recorder exactly once.
"""
import pytest
import torch

from test_host import fake_device_tensor as dev

BF16, F32, I32, I64 = torch.bfloat16, torch.float32, torch.int32, torch.int64


def host(*shape, dtype=BF16):
    return torch.zeros(*shape, dtype=dtype)


def vec(n, dtype=F32):
    return dev(n, dtype=dtype)


def cols(t, C):
    return t[:, :C], t[:, C:2 * C], t[:, 2 * C:]


@pytest.fixture
def K(monkeypatch):
    from video_style_transfer_amd import kernels
    calls = []
    monkeypatch.setattr(kernels._lib, "call", lambda name, *args: calls.append((name, args)) or 0)
    monkeypatch.setattr(kernels, "_stream", lambda: 0)
    monkeypatch.setattr(kernels, "_workspace", lambda device: dev(4, dtype=F32))
    kernels.calls = calls
    yield kernels
    del kernels.calls


# wrapper -> (run(K, operands), good operands, {label: (argument, bad operand)}); rows 32 = a 2 x 4 x 4 image, C = 64
def _qkv():
    q, k, v = cols(dev(32, 192), 64)
    return dict(q=q, k=k, v=v)


def _short(i):  # operand i of a [16, 192] buffer: the same row stride, half the rows
    return lambda: cols(dev(16, 192), 64)[i]


WRAPPERS = {
    "group_norm": (
        lambda K, o: K.group_norm(o["x1"], 2, 16, 32, 1e-5, o["gamma"], o["beta"], x2=o["x2"]),
        lambda: dict(x1=dev(32, 64), x2=dev(32, 128)[:, 32:96], gamma=vec(128), beta=vec(128)),
        {"host gamma": ("gamma", lambda: host(128, dtype=F32)), "host beta": ("beta", lambda: host(128, dtype=F32)),
         "bf16 gamma": ("gamma", lambda: vec(128, BF16)), "short x2": ("x2", lambda: dev(16, 64))}),
    "layer_norm": (
        lambda K, o: K.layer_norm(o["x"], o["gamma"], o["beta"], pe=o["pe"], pe_div=4, pe_mod=4),
        lambda: dict(x=dev(32, 64), gamma=vec(64), beta=vec(64), pe=dev(4, 64, dtype=F32)),
        {"host gamma": ("gamma", lambda: host(64, dtype=F32)), "short gamma": ("gamma", lambda: vec(32)),
         "short pe": ("pe", lambda: dev(3, 64, dtype=F32))}),
    "layer_norm_lora": (
        lambda K, o: K.layer_norm_lora(o["x"], o["gamma"], o["beta"], 1e-5, o["A"]),
        lambda: dict(x=dev(32, 64), gamma=vec(64), beta=vec(64), A=dev(16, 64)),
        {"host gamma": ("gamma", lambda: host(64, dtype=F32))}),
    "layer_norm_bwd": (
        lambda K, o: K.layer_norm_bwd(o["x"], o["g"], o["gamma"]),
        lambda: dict(x=dev(32, 64), g=dev(32, 64), gamma=vec(64)),
        {"short g": ("g", lambda: dev(16, 64)), "narrow g": ("g", lambda: dev(32, 32)),
         "host gamma": ("gamma", lambda: host(64, dtype=F32)), "short gamma": ("gamma", lambda: vec(32))}),
    "group_norm_bwd": (
        lambda K, o: K.group_norm_bwd(o["x"], o["g"], 2, 16, 32, 1e-5, o["gamma"], o["beta"]),
        lambda: dict(x=dev(32, 64), g=dev(32, 64), gamma=vec(64), beta=vec(64)),
        {"host gamma": ("gamma", lambda: host(64, dtype=F32)), "host beta": ("beta", lambda: host(64, dtype=F32))}),
    "conv3x3": (
        lambda K, o: K.conv3x3(o["x1"], 2, 4, 4, o["w"], o["bias"], row_bias=o["row_bias"], row_bias_div=16),
        lambda: dict(x1=dev(32, 64), w=dev(64, 576), bias=vec(64), row_bias=dev(2, 64, dtype=F32)),
        {"host bias": ("bias", lambda: host(64, dtype=F32)), "short row_bias": ("row_bias", lambda: dev(1, 64, dtype=F32))}),
    "conv3x3_down_pad0": (
        lambda K, o: K.conv3x3_down_pad0(o["x"], 2, 4, 4, o["w"], o["bias"]),
        lambda: dict(x=dev(32, 64), w=dev(64, 576), bias=vec(64)),
        {"host bias": ("bias", lambda: host(64, dtype=F32))}),
    "timestep_embedding": (
        lambda K, o: K.timestep_embedding(o["t"], 2, 64, o["out"], col0=64, step_idx=o["step_idx"]),
        lambda: dict(t=vec(8), out=dev(2, 128), step_idx=dev(1, dtype=I32)),
        {"host out": ("out", lambda: host(2, 128)), "narrow out": ("out", lambda: dev(2, 120)),
         "short out": ("out", lambda: dev(1, 128)), "host step_idx": ("step_idx", lambda: host(1, dtype=I32)),
         "int64 step_idx": ("step_idx", lambda: dev(1, dtype=I64))}),
    "pack_latents": (
        lambda K, o: K.pack_latents(o["lat"], o["out"], sigmas=o["sigmas"], step_idx=o["step_idx"], ncopy=2),
        lambda: dict(lat=dev(1, 4, 2, 4, 4, dtype=F32), out=dev(64, 4), sigmas=vec(3), step_idx=dev(1, dtype=I32)),
        {"host lat": ("lat", lambda: host(1, 4, 2, 4, 4, dtype=F32)), "short out": ("out", lambda: dev(32, 4)),
         "host sigmas": ("sigmas", lambda: host(3, dtype=F32)), "int64 step_idx": ("step_idx", lambda: dev(1, dtype=I64)),
         "host step_idx": ("step_idx", lambda: host(1, dtype=I32))}),
    "vae_sample": (
        lambda K, o: K.vae_sample(o["moments"], 2, 4, 4, o["eps"], 0.13025),
        lambda: dict(moments=dev(32, 8), eps=dev(2, 4, 4, 4, dtype=F32)),
        {"host eps": ("eps", lambda: host(2, 4, 4, 4, dtype=F32))}),
    "temporal_attention": (
        lambda K, o: K.temporal_attention(o["q"], o["k"], o["v"], 1, 2, 16, 1, 64),
        _qkv, {"short k": ("k", _short(1)), "short v": ("v", _short(2))}),
    "spatial_attention_bwd": (
        lambda K, o: K.spatial_attention_bwd(o["q"], o["k"], o["v"], o["o"], o["dout"], o["lse"], 2, 1, 16, 16),
        lambda: dict(_qkv(), o=dev(32, 64), dout=dev(32, 64), lse=vec(32)),
        {"short o": ("o", lambda: dev(16, 64)), "short dout": ("dout", lambda: dev(16, 64))}),
    "step_advance": (
        lambda K, o: K.step_advance(o["step_idx"], 50),
        lambda: dict(step_idx=dev(1, dtype=I32)),
        {"host step_idx": ("step_idx", lambda: host(1, dtype=I32))}),
    # the text encoder's wrappers
    "causal_attention": (
        lambda K, o: K.causal_attention(o["q"], o["k"], o["v"], 2, 1, 16),
        _qkv, {"host q": ("q", lambda: host(32, 64)), "short v": ("v", _short(2))}),
    "quick_gelu": (
        lambda K, o: K.quick_gelu(o["x"], out=o["out"]),
        lambda: dict(x=dev(32, 64), out=dev(32, 64)),
        {"host out": ("out", lambda: host(32, 64)), "fp32 out": ("out", lambda: dev(32, 64, dtype=F32))}),
    "residual_layer_norm": (
        lambda K, o: K.residual_layer_norm(o["h"], o["y"], o["gamma"], o["beta"], 1e-5),
        lambda: dict(h=dev(32, 64, dtype=F32), y=dev(32, 64), gamma=vec(64), beta=vec(64)),
        {"bf16 h": ("h", lambda: dev(32, 64)), "short gamma": ("gamma", lambda: vec(32)),
         "host beta": ("beta", lambda: host(64, dtype=F32)), "short y": ("y", lambda: dev(16, 64))}),
    "embed_tokens": (
        lambda K, o: K.embed_tokens(o["ids"], 16, o["tok"], o["pos"]),
        lambda: dict(ids=dev(32, dtype=I32), tok=dev(100, 64), pos=dev(16, 64)),
        {"fp32 tok": ("tok", lambda: dev(100, 64, dtype=F32)), "fp32 pos": ("pos", lambda: dev(16, 64, dtype=F32)),
         "int64 ids": ("ids", lambda: dev(32, dtype=I64)), "host ids": ("ids", lambda: host(32, dtype=I32)),
         "short pos": ("pos", lambda: dev(8, 64))}),
}


@pytest.mark.parametrize("wrapper,label", [(w, b) for w, (_, _, bads) in WRAPPERS.items() for b in bads])
def test_bad_operand_is_refused_before_the_library(K, wrapper, label):
    run, good, bads = WRAPPERS[wrapper]
    arg, bad = bads[label]
    with pytest.raises(K._lib.VstError, match=f"^{wrapper}: {arg} "):
        run(K, {**good(), arg: bad()})
    assert K.calls == []


@pytest.mark.parametrize("wrapper", list(WRAPPERS))
def test_good_operands_reach_the_library_once(K, wrapper):
    run, good, _ = WRAPPERS[wrapper]
    run(K, good())
    assert len(K.calls) == 1 and K.calls[0][0].startswith("vst_"), K.calls


def test_text_encoder_makes_no_library_call_of_its_own():
    import inspect
    from video_style_transfer_amd import text_encoder as T
    assert not hasattr(T, "_lib") and "_lib.call" not in inspect.getsource(T)
