"""CPU tests of the IP-Adapter host layer: the fp32 definition against a hand-written per-head SDPA,
the fold of the image keys into the query projection, the checkpoint layout, ImagePrompt's validation, and the operand
refusals of kernels.ip_attention_add (the recorder pattern of test_operand_checks.py)."""
import math

import pytest
import torch

from test_host import fake_device_tensor as dev

BF16, F32 = torch.bfloat16, torch.float32


def _manual(q, k, v, heads):
    """softmax(q k^T / sqrt(d)) v per batch element and head, written out."""
    B, N, C = q.shape
    d = C // heads
    out = torch.zeros_like(q)
    for b in range(B):
        for h in range(heads):
            sl = slice(h * d, (h + 1) * d)
            s = q[b, :, sl] @ k[b, :, sl].t() / math.sqrt(d)
            out[b, :, sl] = torch.softmax(s, -1) @ v[b, :, sl]
    return out


def test_reference_matches_per_head_sdpa():
    from video_style_transfer_amd.ip_adapter import decoupled_attention_reference
    g = torch.Generator().manual_seed(0)
    B, N, L, T, heads, C = 2, 7, 5, 3, 2, 128
    q, k, v = (torch.randn(B, n, C, generator=g, dtype=torch.float64) for n in (N, L, L))
    ki, vi = (torch.randn(B, T, C, generator=g, dtype=torch.float64) for _ in range(2))
    want = _manual(q, k, v, heads) + 0.7 * _manual(q, ki, vi, heads)
    got = decoupled_attention_reference(q, k, v, ki, vi, heads, 0.7)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    only = decoupled_attention_reference(q, None, None, ki, vi, heads, 1.0)
    assert torch.allclose(only, _manual(q, ki, vi, heads), rtol=1e-12, atol=1e-12)
    # round_to: each SDPA output passes through the dtype, as `.to(query.dtype)` does under bf16
    r = decoupled_attention_reference(q.float(), None, None, ki.float(), vi.float(), heads, 1.0, round_to=BF16)
    assert torch.equal(r, r.to(BF16).float())


@pytest.mark.parametrize("lora,bias", [(False, False), (True, False), (False, True), (True, True)])
def test_fold_identity_fp64(lora, bias):
    """Scores through G and c equal q . k_ip, with the LoRA operands of a ProjOps and with a bias."""
    from video_style_transfer_amd.ip_adapter import effective_query_weight, fold_image_keys
    from video_style_transfer_amd.lora_linear import ProjOps
    g = torch.Generator().manual_seed(1)
    B, N, T, heads, K = 2, 9, 5, 3, 64
    inner, P = 64 * heads, 32
    f64 = dict(generator=g, dtype=torch.float64)
    w = torch.randn(inner, K + (P if lora else 0), **f64)
    a = torch.randn(P, K, **f64) if lora else None
    b = torch.randn(inner, **f64) if bias else None
    ops = ProjOps(w, a, b, K, inner)
    w_eff = effective_query_weight(ops, torch.float64)
    assert w_eff.shape == (inner, K) and (lora or torch.equal(w_eff, w))
    x = torch.randn(B, N, K, **f64)
    k_ip = torch.randn(B, T, inner, **f64)
    qf = x @ w[:, :K].t() + ((x @ a.t()) @ w[:, K:].t() if lora else 0) + (b if bias else 0)
    want = torch.einsum("bnhd,bthd->bhnt", qf.view(B, N, heads, 64), k_ip.view(B, T, heads, 64))
    G, c = fold_image_keys(k_ip, w_eff, b, heads)
    assert G.shape == (B, heads, T, K) and (c is None) == (not bias)
    got = torch.einsum("bnk,bhtk->bhnt", x, G) + (c[:, :, None, :] if bias else 0)
    assert torch.allclose(got, want, rtol=1e-10, atol=1e-10)


def _tiny_unet():
    from video_style_transfer_amd.config import UNetMotionConfig
    from video_style_transfer_amd.unet_motion import UNetMotionModel
    torch.manual_seed(0)
    return UNetMotionModel(UNetMotionConfig.tiny())


def _state_dict(unet, T=4, embed=32, seed=0):
    from video_style_transfer_amd.ip_adapter import ip_adapter_layers
    g = torch.Generator().manual_seed(seed)
    D = unet.config.cross_attention_dim
    ipa = {}
    for i, (_, m) in enumerate(ip_adapter_layers(unet)):
        for w in ("to_k_ip", "to_v_ip"):
            ipa[f"{2 * i + 1}.{w}.weight"] = torch.randn(m.inner_dim, D, generator=g) * 0.05
    proj = {"proj.weight": torch.randn(T * D, embed, generator=g) * 0.1, "proj.bias": torch.randn(T * D, generator=g),
            "norm.weight": torch.rand(D, generator=g) + 0.5, "norm.bias": torch.randn(D, generator=g) * 0.1}
    return {"image_proj": proj, "ip_adapter": ipa}


def test_load_ip_adapter_round_trip(tmp_path):
    from video_style_transfer_amd.attention_processor import AnimateDiffAttnProcessor2_0
    from video_style_transfer_amd.ip_adapter import (IPAdapterAttnProcessor2_0, ImageProjection, ip_adapter_layers,
                                                     load_ip_adapter)
    unet = _tiny_unet()
    layers = ip_adapter_layers(unet)
    keys = list(unet.attn_processors)
    want = [k for k in keys if ".attn2." in k and "motion_modules" not in k]
    assert [k for k, _ in layers] == want and len(want) > 2
    sd = _state_dict(unet)
    path = tmp_path / "ip.bin"
    torch.save(sd, path)
    assert load_ip_adapter(unet, str(path)) == len(want)
    procs = unet.attn_processors
    assert list(procs) == keys  # the surface keeps its keys and order
    for i, k in enumerate(want):  # id 2 i + 1 lands on the i-th spatial attn2, with the reference's parameter names
        p = procs[k]
        assert isinstance(p, IPAdapterAttnProcessor2_0) and isinstance(p, AnimateDiffAttnProcessor2_0)
        assert p.num_tokens == 4 and p.scale == 1.0
        assert set(dict(p.named_parameters())) == {"to_k_ip.weight", "to_v_ip.weight"}
        assert torch.equal(p.to_k_ip.weight, sd["ip_adapter"][f"{2 * i + 1}.to_k_ip.weight"])
        assert torch.equal(p.to_v_ip.weight, sd["ip_adapter"][f"{2 * i + 1}.to_v_ip.weight"])
        assert not p.to_k_ip.weight.requires_grad
    for k in keys:
        if k not in want:
            assert not isinstance(procs[k], IPAdapterAttnProcessor2_0), k
    hid = unet.encoder_hid_proj
    assert isinstance(hid, ImageProjection) and hid.num_image_text_embeds == 4
    assert set(dict(hid.named_parameters())) == {"image_embeds.weight", "image_embeds.bias", "norm.weight", "norm.bias"}
    assert torch.equal(hid.image_embeds.weight, sd["image_proj"]["proj.weight"])
    assert torch.equal(hid.norm.bias, sd["image_proj"]["norm.bias"])
    # input_lora_ops keeps working: the block's LayerNorm still learns the q operands of an IP layer
    from video_style_transfer_amd.attention_processor import input_lora_ops
    assert input_lora_ops(layers[0][1], False) is not None

    # scales: a float for all, or {prefix: float} with 0 elsewhere
    unet.set_ip_adapter_scale(0.5)
    assert all(procs[k].scale == 0.5 for k in want)
    pre = want[-1].rsplit(".transformer_blocks", 1)[0]
    unet.set_ip_adapter_scale({pre: 0.8})
    under = [k for k in want if k.startswith(pre)]
    assert under and len(under) < len(want)
    assert all(procs[k].scale == (0.8 if k in under else 0.0) for k in want)
    with pytest.raises(ValueError, match="no IP-Adapter layer under"):
        unet.set_ip_adapter_scale({"nowhere": 1.0})
    with pytest.raises(ValueError, match="finite"):
        unet.set_ip_adapter_scale(float("nan"))


def test_load_ip_adapter_refuses_a_wrong_layout():
    from video_style_transfer_amd.ip_adapter import IPAdapterAttnProcessor2_0, load_ip_adapter
    unet = _tiny_unet()
    sd = _state_dict(unet)
    bad = {"image_proj": sd["image_proj"], "ip_adapter": dict(sd["ip_adapter"])}
    bad["ip_adapter"]["2.to_k_ip.weight"] = bad["ip_adapter"].pop("1.to_k_ip.weight")
    with pytest.raises(ValueError, match="ip_adapter keys"):
        load_ip_adapter(unet, bad)
    bad = {"image_proj": sd["image_proj"], "ip_adapter": dict(sd["ip_adapter"])}
    bad["ip_adapter"]["1.to_k_ip.weight"] = torch.zeros(3, 3)
    with pytest.raises(ValueError, match="1.to_k_ip.weight"):
        load_ip_adapter(unet, bad)
    with pytest.raises(ValueError, match="image_proj"):
        load_ip_adapter(unet, {"ip_adapter": sd["ip_adapter"]})
    # nothing was installed by the refused calls
    assert not any(isinstance(p, IPAdapterAttnProcessor2_0) for p in unet.attn_processors.values())
    assert not hasattr(unet, "encoder_hid_proj")


def test_image_prompt_validation():
    from video_style_transfer_amd.ip_adapter import ImagePrompt
    tok = torch.randn(2, 4, 32)
    p = ImagePrompt(tok, 3)
    assert p.rows == 6 and p.num_tokens == 4 and p.version == 0
    assert p.tokens.dtype == BF16 and torch.equal(p.tokens, tok.to(BF16))
    assert p.strength.dtype == F32 and torch.equal(p.strength, torch.ones(6))
    t_ptr, s_ptr = p.tokens.data_ptr(), p.strength.data_ptr()
    p.set_strength(0.5)
    assert p.version == 1 and torch.equal(p.strength, torch.full((6,), 0.5))
    p.set_strength([0.0, 1.0, 2.0])
    assert torch.equal(p.strength, torch.tensor([0.0, 1.0, 2.0] * 2))
    p.set_strength(torch.arange(6.0).view(2, 3))
    assert torch.equal(p.strength, torch.arange(6.0))
    p.set_tokens(tok * 2)
    assert p.version == 4 and torch.equal(p.tokens, (tok * 2).to(BF16))
    assert (p.tokens.data_ptr(), p.strength.data_ptr()) == (t_ptr, s_ptr)  # in place: a captured step holds them
    for bad in (float("nan"), [1.0, float("inf"), 0.0], torch.ones(2), torch.ones(3, 2), torch.ones(2, 3, 1)):
        with pytest.raises(ValueError, match="strength"):
            p.set_strength(bad)
    assert p.version == 4 and torch.equal(p.strength, torch.arange(6.0))  # a refused call writes nothing
    with pytest.raises(ValueError, match="image tokens"):
        p.set_tokens(torch.zeros(2, 5, 32))
    for shape in ((2, 32), (2, 0, 32), (2, 17, 32)):
        with pytest.raises(ValueError, match="image tokens"):
            ImagePrompt(torch.zeros(*shape), 3)
    with pytest.raises(ValueError, match="frames"):
        ImagePrompt(tok, 0)
    with pytest.raises(ValueError, match="strength"):
        ImagePrompt(tok, 3, strength=float("inf"))


# ---- kernels.ip_attention_add: the wrapper refuses a bad operand before the library is touched -------------------
@pytest.fixture
def K(monkeypatch):
    from video_style_transfer_amd import kernels
    calls = []
    monkeypatch.setattr(kernels._lib, "call", lambda name, *args: calls.append((name, args)) or 0)
    monkeypatch.setattr(kernels, "_stream", lambda: 0)
    kernels.calls = calls
    yield kernels
    del kernels.calls


def _good():
    # M = 4 frames x 16 rows, K = 64, 2 heads, 2 token batches (kv_div 2)
    return dict(x=dev(64, 64), G=dev(2 * 2 * 16, 64), gbias=dev(64, dtype=F32), V=dev(32, 128), out=dev(64, 128),
                row_scale=dev(4, dtype=F32))


def _run(K, o, **kw):
    args = dict(Nq=16, heads=2, T=4, kv_div=2)
    args.update(kw)
    return K.ip_attention_add(o["x"], o["G"], o["gbias"], o["V"], o["out"], row_scale=o["row_scale"], **args)


BAD_OPERANDS = {
    "host x": ("x", lambda: torch.zeros(64, 64, dtype=BF16)),
    "fp32 x": ("x", lambda: dev(64, 64, dtype=F32)),
    "x K % 64": ("x", lambda: dev(64, 96)),
    "x rows % Nq": ("x", lambda: dev(60, 64)),
    "x odd stride": ("x", lambda: dev(64, 68)[:, :64]),
    "x misaligned": ("x", lambda: dev(65, 72).reshape(-1)[4:4 + 64 * 72].view(64, 72)[:, :64]),
    "host G": ("G", lambda: torch.zeros(64, 64, dtype=BF16)),
    "short G": ("G", lambda: dev(32, 64)),
    "narrow G": ("G", lambda: dev(64, 32)),
    "G rows % 16 heads": ("G", lambda: dev(72, 64)),
    "G odd stride": ("G", lambda: dev(64, 68)[:, :64]),
    "bf16 gbias": ("gbias", lambda: dev(64, dtype=BF16)),
    "short gbias": ("gbias", lambda: dev(32, dtype=F32)),
    "host gbias": ("gbias", lambda: torch.zeros(64, dtype=F32)),
    "short V": ("V", lambda: dev(16, 128)),
    "narrow V": ("V", lambda: dev(32, 64)),
    "host V": ("V", lambda: torch.zeros(32, 128, dtype=BF16)),
    "short out": ("out", lambda: dev(32, 128)),
    "narrow out": ("out", lambda: dev(64, 64)),
    "fp32 out": ("out", lambda: dev(64, 128, dtype=F32)),
    "out odd stride": ("out", lambda: dev(64, 132)[:, :128]),
    "short row_scale": ("row_scale", lambda: dev(3, dtype=F32)),
    "bf16 row_scale": ("row_scale", lambda: dev(4, dtype=BF16)),
    "host row_scale": ("row_scale", lambda: torch.zeros(4, dtype=F32)),
}


@pytest.mark.parametrize("label", sorted(BAD_OPERANDS))
def test_wrapper_refuses_bad_operand(K, label):
    arg, make = BAD_OPERANDS[label]
    o = _good()
    o[arg] = make()
    with pytest.raises(K._lib.VstError, match=f"^ip_attention_add: {arg} "):
        _run(K, o)
    assert K.calls == []


@pytest.mark.parametrize("kw,arg", [(dict(T=0), "T"), (dict(T=17), "T"), (dict(heads=0), "Nq, heads, kv_div"),
                                    (dict(Nq=0), "Nq, heads, kv_div"), (dict(kv_div=0), "Nq, heads, kv_div"),
                                    (dict(kv_div=1), "G")])  # kv_div 1: four token batches, G holds two
def test_wrapper_refuses_bad_scalars(K, kw, arg):
    with pytest.raises(K._lib.VstError, match=f"^ip_attention_add: {arg} "):
        _run(K, _good(), **kw)
    assert K.calls == []


def test_wrapper_good_operands_reach_the_library_once(K):
    o = _good()
    assert _run(K, o) is o["out"]
    assert len(K.calls) == 1
    name, a = K.calls[0]
    assert name == "vst_ip_attention_add"
    # (x, ldx, K, G, ldg, gbias, V, ldv, nbatch, M, Nq, heads, T, kv_div, scale, layer_scale, row_scale, O, ldo, stream)
    assert a[1:3] == (64, 64) and a[4] == 64 and a[7] == 128 and a[8:14] == (2, 64, 16, 2, 4, 2)
    assert a[14:16] == (0.125, 1.0) and a[18] == 128 and a[0] == o["x"].data_ptr() and a[17] == o["out"].data_ptr()
    # optional operands may be absent, and strided views are operands like any other
    K.calls.clear()
    o = _good()
    o.update(gbias=None, row_scale=None, x=dev(64, 128)[:, 64:], out=dev(64, 256)[:, 128:])
    _run(K, o)
    assert len(K.calls) == 1 and K.calls[0][1][5] is None and K.calls[0][1][16] is None
    assert K.calls[0][1][1] == 128 and K.calls[0][1][18] == 256


def test_library_refuses_without_gpu():
    """The status codes of vst_ip_attention_add come before any launch, so they can be asked for without a GPU."""
    from video_style_transfer_amd import _lib
    lib = _lib.load()
    X, G, V, O = 4096, 8192, 16384, 32768  # never dereferenced: every call below is refused on the host

    def call(x=X, ldx=64, K=64, g=G, ldg=64, gb=None, v=V, ldv=128, nb=2, M=64, Nq=16, heads=2, T=4, kvd=2, rs=None,
             o=O, ldo=128):
        return lib.vst_ip_attention_add(x, ldx, K, g, ldg, gb, v, ldv, nb, M, Nq, heads, T, kvd, 0.125, 1.0, rs, o,
                                        ldo, None)
    for kw in (dict(x=None), dict(g=None), dict(v=None), dict(o=None), dict(K=0), dict(M=0), dict(Nq=0), dict(heads=0),
               dict(T=0), dict(kvd=0), dict(nb=0), dict(T=17), dict(K=96, ldx=96, ldg=96), dict(M=60), dict(nb=1),
               dict(ldx=68), dict(ldg=68), dict(ldv=132), dict(ldo=132), dict(ldx=56), dict(ldg=56), dict(ldv=120),
               dict(ldo=120), dict(x=X + 8), dict(g=G + 2), dict(v=V + 4), dict(o=O + 8), dict(gb=4100), dict(rs=4098),
               dict(M=1 << 24, Nq=1 << 12, nb=1 << 12, ldx=64), dict(nb=1 << 20, ldg=1024, K=64)):
        assert call(**kw) == 1, kw
    assert call(heads=21, ldv=64 * 21, ldo=64 * 21) == 3
    assert call(heads=21, ldv=64 * 21, ldo=64 * 21, T=17) == 1  # a bad argument is reported before the shape
