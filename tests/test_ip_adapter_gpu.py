"""GPU tests of the IP-Adapter image attention: vst_ip_attention_add against the fp32 definition, its
exact cases, views, invariance and status codes; the processor, the UNet against the oracle, the denoiser.

Measured on an MI355X (rel_l2 of the image term against decoupled_attention_reference in fp32 from the unfolded q, k,
v; the yardstick is the same function with q, k, v and its output rounded to bf16; gate: kernel <= 1.5 x yardstick):
shape A 2.166e-3 against 2.004e-3 (1.08 x), B 2.459e-3 against 2.187e-3 (1.12 x), C 2.151e-3 against 1.978e-3 (1.09 x),
tail 2.082e-3 against 1.981e-3 (1.05 x).  Tiny UNet against the oracle: 7.85e-3, the plain forward 7.50e-3."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
NAN = float("nan")


@pytest.fixture(scope="module")
def K():
    from video_style_transfer_amd import kernels
    return kernels


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm()).item()


def bits(t):
    return t.contiguous().view(torch.int16)


def profiled(K, fn):
    K.profile_launches(True)
    try:
        out = fn()
        kinds = [r[0] for r in K.collect_launches()]
    finally:
        K.profile_launches(False)
    return out, kinds


# ------------------------------------------------------------------------------------------ operands
def make_case(Kd, heads, T, Nq, frames, clips, kv_div, bias=False, seed=0, dev=None):
    """CPU inputs (bf16-valued fp32) and the kernel's device operands, rows t >= T of G, gbias and V filled with NaN."""
    from video_style_transfer_amd.ip_adapter import fold_image_keys
    g = torch.Generator().manual_seed(seed)
    nf = frames * clips
    nb = (nf - 1) // kv_div + 1
    M, inner = nf * Nq, 64 * heads

    def r(*shape, s=1.0):
        return (torch.randn(*shape, generator=g) * s).to(BF16).float()
    x, W = r(M, Kd), r(inner, Kd, s=Kd ** -0.5)
    b = r(inner, s=0.5) if bias else None
    k_ip, v_ip = r(nb, T, inner), r(nb, T, inner)
    Gf, cf = fold_image_keys(k_ip, W, b, heads)
    G = torch.full((nb, heads, 16, Kd), NAN)
    G[:, :, :T] = Gf
    V = torch.full((nb, 16, inner), NAN)
    V[:, :T] = v_ip
    c = None
    if bias:
        c = torch.full((nb, heads, 16), NAN)
        c[:, :, :T] = cf
    ops = dict(x=x.to(BF16).to(dev), G=G.view(-1, Kd).to(BF16).to(dev), V=V.view(-1, inner).to(BF16).to(dev),
               gbias=None if c is None else c.view(-1).to(dev))
    return dict(x=x, W=W, b=b, k_ip=k_ip, v_ip=v_ip, nf=nf, nb=nb, M=M, inner=inner, heads=heads, T=T, Nq=Nq,
                kv_div=kv_div, K=Kd, ops=ops)


def launch(K, c, out=None, ops=None, **kw):
    ops = ops or c["ops"]
    if out is None:
        out = torch.zeros(ops["x"].shape[0], c["inner"], dtype=BF16, device=ops["x"].device)
    args = dict(Nq=c["Nq"], heads=c["heads"], T=c["T"], kv_div=c["kv_div"])
    args.update(kw)
    return K.ip_attention_add(ops["x"], ops["G"], ops["gbias"], ops["V"], out, **args)


def reference(c, rounded=False):
    """The image term of unzip_attention_processor.py:1793-1807 from the unfolded q, k, v: fp32, or with q, k, v and
    the SDPA output rounded to bf16 (the reference's own roundings: the yardstick)."""
    from video_style_transfer_amd.ip_adapter import decoupled_attention_reference
    q = c["x"] @ c["W"].t() + (c["b"] if c["b"] is not None else 0)
    if rounded:
        q = q.to(BF16).float()
    idx = torch.arange(c["nf"]) // c["kv_div"]
    o = decoupled_attention_reference(q.view(c["nf"], c["Nq"], -1), None, None, c["k_ip"][idx], c["v_ip"][idx],
                                      c["heads"], 1.0, round_to=BF16 if rounded else None)
    return o.reshape(c["M"], -1)


SHAPES = {  # K, heads, T, Nq, frames, clips, kv_div, bias
    "A": (128, 2, 5, 80, 2, 2, 2, True),     # row tiles straddle frames and token batches; a bias
    "B": (640, 10, 16, 256, 4, 1, 2, False),
    "C": (1280, 20, 4, 256, 2, 1, 1, False),
    # not in the issue's table: the same path with a last row tile of 8 rows (M = 3 * 24) that spans two batches
    "tail": (64, 1, 3, 24, 3, 1, 1, True),
}


@pytest.fixture(scope="module")
def cases(cuda):
    return {n: make_case(*s, seed=i, dev=cuda) for i, (n, s) in enumerate(SHAPES.items())}


# ------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("name", list(SHAPES))
def test_kernel_vs_reference(cuda, K, cases, name):
    c = cases[name]
    ref = reference(c)
    e_y = rel(reference(c, rounded=True), ref)
    out = launch(K, c)
    assert torch.isfinite(out).all()
    e_k = rel(out, ref)
    print(f"ip_attention_add shape {name}: kernel rel_l2 {e_k:.3e}, bf16 reference rel_l2 {e_y:.3e}, "
          f"ratio {e_k / e_y:.3f}")
    assert e_k <= 1.5 * e_y, (name, e_k, e_y)


# ------------------------------------------------------------------------------------------ 2. exact cases
def test_single_token_is_exact_and_zero_frames_keep_their_bits(cuda, K):
    c = make_case(128, 2, 1, 48, 4, 1, 2, seed=11, dev=cuda)
    g = torch.Generator().manual_seed(12)
    O = torch.randn(c["M"], c["inner"], generator=g).to(BF16)
    O[3 * 48:, ::2] = -0.0   # frame 3 has scale 0: these bits must survive
    O[3 * 48:, 1::2] = NAN
    rs = torch.tensor([0.5, 0.25, 1.0, 0.0])  # x layer_scale 2 -> 1, 0.5, 2, 0
    out = launch(K, c, out=O.to(cuda).clone(), layer_scale=2.0, row_scale=rs.to(cuda)).cpu()
    s = (2.0 * rs).repeat_interleave(48).view(-1, 1)
    v0 = c["v_ip"][torch.arange(4) // 2, 0].repeat_interleave(48, 0)   # softmax over one key is 1
    want = (O.float() + s * v0).to(BF16)
    live = slice(0, 3 * 48)
    assert torch.equal(bits(out[live]), bits(want[live]))
    assert torch.equal(bits(out[3 * 48:]), bits(O[3 * 48:]))
    assert (bits(out[3 * 48:, ::2]) == -32768).all() and torch.isnan(out[3 * 48:, 1::2]).all()


def test_scale_sign_and_size(cuda, K, cases):
    c = cases["A"]
    one = launch(K, c).float()
    ref = reference(c)
    for s in (-1.5, 3.0):
        out = launch(K, c, layer_scale=s)
        assert torch.equal(bits(out), bits((s * one).to(BF16)))   # s * bf16 is exact in fp32: one rounding
        assert rel(out, s * ref) < 1e-2
    # layer_scale and row_scale multiply: -1.5 = 3 * -0.5
    rs = torch.full((c["nf"],), -0.5, device=cuda)
    assert torch.equal(bits(launch(K, c, layer_scale=3.0, row_scale=rs)), bits((-1.5 * one).to(BF16)))


# ------------------------------------------------------------------------------------------ 3. padding and views
def test_strided_views_in_poisoned_arenas(cuda, K, cases):
    c = cases["A"]
    dense = launch(K, c)
    ops = c["ops"]

    def arena(t, fill):
        a = torch.full((t.shape[0] + 2, t.shape[1] + 24), fill, dtype=BF16, device=cuda)
        v = a[1:-1, 8:8 + t.shape[1]]
        v.copy_(t)
        return a, v
    xa, xv = arena(ops["x"], NAN)
    ga, gv = arena(ops["G"], NAN)
    va, vv = arena(ops["V"], NAN)
    oa, ov = arena(torch.zeros_like(dense), 7.0)
    before = [t.clone() for t in (xa, ga, va, oa)]
    assert torch.isnan(ops["G"].view(-1, 16, c["K"])[:, c["T"]:]).all() and torch.isnan(ops["gbias"]).any()
    launch(K, c, out=ov, ops=dict(x=xv, G=gv, V=vv, gbias=ops["gbias"]))
    assert torch.isfinite(ov).all() and torch.equal(bits(ov), bits(dense))
    for a, b in zip((xa, ga, va), before):
        assert torch.equal(bits(a), bits(b))
    ob = before[3]
    ob[1:-1, 8:8 + dense.shape[1]] = dense
    assert torch.equal(bits(oa), bits(ob))   # every byte outside the view is unchanged


# ------------------------------------------------------------------------------------------ 4. invariance
def test_repeatable_and_independent_of_the_launch(cuda, K, cases):
    c = cases["A"]   # 4 frames of 80 rows, two clips of two frames, one token batch per clip
    full = launch(K, c)
    assert torch.equal(bits(full), bits(launch(K, c)))
    ops, half = c["ops"], c["M"] // 2
    first = launch(K, c, ops=dict(ops, x=ops["x"][:half]))
    assert torch.equal(bits(first), bits(full[:half]))
    hb = c["heads"] * 16
    second = launch(K, c, ops=dict(x=ops["x"][half:], G=ops["G"][hb:], V=ops["V"][16:], gbias=ops["gbias"][hb:]))
    assert torch.equal(bits(second), bits(full[half:]))
    t = cases["tail"]
    full = launch(K, t)
    assert torch.equal(bits(launch(K, t, ops=dict(t["ops"], x=t["ops"]["x"][:48]))), bits(full[:48]))


# ------------------------------------------------------------------------------------------ 5. status codes
def test_status_codes_before_any_launch(cuda, K, cases):
    from video_style_transfer_amd import _lib
    c = cases["A"]
    o = c["ops"]
    O = torch.full((c["M"], c["inner"]), 3.0, dtype=BF16, device=cuda)
    rs = torch.ones(c["nf"], device=cuda)
    good = dict(x=o["x"].data_ptr(), ldx=c["K"], K=c["K"], G=o["G"].data_ptr(), ldg=c["K"], gb=o["gbias"].data_ptr(),
                V=o["V"].data_ptr(), ldv=c["inner"], nb=c["nb"], M=c["M"], Nq=c["Nq"], heads=c["heads"], T=c["T"],
                kvd=c["kv_div"], rs=rs.data_ptr(), O=O.data_ptr(), ldo=c["inner"])

    def status(**kw):
        a = dict(good, **kw)
        return _lib.load().vst_ip_attention_add(a["x"], a["ldx"], a["K"], a["G"], a["ldg"], a["gb"], a["V"], a["ldv"],
                                                a["nb"], a["M"], a["Nq"], a["heads"], a["T"], a["kvd"], 0.125, 1.0,
                                                a["rs"], a["O"], a["ldo"],
                                                torch.cuda.current_stream().cuda_stream)
    bad = [dict(x=None), dict(G=None), dict(V=None), dict(O=None), dict(K=0), dict(M=0), dict(Nq=0), dict(heads=0),
           dict(T=0), dict(kvd=0), dict(nb=0), dict(T=17), dict(K=96), dict(Nq=70), dict(nb=1), dict(kvd=1),
           dict(ldx=c["K"] + 4), dict(ldg=c["K"] + 4), dict(ldv=c["inner"] + 4), dict(ldo=c["inner"] + 4),
           dict(ldx=c["K"] - 8), dict(ldg=c["K"] - 8), dict(ldv=c["inner"] - 8), dict(ldo=c["inner"] - 8),
           dict(x=good["x"] + 8), dict(G=good["G"] + 2), dict(V=good["V"] + 4), dict(O=good["O"] + 8),
           dict(gb=good["gb"] + 4), dict(rs=good["rs"] + 2),
           dict(ldx=1 << 23, M=1 << 8, Nq=1 << 7), dict(ldg=1 << 26), dict(ldv=1 << 27), dict(ldo=1 << 23)]
    for kw in bad:
        assert status(**kw) == 1, kw
    assert status(heads=21, ldv=64 * 21, ldo=64 * 21) == 3
    torch.cuda.synchronize()
    assert (O == 3.0).all()
    # through the wrapper nothing is recorded either
    K.profile_launches(True)
    try:
        with pytest.raises(_lib.VstError, match="^ip_attention_add: T "):
            launch(K, c, out=O, T=17)
        assert K.collect_launches() == []
    finally:
        K.profile_launches(False)
    assert (O == 3.0).all()
    assert status() == 0   # and the good call runs
    torch.cuda.synchronize()
    assert not (O == 3.0).all()


# ------------------------------------------------------------------------------------------ 6. processor
def test_processor_fused_text_path_plus_image_add(cuda, K):
    from test_gemm_xattn_gpu import check
    from video_style_transfer_amd import attention_processor as AP
    from video_style_transfer_amd.attention_processor import AttnCall, Attention
    from video_style_transfer_amd.ip_adapter import IPAdapterAttnProcessor2_0, ImagePrompt
    from video_style_transfer_amd.utils import attach_unziplora_layers
    torch.manual_seed(3)
    attn = Attention(1280, 2048, 20, 64).to(cuda)
    holder = torch.nn.Module()
    holder.blk = torch.nn.Module()
    holder.blk.attn2 = attn
    attach_unziplora_layers(holder, 8)
    holder.to(cuda)
    with torch.no_grad():
        for name, p in holder.named_parameters():
            if "lora" in name and "up" in name:
                p.normal_(0.0, 0.05)
    proc = IPAdapterAttnProcessor2_0(1280, 2048, num_tokens=4).to(cuda)
    with torch.no_grad():
        proc.to_v_ip.weight.mul_(4.0)
    attn.set_processor(proc)
    holder.requires_grad_(False)
    x = (torch.randn(4, 256, 1280, device=cuda) * 0.5).to(BF16)
    enc = torch.randn(2, 77, 2048, device=cuda).to(BF16)
    tokens = torch.randn(2, 4, 2048, device=cuda).to(BF16)
    prompt = ImagePrompt(tokens, 2)
    proc(attn, x, encoder_hidden_states=enc, _vst=AttnCall(image_prompt=prompt))   # projects the text K/V and folds the keys
    o_fused, kinds = profiled(K, lambda: proc(attn, x, encoder_hidden_states=enc, _vst=AttnCall(image_prompt=prompt)))
    i = kinds.index("gemm_xattn")
    assert kinds[i + 1] == "ip_attention_add" and kinds.count("ip_attention_add") == 1, kinds
    assert "spatial_attention" not in kinds
    orig = AP._cross_fusable
    AP._cross_fusable = lambda *a, **k: False
    try:
        o_two, kinds2 = profiled(K, lambda: proc(attn, x, encoder_hidden_states=enc, _vst=AttnCall(image_prompt=prompt)))
    finally:
        AP._cross_fusable = orig
    assert "gemm_xattn" not in kinds2 and kinds2[kinds2.index("spatial_attention") + 1] == "ip_attention_add"
    check(o_fused, o_two, 5e-3, 1e-2, "IP processor: fused attn2 + image add vs two-launch + image add")
    # the reference's calling convention: the image tokens are the last rows of encoder_hidden_states
    cat = torch.cat([enc, tokens], 1)
    o_cat = proc(attn, x, encoder_hidden_states=cat)
    assert torch.equal(bits(o_cat), bits(o_fused))
    o_cat2, kinds3 = profiled(K, lambda: proc(attn, x, encoder_hidden_states=cat))
    assert torch.equal(bits(o_cat2), bits(o_fused))
    assert kinds3 == kinds, kinds3   # nothing is projected again: the text K/V and the fold are cached on the tensor
    # the image term is there, and a layer scale of 0 launches nothing and gives the text-only bits
    plain = AP.AnimateDiffAttnProcessor2_0()(attn, x, encoder_hidden_states=enc)
    assert rel(o_fused, plain) > 2e-2
    proc.scale = 0.0
    o_zero, kinds0 = profiled(K, lambda: proc(attn, x, encoder_hidden_states=enc, _vst=AttnCall(image_prompt=prompt)))
    assert "ip_attention_add" not in kinds0 and torch.equal(bits(o_zero), bits(plain))


# ------------------------------------------------------------------------------------------ 7. UNet
IP_SEED, T_IP = 21, 4


def ip_state_dict(unet, seed=IP_SEED):
    """An IP-Adapter checkpoint for the tiny model: to_v_ip large enough that the image term moves the output."""
    from video_style_transfer_amd.ip_adapter import ip_adapter_layers
    g = torch.Generator().manual_seed(seed)
    D = unet.config.cross_attention_dim
    ipa = {}
    for i, (_, m) in enumerate(ip_adapter_layers(unet)):
        ipa[f"{2 * i + 1}.to_k_ip.weight"] = (torch.randn(m.inner_dim, D, generator=g) * D ** -0.5).to(BF16).float()
        ipa[f"{2 * i + 1}.to_v_ip.weight"] = (torch.randn(m.inner_dim, D, generator=g) * 4 * D ** -0.5).to(BF16).float()
    proj = {"proj.weight": (torch.randn(T_IP * D, 64, generator=g) * 0.125).to(BF16).float(),
            "proj.bias": torch.zeros(T_IP * D), "norm.weight": torch.ones(D), "norm.bias": torch.zeros(D)}
    return {"image_proj": proj, "ip_adapter": ipa}


def image_tokens(cfg, B, seed=IP_SEED + 1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, T_IP, cfg.cross_attention_dim, generator=g).to(BF16).float()


@pytest.fixture(scope="module")
def tiny(cuda):
    """Tiny UNet with its plain outputs taken BEFORE the IP-Adapter is loaded onto it."""
    from test_parity_gpu import _setup
    from video_style_transfer_amd.ip_adapter import load_ip_adapter
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser
    from video_style_transfer_amd.utils import build_unet
    cfg, sd, lat, enc, pooled, tids = _setup("tiny", 4, 16, seed=5, B=2)
    unet = build_unet(cfg, state_dict=sd, device=cuda)
    kw = dict(added_cond_kwargs={"text_embeds": pooled.to(cuda), "time_ids": tids.to(cuda)})
    t = torch.tensor([761.0, 761.0])
    plain = unet(lat.to(cuda), t.to(cuda), enc.to(cuda), **kw).sample.clone()
    d = dict(cfg=cfg, sd=sd, lat=lat, enc=enc, pooled=pooled, tids=tids, unet=unet, kw=kw, t=t, plain=plain)
    den = AnimateDiffDenoiser(unet, 4, 128, 128, num_inference_steps=10, guidance_scale=7.5, device=cuda)
    den.set_prompt_embeds(enc[1:2], pooled[1:2], enc[0:1], pooled[0:1])
    den.init_latents(3)
    d["den_plain"] = den.run_steps(3).clone()
    d["ipsd"] = ip_state_dict(unet)
    assert load_ip_adapter(unet, d["ipsd"]) > 0
    return d


def test_unet_vs_oracle(cuda, K, tiny, monkeypatch):
    import oracle.unet as OU
    from video_style_transfer_amd.ip_adapter import (ImagePrompt, decoupled_attention_reference, ip_adapter_layers)
    cfg, sd, lat, enc, pooled, tids, unet, kw, t = (tiny[k] for k in ("cfg", "sd", "lat", "enc", "pooled", "tids",
                                                                      "unet", "kw", "t"))
    B, Fr = 2, 4
    tokens = image_tokens(cfg, B)
    names = [k[:-len(".processor")] for k, _ in ip_adapter_layers(unet)]
    ipw = {n: (tiny["ipsd"]["ip_adapter"][f"{2 * i + 1}.to_k_ip.weight"],
               tiny["ipsd"]["ip_adapter"][f"{2 * i + 1}.to_v_ip.weight"]) for i, n in enumerate(names)}
    ref0 = OU.unet_forward(sd, cfg.to_dict(), lat, t, enc, pooled, tids)
    e0 = rel(tiny["plain"], ref0)
    orig = OU.attention
    patched = []

    def with_image(P, name, x, enc_, heads, lora):
        if enc_ is None or "motion_modules" in name:
            return orig(P, name, x, enc_, heads, lora)
        patched.append(name)

        def pr(n, t_):
            return OU.proj(P, f"{name}.{'to_out.0' if n == 'to_out' else n}", t_, lora)
        BF = x.shape[0]
        e = enc_.repeat_interleave(BF // enc_.shape[0], 0)
        tok = tokens.repeat_interleave(BF // B, 0)
        wk, wv = ipw[name]
        o = decoupled_attention_reference(pr("to_q", x), pr("to_k", e), pr("to_v", e), tok @ wk.t(), tok @ wv.t(),
                                          heads, 1.0)
        return pr("to_out", o)

    monkeypatch.setattr(OU, "attention", with_image)
    try:
        ref = OU.unet_forward(sd, cfg.to_dict(), lat, t, enc, pooled, tids)
    finally:
        monkeypatch.undo()
    assert sorted(set(patched)) == sorted(names)
    d_ref = rel(ref, ref0)
    assert d_ref >= 5e-2, d_ref   # the image prompt moves the oracle's output

    prompt = ImagePrompt(tokens.to(cuda), Fr)

    def run(p=prompt):
        return unet(lat.to(cuda), t.to(cuda), enc.to(cuda), image_prompt=p, **kw).sample

    out, kinds = profiled(K, run)
    e = rel(out, ref)
    d_hip = rel(out, tiny["plain"])
    print(f"tiny UNet + image prompt: rel_l2 vs oracle {e:.3e} (plain forward {e0:.3e}); with/without image prompt: "
          f"oracle {d_ref:.3e}, HIP {d_hip:.3e}")
    assert kinds.count("ip_attention_add") == len(names)
    assert torch.isfinite(out).all() and e <= 3e-2 and e <= 1.25 * e0 + 2e-3, (e, e0)
    assert d_hip >= 0.5 * d_ref, (d_hip, d_ref)
    # strength 0 on every row: the plain forward bit for bit
    prompt.set_strength(0.0)
    assert torch.equal(run(), tiny["plain"])
    prompt.set_strength(1.0)
    # a per-layer scale of 0 launches nothing
    unet.set_ip_adapter_scale(0.0)
    try:
        out0, kinds0 = profiled(K, run)
    finally:
        unet.set_ip_adapter_scale(1.0)
    assert "ip_attention_add" not in kinds0 and torch.equal(out0, tiny["plain"])
    # block selection: only the layers under the prefix launch
    pre = names[-1].rsplit(".transformer_blocks", 1)[0]
    unet.set_ip_adapter_scale({pre: 1.0})
    try:
        _, kinds1 = profiled(K, run)
    finally:
        unet.set_ip_adapter_scale(1.0)
    assert kinds1.count("ip_attention_add") == sum(n.startswith(pre) for n in names)


# ------------------------------------------------------------------------------------------ 8. denoiser
def _denoiser(tiny, cuda, use_graph=True):
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser
    den = AnimateDiffDenoiser(tiny["unet"], 4, 128, 128, num_inference_steps=10, guidance_scale=7.5, device=cuda,
                              use_graph=use_graph)
    den.set_prompt_embeds(tiny["enc"][1:2], tiny["pooled"][1:2], tiny["enc"][0:1], tiny["pooled"][0:1])
    return den


def test_denoiser_graph_equals_eager_and_new_values_keep_the_graph(cuda, tiny):
    from video_style_transfer_amd.ip_adapter import load_ip_adapter, unload_ip_adapter
    g = torch.Generator().manual_seed(31)
    emb = [torch.randn(1, 64, generator=g) for _ in range(3)]
    ramp = torch.linspace(0.0, 1.5, 4)

    def three(den):
        den.init_latents(3)
        return den.run_steps(3).clone()
    dg, de = _denoiser(tiny, cuda, True), _denoiser(tiny, cuda, False)
    for d in (dg, de):
        d.set_image_prompt(emb[0])
    og, oe = three(dg), three(de)
    assert dg.graph is not None and de.graph is None
    assert torch.isfinite(og).all() and torch.equal(og, oe) and not torch.equal(og, tiny["den_plain"])
    # new tokens and a per-frame strength ramp: the same graph object and buffers, a fresh eager denoiser's bits
    g0, p0 = dg.graph, dg.image_prompt
    ptrs = (p0.tokens.data_ptr(), p0.strength.data_ptr())
    dg.set_image_prompt(emb[1], negative_image_embeds=emb[2], strength=ramp)
    og2 = three(dg)
    assert dg.graph is g0 and dg.image_prompt is p0 and ptrs == (p0.tokens.data_ptr(), p0.strength.data_ptr())
    fresh = _denoiser(tiny, cuda, False)
    fresh.set_image_prompt(emb[1], negative_image_embeds=emb[2], strength=ramp)
    assert torch.equal(og2, three(fresh)) and not torch.equal(og2, og)
    # tokens= bypasses the projection: the projected embeds given as tokens are the same run
    tok = tiny["unet"].encoder_hid_proj(emb[1].to(cuda))
    neg = tiny["unet"].encoder_hid_proj(emb[2].to(cuda))
    fresh.set_image_prompt(tokens=tok, negative_tokens=neg, strength=ramp)
    assert torch.equal(og2, three(fresh))
    # clearing the prompt (and taking the adapter off the model) is the plain run again
    dg.clear_image_prompt()
    assert dg.graph is None and dg.image_prompt is None
    unload_ip_adapter(tiny["unet"])
    try:
        assert torch.equal(three(dg), tiny["den_plain"])
    finally:
        load_ip_adapter(tiny["unet"], tiny["ipsd"])


# ------------------------------------------------------------------------------------------ 9. refusals
def test_refusals_before_any_launch(cuda, K, tiny, monkeypatch):
    from video_style_transfer_amd._lib import VstError
    from video_style_transfer_amd.autograd import unet_train_tokens
    from video_style_transfer_amd.ip_adapter import (ImagePrompt, ip_adapter_layers, load_ip_adapter,
                                                     unload_ip_adapter)
    from video_style_transfer_amd.lora_gate import LoraGate
    cfg, lat, enc, unet, kw, t = (tiny[k] for k in ("cfg", "lat", "enc", "unet", "kw", "t"))
    tokens = image_tokens(cfg, 2).to(cuda)

    def run(**extra):
        return unet(lat.to(cuda), t.to(cuda), enc.to(cuda), **extra, **kw)
    K.profile_launches(True)
    try:
        with pytest.raises(VstError, match="image_prompt.*no image prompt"):
            run()
        with pytest.raises(VstError, match="image_prompt.*rows"):
            run(image_prompt=ImagePrompt(tokens, 3))
        with pytest.raises(VstError, match="image_prompt.*image tokens"):
            run(image_prompt=ImagePrompt(tokens[:, :3], 4))
        with pytest.raises(VstError, match="image_prompt.*lora_gate"):
            run(image_prompt=ImagePrompt(tokens, 4), lora_gate=LoraGate(8, cuda))
        with pytest.raises(VstError, match="image_prompt.*ImagePrompt"):
            run(image_prompt=tokens)
        layer = ip_adapter_layers(unet)[0][1]
        monkeypatch.setattr(layer, "dim_head", 32)
        with pytest.raises(VstError, match="image_prompt.*head_dim 64"):
            run(image_prompt=ImagePrompt(tokens, 4))
        monkeypatch.undo()
        with pytest.raises(NotImplementedError, match="image_prompt.*inference only"):
            unet_train_tokens(unet, None, 2, 4, 16, 16, None, None)
        den = _denoiser(tiny, cuda)
        with pytest.raises(ValueError, match="finite"):
            den.set_image_prompt(tokens=tokens[:1], negative_tokens=tokens[1:], strength=float("nan"))
        with pytest.raises(ValueError, match="one of them"):
            den.set_image_prompt()
        with pytest.raises(ValueError, match="image tokens"):
            den.set_image_prompt(tokens=tokens[0])
        den.set_lora_gates(style=0.5)
        with pytest.raises(VstError, match="image_prompt.*lora_gate"):
            den.set_image_prompt(tokens=tokens[:1], negative_tokens=tokens[1:])
        unload_ip_adapter(unet)
        try:
            with pytest.raises(VstError, match="image_prompt.*no IP-Adapter processors"):
                run(image_prompt=ImagePrompt(tokens, 4))
            launches = K.collect_launches()
        finally:
            load_ip_adapter(unet, tiny["ipsd"])
    finally:
        K.profile_launches(False)
    assert launches == [], [k[0] for k in launches]
