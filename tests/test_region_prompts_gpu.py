"""GPU tests of regional prompts: vst_region_attention against the definition, its exact cases (one-hot
rows, dead regions, a single key), views, invariance and status codes; the processor, the tiny UNet against the oracle
with its attn2 patched to the regional definition, the IP-Adapter on top, the denoiser.

Measured on an MI355X (rel_l2 against the fp32 definition; the yardstick is the same definition with each region's
attention output rounded to bf16; gate: kernel <= 1.5 x yardstick): blocks_end_inside 2.096e-3 against 1.647e-3
(1.27 x), short_tail 1.949e-3 against 1.645e-3 (1.19 x), ten_heads 2.108e-3 against 1.655e-3 (1.27 x), long_prompt
2.124e-3 against 1.672e-3 (1.27 x).  Tiny UNet against the oracle with attn2 patched to the definition: 7.768e-3, the
plain forward 7.503e-3 (1.04 x; the regions move the oracle by 1.443e-1); with an IP-Adapter on top 8.055e-3 (1.07 x;
the image term moves the regional oracle by 2.283e-1)."""
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
def soft_weights(nimg, Nq, R, g):
    """Normalised fp32 [nimg*Nq, 4] with every kind of row: soft everywhere, some entries exactly 0, region 0 dead on
    the first 40 rows of every image, the last region dead on a whole 128-row block where there is one; columns >= R
    NaN."""
    raw = torch.rand(nimg, Nq, R, generator=g) + 0.05
    drop = torch.rand(nimg, Nq, R, generator=g) < 0.3
    keep = torch.arange(Nq).view(1, Nq, 1) % R == torch.arange(R).view(1, 1, R)   # one region always stays
    raw = torch.where(drop & ~keep, torch.zeros(()), raw)
    if R > 1:
        raw[:, :40, 0] = 0.0
        raw[:, :40, 1] += 0.5
        raw[:, :128, R - 1] = 0.0
        raw[:, :128, 0] += (raw[:, :128].sum(-1) == 0).float()
    w = torch.full((nimg, Nq, 4), NAN)
    w[..., :R] = raw / raw.sum(-1, keepdim=True)
    return w.view(nimg * Nq, 4)


def make_case(heads, Nq, Nk, R, frames, clips, kv_div, seed=0, dev=None, wts=None):
    """CPU inputs (bf16-valued fp32) and the device operands.  q [nimg, Nq, inner]; k, v [nkv, R, Nk, inner]."""
    g = torch.Generator().manual_seed(seed)
    nimg = frames * clips
    nkv = nimg // kv_div
    inner = 64 * heads

    def r(*shape):
        return torch.randn(*shape, generator=g).to(BF16).float()
    q, k, v = r(nimg, Nq, inner), r(nkv, R, Nk, inner), r(nkv, R, Nk, inner)
    w = soft_weights(nimg, Nq, R, g) if wts is None else wts
    ops = dict(q=q.view(-1, inner).to(BF16).to(dev), k=k.view(-1, inner).to(BF16).to(dev),
               v=v.view(-1, inner).to(BF16).to(dev), wts=w.to(dev))
    return dict(q=q, k=k, v=v, w=w, nimg=nimg, nkv=nkv, inner=inner, heads=heads, Nq=Nq, Nk=Nk, R=R, kv_div=kv_div,
                ops=ops)


def launch(K, c, ops=None, out=None, **kw):
    ops = ops or c["ops"]
    args = dict(nimg=c["nimg"], heads=c["heads"], Nq=c["Nq"], Nk=c["Nk"], R=c["R"], kv_div=c["kv_div"])
    args.update(kw)
    return K.region_attention(ops["q"], ops["k"], ops["v"], ops["wts"], out=out, **args)


def definition(c, rounded=False):
    """O[m] = sum over r with w_r[m] != 0 of w_r[m] softmax(q_m K_r^T / 8) V_r in fp32; `rounded`: q, K, V (already
    bf16 values) and each region's attention output rounded to bf16, the yardstick."""
    nimg, Nq, heads, R = c["nimg"], c["Nq"], c["heads"], c["R"]
    q = c["q"].view(nimg, Nq, heads, 64).transpose(1, 2)                     # [nimg, heads, Nq, 64]
    idx = torch.arange(nimg) // c["kv_div"]
    w = c["w"].view(nimg, Nq, 4)
    out = torch.zeros(nimg, Nq, heads * 64)
    for r in range(R):
        k = c["k"][idx, r].view(nimg, -1, heads, 64).transpose(1, 2)
        v = c["v"][idx, r].view(nimg, -1, heads, 64).transpose(1, 2)
        p = torch.softmax(q @ k.transpose(-1, -2) * 0.125, -1)
        o = (p @ v).transpose(1, 2).reshape(nimg, Nq, heads * 64)
        if rounded:
            o = o.to(BF16).float()
        wr = w[..., r:r + 1]
        out = out + torch.where(wr != 0, wr * o, torch.zeros(()))
    return out.view(nimg * Nq, -1)


SHAPES = {  # heads, Nq, Nk, R, frames, clips, kv_div
    "blocks_end_inside": (2, 80, 77, 3, 2, 2, 2),    # query blocks end inside an image, two tiles per region
    "short_tail": (1, 24, 5, 4, 3, 1, 1),            # one short tile, a 24-row tail
    "ten_heads": (10, 256, 77, 2, 2, 1, 2),
    "long_prompt": (2, 160, 130, 2, 1, 1, 1),        # three key tiles
}


@pytest.fixture(scope="module")
def cases(cuda):
    return {n: make_case(*s, seed=i, dev=cuda) for i, (n, s) in enumerate(SHAPES.items())}


# ------------------------------------------------------------------------------------------ 1. against the definition
@pytest.mark.parametrize("name", list(SHAPES))
def test_kernel_vs_definition(cuda, K, cases, name):
    c = cases[name]
    ref = definition(c)
    e_y = rel(definition(c, rounded=True), ref)
    out = launch(K, c)
    assert torch.isfinite(out).all()
    e_k = rel(out, ref)
    print(f"region_attention shape {name}: kernel rel_l2 {e_k:.3e}, bf16 yardstick rel_l2 {e_y:.3e}, "
          f"ratio {e_k / e_y:.3f}")
    assert e_k <= 1.5 * e_y, (name, e_k, e_y)


def test_lds_plans_give_the_same_bits(cuda, K, cases):
    from video_style_transfer_amd import _lib
    lib = _lib.load()
    prev = lib.vst_region_plan(0)
    try:
        for name in ("blocks_end_inside", "short_tail", "ten_heads"):
            lib.vst_region_plan(0)
            walk = launch(K, cases[name])
            for plan in (1, -1):   # everything up front; the default's choice
                lib.vst_region_plan(plan)
                assert torch.equal(bits(launch(K, cases[name])), bits(walk)), (name, plan)
    finally:
        lib.vst_region_plan(prev)


# ------------------------------------------------------------------------------------------ 2. exact cases
def one_hot(nimg, Nq, R, stripe):
    """([nimg*Nq] region of every row, fp32 [nimg*Nq, 4] one-hot weights, NaN past R): stripes of `stripe` rows."""
    region = ((torch.arange(Nq) // stripe) % R).repeat(nimg)
    w = torch.full((nimg * Nq, 4), NAN)
    w[:, :R] = torch.nn.functional.one_hot(region, R).float()
    return region, w


@pytest.mark.parametrize("name", ["blocks_end_inside", "long_prompt", "short_tail"])
def test_one_hot_rows_carry_spatial_attention_bits(cuda, K, cases, name):
    c = cases[name]
    region, w = one_hot(c["nimg"], c["Nq"], c["R"], 37 if c["Nq"] > 37 else 5)   # stripes cut through query blocks
    out = launch(K, c, ops=dict(c["ops"], wts=w.to(cuda)))
    want = torch.empty_like(out)
    for r in range(c["R"]):
        k = c["k"][:, r].reshape(-1, c["inner"]).to(BF16).to(cuda)   # this region's K/V, gathered contiguous
        v = c["v"][:, r].reshape(-1, c["inner"]).to(BF16).to(cuda)
        o = K.spatial_attention(c["ops"]["q"], k, v, c["nimg"], c["heads"], c["Nq"], c["Nk"], c["kv_div"])
        rows = (region == r).to(cuda)
        want[rows] = o[rows]
    assert torch.isfinite(out).all() and torch.equal(bits(out), bits(want))


def test_dead_region_costs_no_bit(cuda, K, cases):
    c = cases["blocks_end_inside"]   # R = 3
    g = torch.Generator().manual_seed(41)
    nimg, Nq, inner = c["nimg"], c["Nq"], c["inner"]
    # (a) region 1 has zero weight on every row and NaN K/V: the call without it, bit for bit
    w = soft_weights(nimg, Nq, 2, g)
    w3 = torch.full_like(w, NAN)
    w3[:, 0], w3[:, 1], w3[:, 2] = w[:, 0], 0.0, w[:, 1]
    k3, v3 = c["k"].clone(), c["v"].clone()
    k3[:, 1], v3[:, 1] = NAN, NAN
    with_dead = launch(K, c, ops=dict(q=c["ops"]["q"], k=k3.view(-1, inner).to(BF16).to(cuda),
                                      v=v3.view(-1, inner).to(BF16).to(cuda), wts=w3.to(cuda)))
    two = dict(q=c["ops"]["q"], k=c["k"][:, [0, 2]].reshape(-1, inner).to(BF16).to(cuda),
               v=c["v"][:, [0, 2]].reshape(-1, inner).to(BF16).to(cuda), wts=w.to(cuda))
    without = launch(K, c, ops=two, R=2)
    assert torch.isfinite(with_dead).all() and torch.equal(bits(with_dead), bits(without))
    # (b) region 1 dead on some rows only (stripes through the query blocks), NaN-free: those rows have the bits of
    # the call without it
    dead = ((torch.arange(Nq) // 23) % 2 == 0).repeat(nimg)
    w3b = w3.clone()
    w3b[:, :3] = torch.rand(nimg * Nq, 3, generator=g) + 0.1
    w3b[dead, 1] = 0.0
    w3b[:, :3] /= w3b[:, :3].sum(-1, keepdim=True)
    partly = launch(K, c, ops=dict(c["ops"], wts=w3b.to(cuda)))
    w2b = torch.full_like(w, NAN)
    w2b[:, 0], w2b[:, 1] = w3b[:, 0], w3b[:, 2]
    without_b = launch(K, c, ops=dict(two, wts=w2b.to(cuda)), R=2)
    d = dead.to(cuda)
    assert torch.equal(bits(partly[d]), bits(without_b[d]))
    assert not torch.equal(bits(partly[~d]), bits(without_b[~d]))   # (and the live rows do take from it)


def test_single_key_gives_the_value_row(cuda, K):
    heads, Nq, R, nimg, kv_div = 2, 150, 4, 4, 2
    region, w = one_hot(nimg, Nq, R, 29)
    c = make_case(heads, Nq, 1, R, nimg, 1, kv_div, seed=51, dev=cuda, wts=w)
    out = launch(K, c).cpu()
    want = c["v"][torch.arange(nimg).repeat_interleave(Nq) // kv_div, region, 0]   # [nimg*Nq, inner]
    assert torch.equal(bits(out), bits(want.to(BF16)))


# ------------------------------------------------------------------------------------------ 3. padding and views
def test_strided_views_in_poisoned_arenas(cuda, K, cases):
    c = cases["blocks_end_inside"]
    dense = launch(K, c)
    ops = c["ops"]
    assert torch.isnan(ops["wts"][:, c["R"]:]).all()   # columns >= R are NaN in every test here

    def arena(t, fill):
        a = torch.full((t.shape[0] + 2, t.shape[1] + 24), fill, dtype=BF16, device=cuda)
        v = a[1:-1, 8:8 + t.shape[1]]
        v.copy_(t)
        return a, v
    qa, qv = arena(ops["q"], NAN)
    ka, kv_ = arena(ops["k"], NAN)
    va, vv = arena(ops["v"], NAN)
    oa, ov = arena(torch.zeros_like(dense), 7.0)
    before = [t.clone() for t in (qa, ka, va, oa)]
    launch(K, c, ops=dict(q=qv, k=kv_, v=vv, wts=ops["wts"]), out=ov)
    assert torch.isfinite(ov).all() and torch.equal(bits(ov), bits(dense))
    for a, b in zip((qa, ka, va), before):
        assert torch.equal(bits(a), bits(b))
    ob = before[3]
    ob[1:-1, 8:8 + dense.shape[1]] = dense
    assert torch.equal(bits(oa), bits(ob))   # every byte outside the view is unchanged
    # the second half of the images from inside the arenas, every row of the other images NaN (q, weights, K/V) and
    # their O rows guarded
    half, hk = dense.shape[0] // 2, ops["k"].shape[0] // 2
    qa[:1 + half], ka[:1 + hk], va[:1 + hk] = NAN, NAN, NAN
    wts = ops["wts"].clone()
    wts[:half] = NAN
    oa.fill_(7.0)
    launch(K, c, ops=dict(q=qv[half:], k=kv_[hk:], v=vv[hk:], wts=wts[half:]), out=ov[half:], nimg=c["nimg"] // 2)
    ob.fill_(7.0)
    ob[1 + half:-1, 8:8 + dense.shape[1]] = dense[half:]
    assert torch.equal(bits(oa), bits(ob))


# ------------------------------------------------------------------------------------------ 4. invariance
def test_repeatable_and_independent_of_the_launch(cuda, K, cases):
    for name in ("blocks_end_inside", "ten_heads"):
        c = cases[name]
        full = launch(K, c)
        assert torch.equal(bits(full), bits(launch(K, c)))
        ops, half, hk = c["ops"], full.shape[0] // 2, c["ops"]["k"].shape[0] // 2
        if c["nkv"] > 1:   # the second half of the images alone, with its own token batches
            second = launch(K, c, ops=dict(q=ops["q"][half:], k=ops["k"][hk:], v=ops["v"][hk:], wts=ops["wts"][half:]),
                            nimg=c["nimg"] // 2)
        else:              # one token batch serves both images: the second image alone, kv_div 1
            second = launch(K, c, ops=dict(ops, q=ops["q"][half:], wts=ops["wts"][half:]), nimg=c["nimg"] // 2,
                            kv_div=1)
        assert torch.equal(bits(second), bits(full[half:])), name


# ------------------------------------------------------------------------------------------ 5. status codes
def test_status_codes_before_any_launch(cuda, K, cases):
    from video_style_transfer_amd import _lib
    c = cases["blocks_end_inside"]
    o = c["ops"]
    inner = c["inner"]
    O = torch.full((c["nimg"] * c["Nq"], inner), 3.0, dtype=BF16, device=cuda)
    good = dict(q=o["q"].data_ptr(), ldq=inner, k=o["k"].data_ptr(), v=o["v"].data_ptr(), ldkv=inner,
                w=o["wts"].data_ptr(), O=O.data_ptr(), ldo=inner, nimg=c["nimg"], heads=c["heads"], Nq=c["Nq"],
                Nk=c["Nk"], R=c["R"], kvd=c["kv_div"])

    def status(**kw):
        a = dict(good, **kw)
        return _lib.load().vst_region_attention(a["q"], a["ldq"], a["k"], a["v"], a["ldkv"], a["w"], a["O"], a["ldo"],
                                                a["nimg"], a["heads"], a["Nq"], a["Nk"], a["R"], a["kvd"], 0.125,
                                                torch.cuda.current_stream().cuda_stream)
    bad = [dict(q=None), dict(k=None), dict(v=None), dict(w=None), dict(O=None),
           dict(nimg=0), dict(heads=0), dict(Nq=0), dict(Nk=0), dict(R=0), dict(kvd=0), dict(Nq=-1), dict(R=5),
           dict(kvd=3),                                                         # nimg = 4 images over batches of 3
           dict(ldq=inner + 4), dict(ldkv=inner + 4), dict(ldo=inner + 4),      # no multiple of 8
           dict(ldq=inner - 8), dict(ldkv=inner - 8), dict(ldo=inner - 8),      # too short
           dict(q=good["q"] + 8), dict(k=good["k"] + 2), dict(v=good["v"] + 4), dict(O=good["O"] + 8),
           dict(w=good["w"] + 4),                                               # bases off 16 bytes
           dict(ldq=1 << 23, Nq=1 << 7), dict(ldkv=1 << 23), dict(ldo=1 << 23, Nq=1 << 7),   # past 2^31 - 1 bytes
           dict(Nk=1 << 22)]
    for kw in bad:
        assert status(**kw) == 1, kw
    torch.cuda.synchronize()
    assert (O == 3.0).all()
    # through the wrapper nothing is recorded either
    K.profile_launches(True)
    try:
        with pytest.raises(_lib.VstError, match="^region_attention: R "):
            launch(K, c, out=O, R=5)
        assert K.collect_launches() == []
    finally:
        K.profile_launches(False)
    assert (O == 3.0).all()
    assert status() == 0   # and the good call runs
    torch.cuda.synchronize()
    assert not (O == 3.0).all()


# ------------------------------------------------------------------------------------------ 6. processor
def test_processor_launches(cuda, K):
    from video_style_transfer_amd import attention_processor as AP
    from video_style_transfer_amd.attention_processor import AttnCall, Attention
    from video_style_transfer_amd.region_prompts import RegionPrompts
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
    holder.requires_grad_(False)
    proc = attn.processor
    x = (torch.randn(4, 256, 1280, device=cuda) * 0.5).to(BF16)
    enc = torch.randn(2, 77, 2048, device=cuda).to(BF16)
    other = torch.randn(2, 77, 2048, device=cuda).to(BF16)
    raw = torch.zeros(4, 2, 16, 16)
    raw[:, 0, :, :8] = 1.0    # the base prompt on the left half, the other prompt on the right
    raw[:, 1, :, 8:] = 1.0
    rp = RegionPrompts(torch.stack([enc, other], 1), raw, 2, [(16, 16)], cuda)
    call = AttnCall(regions=(rp, rp.table((16, 16))))
    proc(attn, x, encoder_hidden_states=enc, _vst=call)   # projects the regions' K/V
    o_reg, kinds = profiled(K, lambda: proc(attn, x, encoder_hidden_states=enc, _vst=call))
    assert kinds.count("region_attention") == 1 and "gemm_xattn" not in kinds and "spatial_attention" not in kinds, kinds
    # without regions: the fused launch, as before, whatever else the call carries
    proc(attn, x, encoder_hidden_states=enc)
    o_plain, kinds0 = profiled(K, lambda: proc(attn, x, encoder_hidden_states=enc, _vst=AttnCall(regions=None)))
    o_none, kinds1 = profiled(K, lambda: proc(attn, x, encoder_hidden_states=enc))
    assert kinds0 == kinds1 and "gemm_xattn" in kinds0 and "region_attention" not in kinds0, kinds0
    assert torch.equal(bits(o_plain), bits(o_none))
    # one-hot halves: each half of every image carries the two-launch path's bits for its own prompt
    orig = AP._cross_fusable
    AP._cross_fusable = lambda *a, **k: False
    try:
        o_base = proc(attn, x, encoder_hidden_states=enc)
        o_other = proc(attn, x, encoder_hidden_states=other)
    finally:
        AP._cross_fusable = orig
    left = (torch.arange(256, device=cuda) % 16 < 8)
    assert torch.equal(bits(o_reg[:, left]), bits(o_base[:, left]))
    assert torch.equal(bits(o_reg[:, ~left]), bits(o_other[:, ~left]))
    assert not torch.equal(bits(o_reg[:, ~left]), bits(o_base[:, ~left]))


# ------------------------------------------------------------------------------------------ 7. UNet
HW, FR = 16, 4


def region_inputs(cfg, enc, seed=61):
    """Two regions for the tiny model's B = 2 clips of 4 frames at 16 x 16: states [2, 2, 77, D] (slot 0 the call's
    own text) and raw weights [8, 2, 16, 16]: a soft vertical ramp that moves over the frames, a hard band of base
    only, a hard band of the other prompt only."""
    g = torch.Generator().manual_seed(seed)
    other = (torch.randn(2, 77, cfg.cross_attention_dim, generator=g) * 2.0).to(BF16).float()
    states = torch.stack([enc, other], 1)
    ramp = torch.linspace(0.0, 1.0, HW).view(1, 1, HW).expand(2 * FR, HW, HW).clone()
    ramp = (ramp + 0.1 * torch.arange(2 * FR).view(-1, 1, 1)).clamp(0, 1)
    ramp[:, :4] = 0.0
    ramp[:, 12:] = 1.0
    raw = torch.stack([1.0 - ramp, ramp], 1)
    return states, raw


def regional_oracle(OU, states, raw, extra=None):
    """oracle.unet.attention with every spatial attn2 replaced by the regional definition in fp32 (`extra`: a term
    added to the blend ahead of to_out, given (name, q, heads))."""
    import torch.nn.functional as Fn
    from video_style_transfer_amd.region_prompts import pooled_weights
    orig = OU.attention
    seen = []

    def sdpa(q, k, v, heads):
        B, N, C = q.shape

        def split(t):
            return t.reshape(B, -1, heads, C // heads).transpose(1, 2)
        return Fn.scaled_dot_product_attention(split(q), split(k), split(v)).transpose(1, 2).reshape(B, N, C)

    def attention(P, name, x, enc_, heads, lora):
        if enc_ is None or "motion_modules" in name:
            return orig(P, name, x, enc_, heads, lora)
        seen.append(name)

        def pr(n, t_):
            return OU.proj(P, f"{name}.{'to_out.0' if n == 'to_out' else n}", t_, lora)
        BF, N, _ = x.shape
        H = int(round(N ** 0.5))
        w = pooled_weights(raw, HW // H).reshape(BF, raw.shape[1], N)
        q = pr("to_q", x)
        out = 0
        for r in range(raw.shape[1]):
            e = states[:, r].repeat_interleave(BF // states.shape[0], 0)
            out = out + w[:, r].unsqueeze(-1) * sdpa(q, pr("to_k", e), pr("to_v", e), heads)
        if extra is not None:
            out = out + extra(name, q, heads, sdpa)
        return pr("to_out", out)
    return attention, seen


@pytest.fixture(scope="module")
def tiny(cuda):
    import oracle.unet as OU
    from test_parity_gpu import _setup
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser
    from video_style_transfer_amd.utils import build_unet
    cfg, sd, lat, enc, pooled, tids = _setup("tiny", FR, HW, seed=5, B=2)
    # the synthetic model's text path is weak: the spatial attn2 values times 4 (exact in bf16), for the plain runs
    # too, so that the regions move the output well clear of the error without sharpening any softmax
    sd = {k: (v * 4.0 if k.endswith("attn2.to_v.weight") and "motion_modules" not in k else v) for k, v in sd.items()}
    unet = build_unet(cfg, state_dict=sd, device=cuda)
    kw = dict(added_cond_kwargs={"text_embeds": pooled.to(cuda), "time_ids": tids.to(cuda)})
    t = torch.tensor([761.0, 761.0])
    plain = unet(lat.to(cuda), t.to(cuda), enc.to(cuda), **kw).sample.clone()
    ref0 = OU.unet_forward(sd, cfg.to_dict(), lat, t, enc, pooled, tids)
    d = dict(cfg=cfg, sd=sd, lat=lat, enc=enc, pooled=pooled, tids=tids, unet=unet, kw=kw, t=t, plain=plain, ref0=ref0,
             e0=rel(plain, ref0))
    den = AnimateDiffDenoiser(unet, FR, 8 * HW, 8 * HW, num_inference_steps=10, guidance_scale=7.5, device=cuda)
    den.set_prompt_embeds(enc[1:2], pooled[1:2], enc[0:1], pooled[0:1])
    den.init_latents(3)
    d["den_plain"] = den.run_steps(3).clone()
    return d


def _region_prompts(tiny, cuda):
    from video_style_transfer_amd.region_prompts import RegionPrompts, attention_levels
    states, raw = region_inputs(tiny["cfg"], tiny["enc"])
    return states, raw, RegionPrompts(states, raw, FR, attention_levels(tiny["unet"], (HW, HW)), cuda)


def test_unet_vs_oracle(cuda, K, tiny, monkeypatch):
    import oracle.unet as OU
    cfg, sd, lat, enc, pooled, tids, unet, kw, t = (tiny[k] for k in ("cfg", "sd", "lat", "enc", "pooled", "tids",
                                                                      "unet", "kw", "t"))
    states, raw, rp = _region_prompts(tiny, cuda)
    patched, seen = regional_oracle(OU, states, raw)
    monkeypatch.setattr(OU, "attention", patched)
    try:
        ref = OU.unet_forward(sd, cfg.to_dict(), lat, t, enc, pooled, tids)
    finally:
        monkeypatch.undo()
    n_attn2 = len(set(seen))
    out, kinds = profiled(K, lambda: unet(lat.to(cuda), t.to(cuda), enc.to(cuda), region_prompts=rp, **kw).sample)
    e, e0, moved = rel(out, ref), tiny["e0"], rel(ref, tiny["ref0"])
    print(f"tiny UNet + regional prompts: rel_l2 vs regional oracle {e:.3e}, plain forward vs plain oracle {e0:.3e} "
          f"(ratio {e / e0:.3f}); regional oracle vs plain oracle {moved:.3e}")
    assert kinds.count("region_attention") == n_attn2 > 0 and "gemm_xattn" not in kinds, kinds
    assert moved > 10 * e, (moved, e)   # the test cannot pass with the regions ignored
    assert torch.isfinite(out).all() and e <= 1.5 * e0, (e, e0)
    # without the option: the plain forward, bit for bit
    assert torch.equal(unet(lat.to(cuda), t.to(cuda), enc.to(cuda), **kw).sample, tiny["plain"])


def test_unet_with_ip_adapter(cuda, K, tiny, monkeypatch):
    import oracle.unet as OU
    from test_ip_adapter_gpu import image_tokens, ip_state_dict
    from video_style_transfer_amd.ip_adapter import ImagePrompt, ip_adapter_layers, load_ip_adapter, unload_ip_adapter
    cfg, sd, lat, enc, pooled, tids, unet, kw, t = (tiny[k] for k in ("cfg", "sd", "lat", "enc", "pooled", "tids",
                                                                      "unet", "kw", "t"))
    states, raw, rp = _region_prompts(tiny, cuda)
    ipsd = ip_state_dict(unet)
    tokens = image_tokens(cfg, 2)
    assert load_ip_adapter(unet, ipsd) > 0
    try:
        names = [k[:-len(".processor")] for k, _ in ip_adapter_layers(unet)]
        ipw = {n: (ipsd["ip_adapter"][f"{2 * i + 1}.to_k_ip.weight"], ipsd["ip_adapter"][f"{2 * i + 1}.to_v_ip.weight"])
               for i, n in enumerate(names)}

        def image_term(name, q, heads, sdpa):
            tok = tokens.repeat_interleave(q.shape[0] // 2, 0)
            wk, wv = ipw[name]
            return sdpa(q, tok @ wk.t(), tok @ wv.t(), heads)
        regional, _ = regional_oracle(OU, states, raw)
        both, _ = regional_oracle(OU, states, raw, extra=image_term)
        refs = []
        for fn in (regional, both):
            monkeypatch.setattr(OU, "attention", fn)
            try:
                refs.append(OU.unet_forward(sd, cfg.to_dict(), lat, t, enc, pooled, tids))
            finally:
                monkeypatch.undo()
        prompt = ImagePrompt(tokens.to(cuda), FR)
        out, kinds = profiled(K, lambda: unet(lat.to(cuda), t.to(cuda), enc.to(cuda), region_prompts=rp,
                                              image_prompt=prompt, **kw).sample)
    finally:
        unload_ip_adapter(unet)
    e, e0, moved = rel(out, refs[1]), tiny["e0"], rel(refs[1], refs[0])
    print(f"tiny UNet + regional prompts + image prompt: rel_l2 vs oracle {e:.3e}, plain forward {e0:.3e} "
          f"(ratio {e / e0:.3f}); the image term moves the regional oracle by {moved:.3e}")
    assert kinds.count("region_attention") == kinds.count("ip_attention_add") == len(names), kinds
    # with the image term ignored the error would be at least moved - (the regional error, within 1.5 e0): the gate
    # below cannot pass then
    assert moved > 2 * 1.5 * e0, (moved, e0)
    assert torch.isfinite(out).all() and e <= 1.5 * e0, (e, e0)


# ------------------------------------------------------------------------------------------ 8. denoiser
def _denoiser(tiny, cuda, use_graph=True):
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser
    den = AnimateDiffDenoiser(tiny["unet"], FR, 8 * HW, 8 * HW, num_inference_steps=10, guidance_scale=7.5,
                              device=cuda, use_graph=use_graph)
    den.set_prompt_embeds(tiny["enc"][1:2], tiny["pooled"][1:2], tiny["enc"][0:1], tiny["pooled"][0:1])
    return den


def test_denoiser_graph_equals_eager_and_new_masks_keep_the_graph(cuda, tiny):
    g = torch.Generator().manual_seed(71)
    emb = (torch.randn(1, 77, tiny["cfg"].cross_attention_dim, generator=g) * 2.0).to(BF16)
    left = torch.zeros(1, 1, HW, HW)
    left[..., :8] = 1.0
    sched = torch.linspace(0.0, 1.0, FR).view(1, FR, 1, 1).expand(1, FR, HW, HW)   # a prompt schedule over the clip

    def three(den):
        den.init_latents(3)
        return den.run_steps(3).clone()
    dg, de = _denoiser(tiny, cuda, True), _denoiser(tiny, cuda, False)
    for d in (dg, de):
        d.set_region_prompts(emb, left)
    og, oe = three(dg), three(de)
    assert dg.graph is not None and de.graph is None
    assert torch.isfinite(og).all() and torch.equal(og, oe) and not torch.equal(og, tiny["den_plain"])
    # new masks: the same graph object and buffers, a fresh eager denoiser's bits
    g0, rp = dg.graph, dg.region_prompts
    ptrs = [t.data_ptr() for t in rp.tables.values()] + [rp.states.data_ptr()]
    dg.set_region_prompts(emb, sched)
    og2 = three(dg)
    assert dg.graph is g0 and dg.region_prompts is rp
    assert ptrs == [t.data_ptr() for t in rp.tables.values()] + [rp.states.data_ptr()]
    fresh = _denoiser(tiny, cuda, False)
    fresh.set_region_prompts(emb, sched)
    assert torch.equal(og2, three(fresh)) and not torch.equal(og2, og)
    # other prompt states drop the captured step
    dg.set_region_prompts(emb * 0.5, sched)
    assert dg.graph is None
    # clearing is the run of a denoiser that never had regions
    dg.clear_region_prompts()
    assert dg.graph is None and dg.region_prompts is None
    assert torch.equal(three(dg), tiny["den_plain"])
