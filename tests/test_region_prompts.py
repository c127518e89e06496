"""CPU tests of regional prompts: pooling and normalisation against the definition in fp64, base
completion, every refusal, the in-place rewrite, ForwardOptions.resolve on a meta-device model, the denoiser's
arguments with a stub shard, and the operand refusals of kernels.region_attention and of the library without a GPU
(the recorder pattern of test_operand_checks.py)."""
import dataclasses
import subprocess
import types

import pytest
import torch

from test_host import fake_device_tensor as dev

BF16, F32 = torch.bfloat16, torch.float32
B, FR, H, W = 2, 4, 8, 8
LEVELS = [(8, 8), (4, 4), (2, 2)]


def _vst_error():
    from video_style_transfer_amd._lib import VstError
    return VstError


# ------------------------------------------------------------------------------------------ weights
def test_pooling_and_normalisation_against_the_definition_fp64():
    from video_style_transfer_amd.region_prompts import RegionPrompts
    g = torch.Generator().manual_seed(0)
    R, rows = 3, B * FR
    raw = torch.rand(rows, R, H, W, generator=g)
    raw[:, 1, :4] = 0.0          # region 1 is absent from the upper half
    raw[:, 2, :, :2] = 0.0
    rp = RegionPrompts(torch.zeros(B, R, 5, 16), raw, FR, LEVELS)
    assert sorted(rp.tables) == sorted(LEVELS)
    for Hl, Wl in LEVELS:
        s = H // Hl
        cells = raw.double().view(rows, R, Hl, s, Wl, s).mean((3, 5))          # p_r: the mean over the s x s cell
        want = (cells / cells.sum(1, keepdim=True)).permute(0, 2, 3, 1).reshape(rows * Hl * Wl, R)
        t = rp.tables[(Hl, Wl)]
        assert t.dtype == F32 and tuple(t.shape) == (rows * Hl * Wl, 4)
        assert torch.allclose(t[:, :R].double(), want, rtol=0, atol=4e-7)
        assert (t[:, R:] == 0).all()
        assert ((t[:, :R] == 0) == (want == 0)).all()                           # a zero stays exactly zero
        assert torch.allclose(t[:, :R].sum(1), torch.ones(t.shape[0]), atol=1e-6)
    # hard 0 / 1 maps aligned to the deepest cells are one-hot at every level, exactly
    hard = torch.zeros(rows, 2, H, W)
    hard[:, 0, :, :4] = 1.0
    hard[:, 1, :, 4:] = 1.0
    rp2 = RegionPrompts(torch.zeros(B, 2, 5, 16), hard, FR, LEVELS)
    for t in rp2.tables.values():
        assert ((t[:, :2] == 0) | (t[:, :2] == 1)).all() and (t[:, :2].sum(1) == 1).all()


def test_base_completion():
    from video_style_transfer_amd.region_prompts import region_weights
    m = torch.zeros(2, 1, H, W)
    m[0, :, :, :4] = 1.0
    m[1, :, :4, :] = 0.5
    raw = region_weights(m, FR, (H, W))
    assert tuple(raw.shape) == (FR, 3, H, W) and raw.dtype == F32
    assert torch.equal(raw[:, 1:], m.permute(1, 0, 2, 3).expand(FR, 2, H, W))
    assert torch.equal(raw[:, 0], (1.0 - m.sum(0)).clamp_min(0.0).expand(FR, H, W))
    assert (raw[:, 0, :4, :4] == 0).all() and (raw[:, 0, 4:, 4:] == 1).all()   # 1 + 0.5 -> 0, nothing -> 1
    # bool masks, per-frame masks, a sequence of masks, an explicit base
    per_frame = torch.zeros(1, FR, H, W, dtype=torch.bool)
    per_frame[0, 2:] = True
    raw = region_weights(per_frame, FR, (H, W))
    assert torch.equal(raw[:, 1], per_frame[0].float()) and torch.equal(raw[:, 0], 1.0 - per_frame[0].float())
    raw = region_weights([m[0], m[1]], FR, (H, W), base_mask=torch.full((1, H, W), 0.25))
    assert (raw[:, 0] == 0.25).all() and torch.equal(raw[:, 1:], m.permute(1, 0, 2, 3).expand(FR, 2, H, W))
    assert tuple(region_weights(torch.zeros(0, 1, H, W), FR, (H, W)).shape) == (FR, 1, H, W)   # the base alone


def test_refusals():
    from video_style_transfer_amd.region_prompts import RegionPrompts, region_weights
    ok = torch.zeros(1, 1, H, W)
    for bad in (torch.full((1, 1, H, W), float("nan")), torch.full((1, 1, H, W), float("inf")),
                torch.full((1, 1, H, W), -0.5), torch.full((1, 1, H, W), 1.5),      # not finite, negative, above 1
                torch.zeros(4, 1, H, W),                                             # more than 3 masks
                torch.zeros(1, 3, H, W), torch.zeros(1, 1, H, W + 1), torch.zeros(1, H, W)):   # shapes
        with pytest.raises(ValueError, match="region masks"):
            region_weights(bad, FR, (H, W))
    with pytest.raises(ValueError, match="no weight in any region"):
        region_weights(ok, FR, (H, W), base_mask=torch.zeros(1, H, W))               # the sum is 0 somewhere
    with pytest.raises(ValueError, match="base_mask"):
        region_weights(ok, FR, (H, W), base_mask=torch.full((1, H, W), -1.0))
    with pytest.raises(ValueError, match="base_mask"):
        region_weights(ok, FR, (H, W), base_mask=torch.zeros(H, W))
    states, raw = torch.zeros(B, 2, 5, 16), torch.ones(B * FR, 2, H, W)

    def holed(v):
        t = raw.clone()
        t[3, :, 2, 5] = v
        return t
    for bad_raw, why in ((holed(float("nan")), "finite"), (holed(-1.0), ">= 0"), (holed(0.0), "no weight in any"),
                         (raw[:-1], "weights"), (raw[:, :1], "weights")):
        with pytest.raises(ValueError, match=why):
            RegionPrompts(states, bad_raw, FR, LEVELS)
    with pytest.raises(ValueError, match="regions"):
        RegionPrompts(torch.zeros(B, 5, 5, 16), torch.ones(B * FR, 5, H, W), FR, LEVELS)
    # h, w that the deepest level's factor does not divide
    with pytest.raises(ValueError, match="deepest attention level"):
        RegionPrompts(states, torch.ones(B * FR, 2, 6, 6), FR, [(6, 6), (3, 3), (2, 2)])
    with pytest.raises(ValueError, match="deepest attention level"):
        RegionPrompts(states, torch.ones(B * FR, 2, 8, 12), FR, [(8, 12), (4, 4)])


def test_in_place_rewrite():
    from video_style_transfer_amd.region_prompts import RegionPrompts
    raw = torch.ones(B * FR, 2, H, W)
    rp = RegionPrompts(torch.zeros(B, 2, 5, 16), raw, FR, LEVELS)
    ptrs = {k: t.data_ptr() for k, t in rp.tables.items()}
    sp, rows_view = rp.states.data_ptr(), rp.states_rows
    assert rp.version == 0 and (rp.tables[(4, 4)][:, :2] == 0.5).all()
    new = raw.clone()
    new[:, 1] = 3.0
    assert rp.set_weights(new) is rp and rp.version == 1
    assert {k: t.data_ptr() for k, t in rp.tables.items()} == ptrs
    assert (rp.tables[(2, 2)][:, 0] == 0.25).all() and (rp.tables[(8, 8)][:, 1] == 0.75).all()
    rp.set_states(torch.ones(B, 2, 5, 16))
    assert rp.version == 2 and rp.states.data_ptr() == sp and rp.states_rows is rows_view
    assert (rows_view == 1).all() and tuple(rows_view.shape) == (B * 2, 5, 16)   # the view the K/V cache keys on
    # a refused rewrite writes nothing
    before = {k: t.clone() for k, t in rp.tables.items()}
    bad = new.clone()
    bad[0, :, 0, 0] = 0.0
    for b in (bad, new[:1], torch.full_like(new, float("nan"))):
        with pytest.raises(ValueError):
            rp.set_weights(b)
    with pytest.raises(ValueError):
        rp.set_states(torch.ones(B, 2, 6, 16))
    assert rp.version == 2 and all(torch.equal(rp.tables[k], before[k]) for k in before)


# ------------------------------------------------------------------------------------------ ForwardOptions
def _model(**cfg_kw):
    from video_style_transfer_amd.config import UNetMotionConfig
    from video_style_transfer_amd.unet_motion import UNetMotionModel
    cfg = dataclasses.replace(UNetMotionConfig.tiny(), **cfg_kw)
    with torch.device("meta"):
        model = UNetMotionModel(cfg)
    return model.requires_grad_(False)


@pytest.fixture(scope="module")
def model():
    return _model()


def _x(F=FR):
    return torch.empty(B * F * H * W, 4, dtype=BF16, device="meta")


def _enc(L=5, D=256):
    return torch.empty(B, L, D, dtype=BF16, device="meta")


def _rp(model, rows=B * FR, frames=FR, L=5, D=256, levels=None, R=2):
    from video_style_transfer_amd.region_prompts import RegionPrompts, attention_levels
    levels = attention_levels(model, (H, W)) if levels is None else levels
    return RegionPrompts(torch.zeros(rows // frames, R, L, D), torch.ones(rows, R, H, W), frames, levels)


def test_attention_levels(model):
    from video_style_transfer_amd.region_prompts import attention_levels
    assert attention_levels(model, (H, W)) == [(4, 4), (2, 2)]     # the tiny model attends after one and two halvings
    assert attention_levels(model, (16, 24)) == [(8, 12), (4, 6)]


def test_resolve_accepts_and_refuses(model):
    from video_style_transfer_amd.lora_gate import LoraGate
    from video_style_transfer_amd.unet_motion import ForwardOptions

    def resolve(rp, enc=_enc(), **given):
        return ForwardOptions.resolve(model, B, FR, (H, W), None, _x(), use_model_defaults=False, enc=enc,
                                      region_prompts=rp, **given)
    rp = _rp(model)
    assert resolve(rp).region_prompts is rp
    assert ForwardOptions.resolve(model, B, FR, (H, W), None, _x(), use_model_defaults=False).region_prompts is None
    E = _vst_error()
    with pytest.raises(E, match=r"region_prompts: 4 rows, expected B \* F = 8"):
        resolve(_rp(model, rows=4, frames=2))
    with pytest.raises(E, match=r"region_prompts: no weight table for the 2 x 2 attention level"):
        resolve(_rp(model, levels=[(4, 4)]))
    with pytest.raises(E, match=r"region_prompts: states of 7 x 256 per region, encoder_hidden_states of 5 x 256"):
        resolve(_rp(model, L=7))
    with pytest.raises(E, match=r"region_prompts: states of 5 x 128 per region"):
        resolve(_rp(model, D=128))
    with pytest.raises(E, match=r"region_prompts: the call has no encoder_hidden_states"):
        resolve(rp, enc=None)
    with pytest.raises(E, match=r"region_prompts: expected a region_prompts.RegionPrompts, got Tensor"):
        resolve(torch.zeros(1))
    with pytest.raises(E, match=r"region_prompts: not together with a lora_gate") as e:
        resolve(rp, lora_gate=LoraGate(B * FR, "cpu"))
    assert e.traceback[-1].name == "refuse_lora_gate"           # the one shared function
    # forward_tokens refuses the same way, before any launch
    with pytest.raises(E, match=r"region_prompts: 4 rows") as e2:
        model.forward_tokens(_x(), B, FR, H, W, None, _enc(), region_prompts=_rp(model, rows=4, frames=2))
    with pytest.raises(TypeError, match="region_prompt"):        # a misspelt option is still a TypeError
        ForwardOptions.resolve(model, B, FR, (H, W), use_model_defaults=False, region_prompt=rp)
    with pytest.raises(TypeError, match="region_prompt"):
        model.forward_tokens(_x(), B, FR, H, W, None, _enc(), region_prompt=rp)


def test_the_new_check_runs_after_the_existing_ones(model):
    """Two faults at once: every existing refusal wins over the regional one, so the single-fault order stands."""
    from video_style_transfer_amd.lora_gate import LoraGate
    from video_style_transfer_amd.unet_motion import ForwardOptions
    bad = _rp(model, rows=4, frames=2)
    E = _vst_error()
    existing = [(dict(cross_frame=(5,)), E, "cross_frame: source frame 5"),
                (dict(freeu=(0.9, float("inf"), 1.3, 1.4)), ValueError, "freeu s2"),
                (dict(token_merging="half"), E, "token_merging: 'half'"),
                (dict(lora_gate=LoraGate(3, "cpu")), E, "lora_gate: 3 rows")]
    for given, exc, msg in existing:
        with pytest.raises(exc, match=msg):
            ForwardOptions.resolve(model, B, FR, (H, W), None, _x(), use_model_defaults=False, enc=_enc(),
                                   region_prompts=bad, **given)
    with pytest.raises(E, match="exceeds the motion modules"):
        ForwardOptions.resolve(model, B, 40, (H, W), None, _x(40), use_model_defaults=False, enc=_enc(),
                               region_prompts=bad)


def test_direct_processor_call_with_a_gate_refuses_through_the_shared_function(model):
    from video_style_transfer_amd.attention_processor import AnimateDiffAttnProcessor2_0, AttnCall, Attention
    from video_style_transfer_amd.lora_gate import LoraGate
    attn = Attention(64, 256, 1, 64).requires_grad_(False)
    rp = _rp(model, rows=2, frames=1)
    call = AttnCall(regions=(rp, rp.table((4, 4))), lora_gate=LoraGate(2, "cpu"))
    with pytest.raises(_vst_error(), match="region_prompts: not together with a lora_gate") as e:
        AnimateDiffAttnProcessor2_0()(attn, torch.zeros(2, 16, 64, dtype=BF16), torch.zeros(2, 5, 256, dtype=BF16),
                                      _vst=call)
    assert e.traceback[-1].name == "refuse_lora_gate"


# ------------------------------------------------------------------------------------------ the denoiser's arguments
def _denoiser(num_clips=1, frames=4, shard=None, guidance=7.5, prompt=True):
    """A denoiser on the CPU around a meta-device model (its levels are read, nothing launches)."""
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser
    den = AnimateDiffDenoiser(_model(), frames, 8 * H, 8 * W, num_inference_steps=10, guidance_scale=guidance,
                              device="cpu", use_graph=False, shard=shard, num_clips=num_clips)
    if prompt:
        g = torch.Generator().manual_seed(1)
        den.set_prompt_embeds(torch.randn(1, 5, 256, generator=g), torch.randn(1, 64, generator=g),
                              torch.randn(1, 5, 256, generator=g), torch.randn(1, 64, generator=g))
    return den


def _masks(n=1, frames=1):
    m = torch.zeros(n, frames, H, W)
    for i in range(n):
        m[i, :, :, 2 * i + 2:2 * i + 4] = 1.0
    return m


def test_set_region_prompts_accepted_forms_and_cfg_order():
    den = _denoiser(num_clips=2, frames=4)
    cond, uncond = den.enc[2:], den.enc[:2]
    emb = torch.randn(2, 5, 256, generator=torch.Generator().manual_seed(2)).to(BF16)
    den.graph = "captured"
    den.set_region_prompts(emb, _masks(2))
    rp = den.region_prompts
    assert den.graph is None and rp.R == 3 and rp.rows == 2 * 2 * 4 and rp.frames == 4
    assert den._options()["region_prompts"] is rp
    # UNet batch order [uncond clip 0, uncond clip 1, cond clip 0, cond clip 1]
    assert tuple(rp.states.shape) == (4, 3, 5, 256)
    assert torch.equal(rp.states[2:, 0], cond) and torch.equal(rp.states[2:, 1:], emb.expand(2, 2, 5, 256))
    assert torch.equal(rp.states[:2], uncond.unsqueeze(1).expand(2, 3, 5, 256))   # uncond states in every slot
    for (Hl, Wl), t in rp.tables.items():
        t = t.view(2, 2, 4, Hl, Wl, 4)                                            # [copy, clip, frame, Y, X, 4]
        assert (t[0, ..., 0] == 1).all() and (t[0, ..., 1:] == 0).all()           # the uncond rows are (1, 0, 0, 0)
        assert (t[1, ..., 3] == 0).all() and torch.equal(t[1, 0], t[1, 1])
    t = rp.tables[(4, 4)].view(2, 2, 4, 4, 4, 4)[1, 0, 0]                         # columns 2-3 and 4-5 of 8: cells 1, 2
    assert torch.equal(t[0, :, :3], torch.tensor([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [1.0, 0, 0]]))
    # new masks with the same embeds: the same object and buffers, the capture kept
    den.graph = "captured"
    sched = torch.linspace(0, 1, 4).view(1, 4, 1, 1).expand(2, 4, H, W) * 0.5
    den.set_region_prompts(emb, sched)
    assert den.graph == "captured" and den.region_prompts is rp and rp.version == 1
    t = rp.tables[(2, 2)].view(2, 2, 4, 2, 2, 4)[1, 1]
    assert torch.allclose(t[:, 0, 0, 1], torch.linspace(0, 0.5, 4)) and torch.allclose(t[:, 0, 0, 0], 1 - sched[0, :, 0, 0] * 2)
    # other embeds, another n, a new prompt, clear: the capture goes
    den.set_region_prompts(emb * 2, sched)
    assert den.graph is None and den.region_prompts is rp
    den.graph = "captured"
    den.set_region_prompts(emb[:1], _masks(1))
    assert den.graph is None and den.region_prompts is not rp and den.region_prompts.R == 2
    rp = den.region_prompts
    new_cond = torch.ones(1, 5, 256)
    den.set_prompt_embeds(new_cond, torch.zeros(1, 64), torch.zeros(1, 5, 256), torch.zeros(1, 64))
    assert den.region_prompts is rp and (rp.states[2:, 0] == 1).all() and (rp.states[:2] == 0).all()
    assert torch.equal(rp.states[2:, 1], emb[:1].expand(2, 5, 256))               # region 0 follows the prompt
    den.graph = "captured"
    den.clear_region_prompts()
    assert den.graph is None and den.region_prompts is None and den._options()["region_prompts"] is None
    den.graph = "captured"
    den.clear_region_prompts()
    assert den.graph == "captured"
    one = _denoiser(guidance=1.0)                                                 # no CFG: one copy
    one.set_region_prompts(emb[:1], _masks(1), base_mask=torch.full((1, H, W), 0.5))
    assert one.region_prompts.rows == 4 and tuple(one.region_prompts.states.shape) == (1, 2, 5, 256)
    assert torch.allclose(one.region_prompts.tables[(4, 4)][:, 0].view(4, 4, 4)[0, 0],
                          torch.tensor([1.0, 1 / 3, 1.0, 1.0]))


def test_frame_shard_slicing_of_the_tables():
    stub = types.SimpleNamespace(world=1, rank=0, local_frames=lambda F: (F // 2, F // 2))
    emb = torch.zeros(1, 5, 256)
    m = torch.rand(1, 4, H, W, generator=torch.Generator().manual_seed(3))
    whole = _denoiser(num_clips=2, frames=4)
    whole.set_region_prompts(emb, m)
    for given in (m, m[:, 2:]):
        half = _denoiser(num_clips=2, frames=4, shard=stub)
        assert (half.F, half.f0) == (2, 2)
        half.set_region_prompts(emb, given)
        assert half.region_prompts.rows == 2 * 2 * 2
        for lv, t in half.region_prompts.tables.items():
            want = whole.region_prompts.tables[lv].view(4, 4, -1, 4)[:, 2:]
            assert torch.equal(t.view(4, 2, -1, 4), want)
    with pytest.raises(ValueError, match="frames"):
        _denoiser(num_clips=2, frames=4, shard=stub).set_region_prompts(emb, m[:, :3])


def test_refusals_leave_state_alone_and_gates_exclude_regions_in_both_orders():
    den = _denoiser(num_clips=1, frames=4)
    emb = torch.zeros(2, 5, 256)
    den.set_region_prompts(emb, _masks(2))
    rp = den.region_prompts
    tabs, st, ver = {k: t.clone() for k, t in rp.tables.items()}, rp.states.clone(), rp.version
    den.graph = "captured"
    bad = [(emb, _masks(1)), (emb, _masks(2, 3)), (emb[0], _masks(2)), (torch.zeros(4, 5, 256), _masks(4)),
           (torch.zeros(2, 6, 256), _masks(2)), (emb, torch.full((2, 1, H, W), float("nan"))),
           (emb, -_masks(2)), (emb, _masks(2)[..., :6])]
    for e, m in bad:
        with pytest.raises(ValueError):
            den.set_region_prompts(e, m)
    with pytest.raises(ValueError, match="no weight in any region"):
        den.set_region_prompts(emb, _masks(2), base_mask=torch.zeros(1, H, W))
    with pytest.raises(_vst_error(), match="region_prompts: not together with a lora_gate") as e1:
        den.set_lora_gates(style=0.5)                           # gates after regions
    assert e1.traceback[-1].name == "refuse_lora_gate"
    with pytest.raises(ValueError, match="prompt states"):
        den.set_prompt_embeds(torch.zeros(1, 6, 256), torch.zeros(1, 64), torch.zeros(1, 6, 256), torch.zeros(1, 64))
    assert den.region_prompts is rp and rp.version == ver and torch.equal(rp.states, st) and den.lora_gate is None
    assert all(torch.equal(rp.tables[k], tabs[k]) for k in tabs) and den.graph == "captured"
    assert den.enc.shape[1] == 5
    gated = _denoiser()
    gated.set_lora_gates(style=0.5)
    table = gated.lora_gate.table.clone()
    with pytest.raises(_vst_error(), match="region_prompts: not together with a lora_gate") as e2:
        gated.set_region_prompts(emb, _masks(2))                # regions after gates
    assert e2.traceback[-1].name == "refuse_lora_gate"
    assert gated.region_prompts is None and torch.equal(gated.lora_gate.table, table)
    with pytest.raises(ValueError, match="set_prompt_embeds"):
        _denoiser(prompt=False).set_region_prompts(emb, _masks(2))


# ------------------------------------------------------------------------------------------ wrapper and library
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
    # 4 images of 16 rows, 2 heads, 2 token batches (kv_div 2) of 3 regions of 5 keys
    return dict(q=dev(64, 128), k=dev(30, 128), v=dev(30, 128), wts=dev(64, 4, dtype=F32), out=dev(64, 128))


def _run(K, o, **kw):
    args = dict(nimg=4, heads=2, Nq=16, Nk=5, R=3, kv_div=2)
    args.update(kw)
    return K.region_attention(o["q"], o["k"], o["v"], o["wts"], out=o["out"], **args)


BAD_OPERANDS = {
    "host q": ("q", lambda: torch.zeros(64, 128, dtype=BF16)),
    "fp32 q": ("q", lambda: dev(64, 128, dtype=F32)),
    "short q": ("q", lambda: dev(48, 128)),
    "narrow q": ("q", lambda: dev(64, 64)),
    "q odd stride": ("q", lambda: dev(64, 132)[:, :128]),
    "q misaligned": ("q", lambda: dev(65, 136).reshape(-1)[4:4 + 64 * 136].view(64, 136)[:, :128]),
    "host k": ("k", lambda: torch.zeros(30, 128, dtype=BF16)),
    "short k": ("k", lambda: dev(20, 128)),
    "narrow k": ("k", lambda: dev(30, 64)),
    "short v": ("v", lambda: dev(20, 128)),
    "fp32 v": ("v", lambda: dev(30, 128, dtype=F32)),
    "v other stride": ("k and v", lambda: dev(30, 256)[:, :128]),
    "short out": ("out", lambda: dev(32, 128)),
    "narrow out": ("out", lambda: dev(64, 64)),
    "fp32 out": ("out", lambda: dev(64, 128, dtype=F32)),
    "out odd stride": ("out", lambda: dev(64, 132)[:, :128]),
    "bf16 wts": ("wts", lambda: dev(64, 4, dtype=BF16)),
    "short wts": ("wts", lambda: dev(60, 4, dtype=F32)),
    "three-column wts": ("wts", lambda: dev(64, 3, dtype=F32)),
    "strided wts": ("wts", lambda: dev(64, 8, dtype=F32)[:, :4]),
    "host wts": ("wts", lambda: torch.zeros(64, 4, dtype=F32)),
}


@pytest.mark.parametrize("label", sorted(BAD_OPERANDS))
def test_wrapper_refuses_bad_operand(K, label):
    arg, make = BAD_OPERANDS[label]
    o = _good()
    o["v" if arg == "k and v" else arg] = make()
    with pytest.raises(K._lib.VstError, match=f"^region_attention: {arg} "):
        _run(K, o)
    assert K.calls == []


@pytest.mark.parametrize("kw,arg", [(dict(R=0), "R"), (dict(R=5), "R"), (dict(heads=0), "nimg, heads"),
                                    (dict(Nq=0), "nimg, heads"), (dict(Nk=0), "nimg, heads"),
                                    (dict(kv_div=0), "nimg, heads"), (dict(nimg=0), "nimg, heads"),
                                    (dict(kv_div=3), "nimg"), (dict(R=4), "k"), (dict(Nk=6), "k")])
def test_wrapper_refuses_bad_scalars(K, kw, arg):
    with pytest.raises(K._lib.VstError, match=f"^region_attention: {arg}"):
        _run(K, _good(), **kw)
    assert K.calls == []


def test_wrapper_good_operands_reach_the_library_once(K):
    o = _good()
    assert _run(K, o) is o["out"]
    assert len(K.calls) == 1
    name, a = K.calls[0]
    assert name == "vst_region_attention"
    # (q, ldq, Kt, Vt, ldkv, wts, O, ldo, nimg, heads, Nq, Nk, R, kv_div, scale, stream)
    assert a[0] == o["q"].data_ptr() and a[2] == o["k"].data_ptr() and a[3] == o["v"].data_ptr()
    assert a[5] == o["wts"].data_ptr() and a[6] == o["out"].data_ptr()
    assert (a[1], a[4], a[7]) == (128, 128, 128) and a[8:15] == (4, 2, 16, 5, 3, 2, 0.125)
    # strided column views are operands like any other, and the output may be left to the wrapper
    K.calls.clear()
    kv = dev(30, 256)
    o.update(q=dev(64, 256)[:, 128:], k=kv[:, :128], v=kv[:, 128:])
    _run(K, o)
    assert len(K.calls) == 1 and (K.calls[0][1][1], K.calls[0][1][4]) == (256, 256)


def test_library_exports_and_refuses_without_gpu():
    """The status codes of vst_region_attention come before any launch, so they can be asked for without a GPU."""
    from video_style_transfer_amd import _lib
    assert "vst_region_attention" in _lib.exported_symbols() and "vst_region_plan" in _lib.exported_symbols()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    assert " T vst_region_attention\n" in nm.stdout and " T vst_region_plan\n" in nm.stdout
    lib = _lib.load()
    Q, Kt, Vt, Wt, O = 4096, 8192, 16384, 32768, 65536  # never dereferenced: every call below is refused on the host

    def call(q=Q, ldq=128, k=Kt, v=Vt, ldkv=128, w=Wt, o=O, ldo=128, nimg=4, heads=2, Nq=16, Nk=5, R=3, kvd=2):
        return lib.vst_region_attention(q, ldq, k, v, ldkv, w, o, ldo, nimg, heads, Nq, Nk, R, kvd, 0.125, None)
    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(w=None), dict(o=None), dict(nimg=0), dict(heads=0),
               dict(Nq=0), dict(Nk=0), dict(R=0), dict(kvd=0), dict(nimg=-4), dict(R=5), dict(kvd=3),
               dict(ldq=132), dict(ldkv=132), dict(ldo=132), dict(ldq=120), dict(ldkv=120), dict(ldo=120),
               dict(q=Q + 8), dict(k=Kt + 2), dict(v=Vt + 4), dict(o=O + 8), dict(w=Wt + 4),
               dict(nimg=1 << 12, Nq=1 << 12, kvd=1), dict(Nk=1 << 22), dict(ldq=1 << 25), dict(ldo=1 << 25),
               dict(ldkv=1 << 26)):
        assert call(**kw) == 1, kw
    prev = lib.vst_region_plan(1)
    assert prev in (-1, 0, 1) and lib.vst_region_plan(prev) == 1
