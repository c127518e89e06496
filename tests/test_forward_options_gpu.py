"""Every per-call option of UNetMotionModel.forward launches what it launched and computes the bits it computed when
tests/golden/forward_options.json was recorded (tools/record_forward_options.py, at the commit before ForwardOptions
and AttnCall replaced the keyword lists and the `_vst_*` side channel).  Equality is exact: the forward runs under
kernels.row_invariant and is bit-stable from run to run."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_forward_options",
                                               os.path.join(ROOT, "tools", "record_forward_options.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)


@pytest.fixture(scope="module")
def golden():
    with open(R.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def recorded(cuda):
    return R.record(cuda)   # all sets on one tiny model, once


@pytest.mark.parametrize("name", R.NAMES)
def test_option_set_launches_and_bits(golden, recorded, name):
    want, got = golden[name], recorded[name]
    assert len(got["launches"]) == len(want["launches"])
    for i, (g, w) in enumerate(zip(got["launches"], want["launches"])):
        assert g == w, f"{name}: launch {i} is {g}, recorded {w}"
    assert got["sha256"] == want["sha256"], name


def test_forward_equals_forward_tokens_under_resolved_options(cuda):
    """forward() is resolve (with the model's defaults) + the launches of forward_tokens(options=...)."""
    from test_parity_gpu import _setup
    from video_style_transfer_amd import kernels as K
    from video_style_transfer_amd.unet_motion import BF16, ForwardOptions, TemporalContext
    from video_style_transfer_amd.utils import build_unet
    cfg, sd, lat, enc, pooled, tids = _setup("tiny", R.FRAMES, R.HW)
    unet = build_unet(cfg, state_dict=sd, device=cuda)
    lat, enc = lat.to(cuda), enc.to(cuda)
    t = torch.tensor([R.TIMESTEP] * R.B, device=cuda)
    kw = dict(cross_frame=("first",), freeu=(0.9, 0.2, 1.3, 1.4), temporal_context=TemporalContext(2, 1))
    unet.enable_token_merging(ratio=0.5, use_rand=False)
    want = unet(lat, t, enc, added_cond_kwargs={"text_embeds": pooled.to(cuda), "time_ids": tids.to(cuda)}, **kw).sample
    B, C, F, h, w = lat.shape
    opts = ForwardOptions.resolve(unet, B, F, (h, w), None, lat, use_model_defaults=True, **kw)
    assert opts.token_merging is unet.token_merging
    emb = unet.embed(t, pooled.to(cuda, BF16), tids.to(cuda), B)
    x = torch.empty(B * F * h * w, C, dtype=BF16, device=cuda)
    K.pack_latents(lat.float().contiguous(), x)
    y = unet.forward_tokens(x, B, F, h, w, emb, enc.to(BF16).contiguous(), options=opts)
    assert torch.equal(y.view(B, F, h, w, -1).permute(0, 4, 1, 2, 3).contiguous().to(lat.dtype), want)
