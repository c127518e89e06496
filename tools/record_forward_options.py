"""Record what UNetMotionModel.forward launches and computes under each per-call option.

For every option set below, on the tiny model and the inputs of tests/test_parity_gpu._setup("tiny", 4, 16) at one
timestep: the launch list [(kind, kernel symbol, shape)] of kernels.profile_launches and the sha256 of the output's
bytes.  Written to tests/golden/forward_options.json, which tests/test_forward_options_gpu.py compares a run with, bit
for bit (the forward runs under kernels.row_invariant and is bit-stable from run to run).  Only `forward(...)` and its
public keywords are used, so the script records any commit.

Every set runs twice and the second run is recorded: the first fills the per-clip caches (text K/V, folded image
keys, folded upsample weights), whose launches depend on what ran before.

    python tools/record_forward_options.py [--out tests/golden/forward_options.json]
"""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, "tests", "golden", "forward_options.json")
B, FRAMES, HW, TIMESTEP = 2, 4, 16, 761.0
NAMES = ("none", "cross_frame_first", "cross_frame_first_prev_adain_qkv", "temporal_context", "lora_gate", "freeu",
         "token_merging", "image_prompt")


def option_sets(cfg, device) -> dict:
    """name -> the keywords of forward() for that set (`image_prompt` needs the IP-Adapter processors loaded)."""
    from test_ip_adapter_gpu import image_tokens
    from video_style_transfer_amd.ip_adapter import ImagePrompt
    from video_style_transfer_amd.lora_gate import LoraGate
    from video_style_transfer_amd.unet_motion import CrossFrameAttention, TemporalContext
    gate = LoraGate(B * FRAMES, device).set([1.0, 0.5, 0.0, 1.5, 1.0, 0.25, 2.0, 0.75],
                                            [0.0, 1.0, 1.25, 0.5, 1.0, 1.0, 0.0, -0.5])
    sets = dict(
        none={},
        cross_frame_first=dict(cross_frame=("first",)),
        cross_frame_first_prev_adain_qkv=dict(cross_frame=CrossFrameAttention(("first", "prev"), adain="qkv")),
        temporal_context=dict(temporal_context=TemporalContext(2, 1)),
        lora_gate=dict(lora_gate=gate),
        freeu=dict(freeu=(0.9, 0.2, 1.3, 1.4)),
        token_merging=dict(token_merging=dict(ratio=0.5, use_rand=False, merge_mlp=True)),
        image_prompt=dict(image_prompt=ImagePrompt(image_tokens(cfg, B).to(device), FRAMES)),
    )
    assert tuple(sets) == NAMES
    return sets


def record(device) -> dict:
    """name -> {"launches": [[kind, symbol, shape], ...], "sha256": hex} for every option set."""
    from test_ip_adapter_gpu import ip_state_dict
    from test_parity_gpu import _setup
    from video_style_transfer_amd import kernels as K
    from video_style_transfer_amd.ip_adapter import load_ip_adapter, unload_ip_adapter
    from video_style_transfer_amd.utils import build_unet
    cfg, sd, lat, enc, pooled, tids = _setup("tiny", FRAMES, HW)
    unet = build_unet(cfg, state_dict=sd, device=device)
    lat, enc = lat.to(device), enc.to(device)
    t = torch.tensor([TIMESTEP] * B, device=device)
    cond = dict(added_cond_kwargs={"text_embeds": pooled.to(device), "time_ids": tids.to(device)})
    out = {}
    for name, kw in option_sets(cfg, device).items():
        if name == "image_prompt":  # (the last set: only this one runs with the processors)
            load_ip_adapter(unet, ip_state_dict(unet))
        try:
            unet(lat, t, enc, **cond, **kw)
            K.profile_launches(True)
            try:
                y = unet(lat, t, enc, **cond, **kw).sample
                launches = [[r[0], r[1], r[5]] for r in K.collect_launches()]
            finally:
                K.profile_launches(False)
        finally:
            if name == "image_prompt":
                unload_ip_adapter(unet)
        raw = y.contiguous().cpu().view(torch.uint8).numpy().tobytes()
        out[name] = {"launches": json.loads(json.dumps(launches)), "sha256": hashlib.sha256(raw).hexdigest()}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    rec = record(torch.device("cuda:0"))
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    for name in NAMES:
        print(f"{name}: {len(rec[name]['launches'])} launches, sha256 {rec[name]['sha256'][:16]}")


if __name__ == "__main__":
    main()
