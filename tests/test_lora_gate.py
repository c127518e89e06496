"""Per-frame content / style strength, host side, no GPU: the key of every u column that build_ops
records, the gate tables a LoraGate expands from them, what set_lora_gates accepts and refuses, how it slices a
frame shard's rows, and the argument checks of the three new C entries."""
import types

import pytest
import torch

from video_style_transfer_amd import _lib
from video_style_transfer_amd.lora_gate import LoraGate
from video_style_transfer_amd.lora_linear import (LoRACompatibleLinear, LoRALinearLayer, build_ops, gate_operands,
                                                  run_ops)
from video_style_transfer_amd.unziplora_linear_layer import UnZipLoRALinearLayerInfer

R = 8


def _unzip_linear(n_in=64, n_out=48):
    lin = LoRACompatibleLinear(n_in, n_out, bias=False)
    lin.set_lora_layer(UnZipLoRALinearLayerInfer(n_in, n_out, rank=R, lora_matrix_key=["content", "style"]))
    return lin.requires_grad_(False)


C8, S8, U = (0,) * R, (1,) * R, -1


@pytest.mark.parametrize("forward_type,masked,per_layer", [
    ("both", None, C8 + S8),
    ("content", None, C8),
    ("style", None, S8),
    ("both", "style", C8),     # a masked key contributes no columns
    ("both", "content", S8),
])
@pytest.mark.parametrize("nproj", [1, 3])
def test_build_ops_records_column_keys(forward_type, masked, per_layer, nproj):
    lins = [_unzip_linear() for _ in range(nproj)]
    for lin in lins:
        lin.lora_layer.set_forward(forward_type)
        if masked:
            lin.lora_layer.set_layer_mask(masked, True)
    ops = build_ops(lins, 1.0, mode="fused")
    P = ops.a.shape[0]
    real = per_layer * nproj
    assert P % 32 == 0 and len(ops.keys) == P
    assert ops.keys == real + (U,) * (P - len(real))
    assert ops.gated and not ops.folded
    assert (ops.gn, ops.gr) == (48, len(per_layer))
    # the expanded table: column c is the content or the style gate of the row, 1 where the column has no key
    gate = LoraGate(3).set(content=[0.5, 2.0, -1.0], style=[0.25, 0.0, 3.0])
    t = gate.expanded(ops.keys)
    assert t.shape == (3, P) and t.dtype == torch.float32
    want = torch.ones(3, P)
    for c, k in enumerate(ops.keys):
        if k >= 0:
            want[:, c] = gate.table[:, k]
    assert torch.equal(t, want)
    assert gate.expanded(ops.keys) is t  # one buffer per layout
    g, div = gate_operands(ops, gate, 3 * 10)
    assert g is t and div == 10
    with pytest.raises(_lib.VstError):
        gate_operands(ops, gate, 31)  # rows no multiple of the gate rows


def test_plain_lora_and_no_lora_columns_are_ungated():
    lin = LoRACompatibleLinear(64, 48, bias=False)
    lin.set_lora_layer(LoRALinearLayer(64, 48, rank=4))
    lin.requires_grad_(False)
    ops = build_ops([lin], 1.0, mode="fused")
    assert ops.keys == (U,) * 32 and not ops.gated
    gate = LoraGate(2).set(0.0, 0.0)
    assert gate_operands(ops, gate, 20) == (None, 1)  # runs as without a gate
    plain = build_ops([LoRACompatibleLinear(64, 48).requires_grad_(False)], 1.0, mode="fused")
    assert plain.keys == () and gate_operands(plain, gate, 20) == (None, 1)
    # a mix: UnZipLoRA columns keep their keys, the plain LoRA's are -1
    both = build_ops([_unzip_linear(), lin], 1.0, mode="fused")
    assert both.keys == C8 + S8 + (U,) * 4 + (U,) * 12 and both.gr == 0


def test_expanded_tables_are_rewritten_in_place():
    gate = LoraGate(4)
    keys = C8 + S8 + (U,) * 16
    t = gate.expanded(keys)
    ptr, v0 = t.data_ptr(), gate.version
    assert torch.equal(t, torch.ones(4, 32))
    gate.set(content=0.5, style=[0.0, 1.0, 2.0, 3.0])
    assert gate.version == v0 + 1 and gate.expanded(keys).data_ptr() == ptr
    assert torch.equal(t[:, :8], torch.full((4, 8), 0.5))
    assert torch.equal(t[:, 8:16], torch.tensor([0.0, 1.0, 2.0, 3.0])[:, None].expand(4, 8))
    assert torch.equal(t[:, 16:], torch.ones(4, 16))
    before, tab = t.clone(), gate.table.clone()
    for bad in ([1.0, 2.0], float("nan"), [1.0, float("inf"), 0.0, 0.0], torch.ones(2, 2)):
        with pytest.raises(ValueError):
            gate.set(content=1.0, style=bad)
        with pytest.raises(ValueError):
            gate.set(content=bad)
    assert torch.equal(t, before) and torch.equal(gate.table, tab) and gate.version == v0 + 1
    with pytest.raises(ValueError):
        gate.expanded((0, 1, 2, 0))
    with pytest.raises(ValueError):
        gate.expanded((0, 1, 0))  # not a multiple of 4 columns


def test_folded_mode_refuses_a_gate():
    lin = _unzip_linear()
    ops = build_ops([lin], 1.0, mode="folded")
    assert ops.a is None and ops.folded and ops.keys == ()
    gate = LoraGate(2)
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    with pytest.raises(_lib.VstError, match="folded"):
        run_ops(x, ops, gate=gate)
    with pytest.raises(_lib.VstError, match="folded"):
        gate_operands(ops, gate, 4)


# ----------------------------------------------------------------------------- the denoiser's gate arguments
def _denoiser(num_clips=1, frames=4, shard=None, guidance=7.5):
    """A denoiser on the CPU around a module that only carries the config: nothing here launches."""
    from video_style_transfer_amd.config import UNetMotionConfig
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser
    unet = torch.nn.Module()
    unet.config = UNetMotionConfig.tiny()
    return AnimateDiffDenoiser(unet, frames, 128, 128, num_inference_steps=10, guidance_scale=guidance, device="cpu",
                               use_graph=False, shard=shard, num_clips=num_clips)


def test_set_lora_gates_accepted_forms_and_cfg_order():
    den = _denoiser(num_clips=2, frames=4)
    assert den.lora_gate is None
    den.graph = "captured"
    den.set_lora_gates(style=0.6)
    assert den.graph is None  # the first set drops the captured step
    gate = den.lora_gate
    assert gate.rows == 2 * 2 * 4
    assert torch.equal(gate.table, torch.tensor([1.0, 0.6]).expand(16, 2))
    den.graph = "captured"
    ramp = torch.linspace(0, 1, 4)
    den.set_lora_gates(content=ramp, style=torch.stack([ramp, 2 * ramp]))
    assert den.graph == "captured" and den.lora_gate is gate  # new values keep the capture and the buffers
    # UNet batch order [uncond clip 0, uncond clip 1, cond clip 0, cond clip 1] x F, both CFG copies alike
    assert torch.equal(gate.table[:, 0], ramp.repeat(4))
    assert torch.equal(gate.table[:, 1], torch.cat([ramp, 2 * ramp, ramp, 2 * ramp]))
    den.clear_lora_gates()
    assert den.lora_gate is None and den.graph is None
    den.graph = "captured"
    den.clear_lora_gates()  # nothing to clear: nothing dropped
    assert den.graph == "captured"
    one = _denoiser(num_clips=1, frames=4, guidance=1.0)  # no CFG: one copy
    one.set_lora_gates(content=[[1.0, 2.0, 3.0, 4.0]])
    assert torch.equal(one.lora_gate.table[:, 0], torch.tensor([1.0, 2.0, 3.0, 4.0]))


def test_set_lora_gates_refusals_leave_state_alone():
    den = _denoiser(num_clips=2, frames=4)
    den.set_lora_gates(content=0.5, style=torch.linspace(0, 1, 4))
    gate, tab, ver = den.lora_gate, den.lora_gate.table.clone(), den.lora_gate.version
    den.graph = "captured"
    bad = [float("nan"), float("inf"), torch.ones(3), torch.ones(5), torch.ones(1, 4), torch.ones(3, 4),
           torch.ones(2, 3), torch.ones(2, 4, 1), torch.tensor([1.0, float("nan"), 1.0, 1.0]),
           torch.full((2, 4), float("-inf"))]
    for b in bad:
        with pytest.raises(ValueError):
            den.set_lora_gates(content=b)
        with pytest.raises(ValueError):
            den.set_lora_gates(content=2.0, style=b)  # the good argument is not written either
        with pytest.raises(ValueError):
            den(content_scale=b)
    assert den.lora_gate is gate and torch.equal(gate.table, tab) and gate.version == ver
    assert den.graph == "captured"
    fresh = _denoiser()
    with pytest.raises(ValueError):
        fresh.set_lora_gates(style=float("nan"))
    assert fresh.lora_gate is None  # a refused first set creates nothing


def test_frame_shard_slicing_of_gate_tables():
    """A rank holding the second half of the clip takes the second half of whole-clip gates, and local gates as they
    are (a stub shard, as test_shard_slicing_of_source_buffers uses)."""
    stub = types.SimpleNamespace(world=1, rank=0, local_frames=lambda F: (F // 2, F // 2))
    whole = _denoiser(num_clips=2, frames=4)
    c = torch.tensor([[0.1, 0.2, 0.3, 0.4], [0.5, 0.6, 0.7, 0.8]])
    s = torch.tensor([1.0, 0.0, 2.0, -1.0])
    whole.set_lora_gates(c, s)
    wt = whole.lora_gate.table.view(2, 2, 4, 2)
    for c_in, s_in in ((c, s), (c[:, 2:], s), (c, s[2:]), (c[:, 2:], s[2:])):
        half = _denoiser(num_clips=2, frames=4, shard=stub)
        assert (half.F, half.f0) == (2, 2)
        half.set_lora_gates(c_in, s_in)
        assert half.lora_gate.rows == 2 * 2 * 2
        assert torch.equal(half.lora_gate.table.view(2, 2, 2, 2), wt[:, :, 2:])
    half = _denoiser(num_clips=2, frames=4, shard=stub)
    with pytest.raises(ValueError):
        half.set_lora_gates(torch.ones(3))
    with pytest.raises(ValueError):
        half.set_lora_gates(torch.ones(2, 3))


# ----------------------------------------------------------------------------- C ABI
def test_gated_entries_reject_bad_arguments_without_gpu():
    """NULL or misaligned gate, gate_div <= 0, ld_gate < P, ld_gate % 4 != 0 -> VST_ERR_ARG (1) before any launch
    (the pointers are never dereferenced)."""
    lib = _lib.load()
    X, A, W, C, G, KT, VT = 4096, 8192, 16384, 32768, 65536, 131072, 262144

    def lora(gate, ld_gate, gate_div):
        return lib.vst_gemm_lora_gated(X, 1280, A, 1280, 32, 1280, 16, W, 1312, 8192, 1280, 1280, None, None, 0, C,
                                       1280, gate, ld_gate, gate_div, None)

    def xattn(gate, ld_gate, gate_div, acat=A):
        return lib.vst_gemm_cross_attention_gated(X, 1280, acat, 1280, 32, 1280, 16, W, 1312, None, 8192, 1280, 1280,
                                                  KT, VT, 1280, 32 * 77, 256, 77, 1, 0.125, C, 1280, gate, ld_gate,
                                                  gate_div, None)

    def gate_k(gate, ld_gate, gate_div, u=X, y=C, P=32, ldu=32, ldy=32):
        return lib.vst_lora_gate(u, ldu, 300, P, gate, ld_gate, gate_div, y, ldy, None)

    for f in (lora, xattn, gate_k):
        assert f(None, 32, 256) == 1, f.__name__      # no gate
        assert f(G, 32, 0) == 1, f.__name__           # gate_div <= 0
        assert f(G, 32, -3) == 1, f.__name__
        assert f(G, 28, 256) == 1, f.__name__         # ld_gate < P
        assert f(G, 34, 256) == 1, f.__name__         # ld_gate % 4
        for off in (4, 8, 12):
            assert f(G + off, 32, 256) == 1, (f.__name__, off)  # base not 16-byte aligned
    assert xattn(G, 32, 256, acat=None) == 1          # a gate without the LoRA operand
    assert gate_k(G, 32, 77, P=12, ldu=16, ldy=16) == 1   # P % 8
    assert gate_k(G, 32, 77, ldu=24) == 1                 # ldu < P
    assert gate_k(G, 32, 77, ldy=36) == 1                 # ldy % 8
    assert gate_k(G, 32, 77, u=X + 2) == 1                # u misaligned
    assert gate_k(G, 32, 77, y=None) == 1
