"""Sliding-window frame attention for long clips (DESIGN.md "Long clips"), host side: the window / weight helpers,
the C ABI entry's export and argument checks, and the fp32 reference of a windowed motion module that the GPU tests
(tests/test_temporal_context_gpu.py) compare the HIP path with, tied here to the golden-pinned oracle."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the fp32 reference
def windowed_motion_module(P, name, x, num_frames, L, S, weighting="pyramid", heads=8):
    """oracle.unet.motion_module with each attention half run inside sliding windows: for every window start s and
    position j < L, q/k/v of frame s + j come from LN(x[s + j]) + pe[j] (the position INSIDE the window), softmax
    attention runs over the window's L frames, and the windows are blended per frame,
    o[f] = sum_s w[f - s] O_s[f - s] / sum_s w[f - s]; then to_out and the residual.  Windowing is active when
    num_frames > L; otherwise there is one window of num_frames frames."""
    import torch.nn.functional as F
    from oracle import ref_ops as R
    from oracle import unet as OU
    from video_style_transfer_amd import kernels as K
    BF, C, H, W = x.shape
    B = BF // num_frames
    Lw = min(L, num_frames)
    starts = K.context_windows(num_frames, L, S)
    w = torch.tensor(K.context_weights(Lw, weighting))
    h = x.reshape(B, num_frames, C, H, W).permute(0, 2, 1, 3, 4)
    h = F.group_norm(h, 32, P[name + ".norm.weight"].float(), P[name + ".norm.bias"].float(), 1e-6)
    h = h.permute(0, 3, 4, 2, 1).reshape(B * H * W, num_frames, C)
    h = OU.linear(P, name + ".proj_in", h)
    blk = name + ".transformer_blocks.0"
    pe = P[blk + ".pos_embed.pe"].float().reshape(1, -1, C)

    def half(h, norm, attn):
        n = OU.layer_norm(P, f"{blk}.{norm}", h)
        num = torch.zeros_like(h)
        den = torch.zeros(num_frames)
        for s in starts:
            nw = n[:, s:s + Lw] + pe[:, :Lw]
            q, k, v = (OU.linear(P, f"{blk}.{attn}.{pj}", nw).view(nw.shape[0], Lw, heads, C // heads).transpose(1, 2)
                       for pj in ("to_q", "to_k", "to_v"))
            o = R.sdpa(q, k, v).transpose(1, 2).reshape(nw.shape[0], Lw, C)
            num[:, s:s + Lw] += o * w.view(1, Lw, 1)
            den[s:s + Lw] += w
        return OU.linear(P, f"{blk}.{attn}.to_out.0", num / den.view(1, -1, 1)) + h

    h = half(h, "norm1", "attn1")
    h = half(h, "norm2", "attn2")
    h = OU.geglu_ff(P, blk + ".ff", OU.layer_norm(P, blk + ".norm3", h)) + h
    h = OU.linear(P, name + ".proj_out", h)
    h = h.reshape(B, H, W, num_frames, C).permute(0, 3, 4, 1, 2).reshape(BF, C, H, W)
    return h + x


def motion_params(C, seed=1, name="mm"):
    """Random parameters of one motion module under oracle.unet's key names (bf16-representable, as on the device)."""
    from video_style_transfer_amd.weights import sinusoid_table
    g = torch.Generator().manual_seed(seed)
    P = {}

    def r(*shape, scale=1.0, shift=0.0):
        return (shift + scale * torch.randn(*shape, generator=g)).to(torch.bfloat16).float()

    P[name + ".norm.weight"], P[name + ".norm.bias"] = r(C, scale=0.1, shift=1.0), r(C, scale=0.1)
    for lin in ("proj_in", "proj_out"):
        P[f"{name}.{lin}.weight"], P[f"{name}.{lin}.bias"] = r(C, C, scale=C ** -0.5), r(C, scale=0.1)
    blk = name + ".transformer_blocks.0"
    for a in ("attn1", "attn2"):
        for pj in ("to_q", "to_k", "to_v"):
            P[f"{blk}.{a}.{pj}.weight"] = r(C, C, scale=C ** -0.5)
        P[f"{blk}.{a}.to_out.0.weight"], P[f"{blk}.{a}.to_out.0.bias"] = r(C, C, scale=C ** -0.5), r(C, scale=0.1)
    for n in ("norm1", "norm2", "norm3"):
        P[f"{blk}.{n}.weight"], P[f"{blk}.{n}.bias"] = r(C, scale=0.1, shift=1.0), r(C, scale=0.1)
    P[f"{blk}.ff.net.0.proj.weight"], P[f"{blk}.ff.net.0.proj.bias"] = r(8 * C, C, scale=C ** -0.5), r(8 * C, scale=0.1)
    P[f"{blk}.ff.net.2.weight"], P[f"{blk}.ff.net.2.bias"] = r(C, 4 * C, scale=(4 * C) ** -0.5), r(C, scale=0.1)
    P[f"{blk}.pos_embed.pe"] = sinusoid_table(C, 32)
    return P


# ---------------------------------------------------------------- host helpers
@pytest.mark.parametrize("F,L,S,starts", [(20, 16, 4, [0, 4]), (23, 16, 4, [0, 4, 7]), (40, 16, 16, [0, 16, 24]),
                                          (33, 32, 8, [0, 1]), (19, 8, 3, [0, 3, 6, 9, 11]), (16, 16, 4, [0])])
def test_context_windows(F, L, S, starts):
    from video_style_transfer_amd import kernels as K
    got = K.context_windows(F, L, S)
    assert got == starts
    if F >= L:  # every window L frames long inside the clip, every frame covered
        assert all(0 <= s and s + L <= F for s in got)
        assert set(f for s in got for f in range(s, s + L)) == set(range(F))


@pytest.mark.parametrize("F,L,S", [(40, 16, 17), (40, 16, 0), (40, 33, 4), (40, 0, 1)])
def test_context_windows_refuses(F, L, S):
    from video_style_transfer_amd import kernels as K
    from video_style_transfer_amd.unet_motion import TemporalContext
    with pytest.raises(ValueError):
        K.context_windows(F, L, S)
    with pytest.raises(ValueError):
        TemporalContext(L, S)


def test_context_weights():
    from video_style_transfer_amd import kernels as K
    assert K.context_weights(16, "pyramid") == [1, 2, 3, 4, 5, 6, 7, 8, 8, 7, 6, 5, 4, 3, 2, 1]
    assert K.context_weights(5, "pyramid") == [1, 2, 3, 2, 1]
    assert K.context_weights(5, "flat") == [1, 1, 1, 1, 1]
    with pytest.raises(ValueError):
        K.context_weights(5, "triangle")


def test_clip_length_check_names_context_length():
    from video_style_transfer_amd import _lib
    from video_style_transfer_amd.unet_motion import TemporalContext, check_clip_length
    with pytest.raises(_lib.VstError, match="context_length"):
        check_clip_length(40, 32, None)
    check_clip_length(32, 32, None)
    check_clip_length(40, 32, TemporalContext(16, 4))
    check_clip_length(16, 32, TemporalContext(16, 4))


# ---------------------------------------------------------------- the C ABI entry
def test_windowed_entry_exported_and_checks_arguments():
    """libvst_hip.so exports vst_temporal_attention_windowed, and the entry refuses bad arguments on the host (no GPU
    needed: every call below returns VST_ERR_ARG before any launch; the pointers are never dereferenced)."""
    from video_style_transfer_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "vst_temporal_attention_windowed")
    assert "vst_temporal_attention_windowed" in _lib.SIGNATURES
    f = _lib.load().vst_temporal_attention_windowed
    Q, O, T = 4096, 8192, 16384

    def call(F=20, L=16, S=4, d=8, ld=64, ldo=64, ldpos=192, weighting=1, pos=T, q=Q, o=O):
        return f(q, q, q, ld, pos, pos, pos, ldpos, o, ldo, 1, F, 8, 8, d, L, S, weighting, 1.0, None)

    assert call(F=15) == 1            # F < L
    assert call(L=33, F=40) == 1      # L > 32
    assert call(L=0) == 1
    assert call(S=17) == 1            # S > L
    assert call(S=0) == 1
    assert call(d=12) == 1            # head_dim % 8
    assert call(d=168, ld=1344 * 3, ldo=1344, ldpos=1344 * 3) == 1   # head_dim > 160
    assert call(ld=60) == 1           # ldqkv % 8
    assert call(ldo=60) == 1
    assert call(ldpos=190) == 1       # table rows are read as 16-byte vectors
    assert call(pos=T + 4) == 1       # ... from 16-byte aligned bases
    assert call(weighting=2) == 1
    assert call(q=None) == 1
    assert call(o=None) == 1
    assert f(Q, Q, Q, 1 << 20, None, None, None, 0, O, 64, 64, 32, 4096, 8, 8, 16, 4, 1, 1.0, None) == 1  # > 2^31 B


# ---------------------------------------------------------------- the reference against the oracle
@pytest.mark.parametrize("weighting", ["pyramid", "flat"])
def test_windowed_reference_equals_oracle_for_one_window(weighting):
    """With L = F there is one window and every weight cancels: the windowed reference is oracle.unet.motion_module."""
    from oracle import unet as OU
    C, Fr, B, H, W = 64, 8, 2, 2, 3
    P = motion_params(C)
    x = torch.randn(B * Fr, C, H, W, generator=torch.Generator().manual_seed(2))
    ref = OU.motion_module(P, "mm", x, Fr)
    got = windowed_motion_module(P, "mm", x, Fr, Fr, 3, weighting)
    assert (got - ref).abs().max() <= 1e-5 * ref.abs().max()
    # a context longer than the clip is inactive too
    got = windowed_motion_module(P, "mm", x, Fr, 16, 4, weighting)
    assert (got - ref).abs().max() <= 1e-5 * ref.abs().max()


def test_windowed_reference_differs_when_windows_are_active():
    """F > L: frames attend inside their windows only, so the result is not the whole-clip module's."""
    from oracle import unet as OU
    C, Fr = 64, 12
    P = motion_params(C)
    x = torch.randn(Fr, C, 2, 2, generator=torch.Generator().manual_seed(3))
    ref = OU.motion_module(P, "mm", x, Fr)
    got = windowed_motion_module(P, "mm", x, Fr, 8, 2)
    assert (got - ref).abs().max() > 1e-3 * ref.abs().max()
