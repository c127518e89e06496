"""Cross-frame spatial self-attention (DESIGN.md "Cross-frame spatial self-attention"), host side: the option's
validation, the key/value frame list, the C ABI entry's export and argument checks, and the fp32 reference that the GPU
tests (tests/test_cross_frame_gpu.py) compare the HIP path with."""
import ctypes

import pytest
import torch


# ---------------------------------------------------------------- the fp32 reference
def frames_ref(q, k, v, nclip, F, N, heads, sources):
    """fp32 torch: rows (b*F + f)*N + p; frame f of clip b attends to the tokens of K.frame_list(f, F, sources) of the
    same clip, concatenated in that order, under one softmax per head (scale 1/8, head_dim 64)."""
    from video_style_transfer_amd import kernels as K
    C = heads * 64
    qh, kh, vh = (t.float()[:, :C].reshape(nclip, F, N, heads, 64).permute(0, 1, 3, 2, 4) for t in (q, k, v))
    out = torch.empty(nclip, F, heads, N, 64)
    for f in range(F):
        fl = K.frame_list(f, F, sources)
        kc = torch.cat([kh[:, j] for j in fl], 2)  # [nclip, heads, len(fl)*N, 64]
        vc = torch.cat([vh[:, j] for j in fl], 2)
        out[:, f] = torch.softmax(qh[:, f] @ kc.transpose(-1, -2) / 8.0, -1) @ vc
    return out.permute(0, 1, 3, 2, 4).reshape(nclip * F * N, C)


def test_reference_collapses_to_plain_sdpa():
    """Rows of a frame whose list is the frame alone equal plain per-frame SDPA; the others do not."""
    nclip, F, N, heads = 2, 3, 24, 2
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(nclip * F * N, heads * 64, generator=g) for _ in range(3))
    plain = frames_ref(q, k, v, nclip * F, 1, N, heads, ("first",)).view(nclip, F, N, -1)   # every frame a clip
    sdpa = torch.nn.functional.scaled_dot_product_attention(
        *(t.view(nclip * F, N, heads, 64).transpose(1, 2) for t in (q, k, v))).transpose(1, 2).reshape(plain.shape)
    assert (plain - sdpa).abs().max() <= 1e-6
    first = frames_ref(q, k, v, nclip, F, N, heads, ("first",)).view(nclip, F, N, -1)
    assert (first[:, 0] - plain[:, 0]).abs().max() <= 1e-6
    assert (first[:, 1:] - plain[:, 1:]).abs().max() > 1e-3
    prev = frames_ref(q, k, v, nclip, F, N, heads, ("prev", 0)).view(nclip, F, N, -1)
    assert (prev[:, 0] - plain[:, 0]).abs().max() <= 1e-6
    assert (prev[:, 1] - first[:, 1]).abs().max() <= 1e-6      # frame 1: [1, 0] either way
    own = frames_ref(q, k, v, nclip, F, N, heads, (2,)).view(nclip, F, N, -1)
    assert (own[:, 2] - plain[:, 2]).abs().max() <= 1e-6


# ---------------------------------------------------------------- the option and the frame list
def test_option_accepts():
    from video_style_transfer_amd.unet_motion import CrossFrameAttention, as_cross_frame
    assert CrossFrameAttention().sources == ("first",)
    for src in (("first",), ("prev",), (3,), ("first", "prev"), ("prev", "first"), (0, 5), ("prev", 0), ["first", 2]):
        assert CrossFrameAttention(src).sources == tuple(src)
    cf = CrossFrameAttention(("first", "prev"))
    assert as_cross_frame(cf) is cf and as_cross_frame(None) is None
    assert as_cross_frame(("first", "prev")) == cf
    assert cf.active(2) and not cf.active(1)
    with pytest.raises(Exception):   # frozen
        cf.sources = ("prev",)


@pytest.mark.parametrize("src", [(), ("first", "prev", 2), ("first", "first"), ("first", 0), (2, 2), ("last",), (-1,),
                                 (1.0,), (True,), (None,)])
def test_option_refuses(src):
    from video_style_transfer_amd.unet_motion import CrossFrameAttention
    with pytest.raises(ValueError):
        CrossFrameAttention(src)


def test_frame_list():
    from video_style_transfer_amd import kernels as K
    assert K.frame_list(0, 1, ("first", "prev")) == [0]
    assert [K.frame_list(f, 4, ("first", "prev")) for f in range(4)] == [[0], [1, 0], [2, 0, 1], [3, 0, 2]]
    assert [K.frame_list(f, 4, ("prev", "first")) for f in range(3)] == [[0], [1, 0], [2, 1, 0]]
    assert [K.frame_list(f, 3, ("first",)) for f in range(3)] == [[0], [1, 0], [2, 0]]
    assert K.frame_list(3, 4, (3,)) == [3]
    assert K.frame_list(1, 4, (3, "prev")) == [1, 3, 0]
    assert K.frame_list(2, 4, ()) == [2]
    with pytest.raises(ValueError):
        K.frame_list(0, 4, (4,))
    with pytest.raises(ValueError):
        K.frame_list(4, 4, ("first",))
    assert [K.frame_source(s) for s in ("first", "prev", 0, 7)] == [0, -2, 0, 7]


def test_check_names_cross_frame():
    """The model-level refusals (no GPU needed: they precede every launch)."""
    import types
    from video_style_transfer_amd import _lib
    from video_style_transfer_amd.unet_motion import CrossFrameAttention, check_cross_frame
    model = types.SimpleNamespace(named_modules=lambda: [])
    check_cross_frame(model, 4, None)
    check_cross_frame(model, 4, CrossFrameAttention((3, "prev")))
    check_cross_frame(model, 1, CrossFrameAttention((3,)))           # single-frame clip: inactive
    with pytest.raises(_lib.VstError, match="cross_frame"):
        check_cross_frame(model, 4, CrossFrameAttention((4,)))
    with pytest.raises(_lib.VstError, match="cross_frame"):
        check_cross_frame(model, 4, CrossFrameAttention(("first",)), types.SimpleNamespace(world=2, rank=0))
    check_cross_frame(model, 4, CrossFrameAttention(("first",)), types.SimpleNamespace(world=1, rank=0))


# ---------------------------------------------------------------- the C ABI entry
def test_frames_entry_exported_and_checks_arguments():
    """libvst_hip.so exports vst_spatial_attention_frames, and the entry refuses bad arguments on the host (no GPU
    needed: every call below returns VST_ERR_ARG before any launch; the pointers are never dereferenced)."""
    from video_style_transfer_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "vst_spatial_attention_frames")
    assert "vst_spatial_attention_frames" in _lib.SIGNATURES
    f = _lib.load().vst_spatial_attention_frames
    Q, KV, O = 4096, 8192, 16384

    def call(q=Q, k=KV, v=KV + 128, o=O, ldq=192, ldkv=192, ldo=64, nclip=1, F=4, heads=1, N=16, src1=0, src2=-1, hd=64):
        return f(q, ldq, k, v, ldkv, o, ldo, nclip, F, heads, N, src1, src2, hd, 0.125, None)

    assert call(hd=40) == 1
    assert call(ldq=196) == 1          # strides: multiples of 8
    assert call(ldkv=100) == 1
    assert call(ldo=68) == 1
    assert call(q=None) == 1
    assert call(k=None) == 1
    assert call(v=None) == 1
    assert call(o=None) == 1
    assert call(src1=4) == 1           # src >= F
    assert call(src1=0, src2=4) == 1
    assert call(src1=-3) == 1          # src < -2
    assert call(src1=0, src2=-3) == 1
    assert call(src1=-1, src2=0) == 1  # a second source without a first
    assert call(src1=-1, src2=-2) == 1
    assert call(src1=2, src2=2) == 1   # two equal sources
    assert call(src1=-2, src2=-2) == 1
    assert call(nclip=0) == 1
    assert call(F=0, src1=-1) == 1
    # byte extents past 2^31 - 1: 64 clips x 32 frames x 4096 tokens at a row stride of 2^20 elements
    assert f(Q, 1 << 20, KV, KV, 1 << 20, O, 64, 64, 32, 1, 4096, 0, -1, 64, 0.125, None) == 1
    assert f(Q, 64, KV, KV, 1 << 20, O, 64, 64, 32, 1, 4096, 0, -1, 64, 0.125, None) == 1     # K/V alone
