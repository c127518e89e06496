"""Host side of the folded upsample conv (vst_conv3x3_up_folded): the entry's refusals, which return before any launch,
and the index map of gemm_common.h's conv_row_folded / conv_tap_pixel_folded / conv_out_row_folded restated in Python
and checked exhaustively against F.interpolate + unfold, so the map is pinned without a device."""
import ctypes

import torch
import torch.nn.functional as F

S = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}  # tap set S(parity, a) of the weight fold
ALIGN = 256  # kFoldRowAlign


def gemm_row(cls, img, y, x, nimg, H, W):
    """Class-major GEMM row of (class, image, input pixel)."""
    up_rows = (nimg * H * W + ALIGN - 1) // ALIGN * ALIGN
    return cls * up_rows + (img * H + y) * W + x


def tap_pixel(cls, y, x, a, b, H, W):
    """Input pixel that tap (a, b) of class (py, px) = (cls >> 1, cls & 1) reads at (y, x); None in the padding."""
    iy, ix = y + (cls >> 1) + a - 1, x + (cls & 1) + b - 1
    return (iy, ix) if 0 <= iy < H and 0 <= ix < W else None


def out_row(cls, img, y, x, H, W):
    return (img * 2 * H + 2 * y + (cls >> 1)) * 2 * W + 2 * x + (cls & 1)


def test_tap_sets_partition_the_kernel():
    for p in (0, 1):
        assert sorted(S[p, 0] + S[p, 1]) == [0, 1, 2]


def test_index_map_against_interpolate_unfold():
    """Every 3x3 tap of every pixel of the nearest-2x upsampled 3x4 image reads the input pixel the folded map names
    for the tap's (class, a, b), or padding where the map says so; the output rows are a bijection."""
    nimg, H, W = 2, 3, 4
    ids = torch.arange(1, nimg * H * W + 1, dtype=torch.float32).reshape(nimg, 1, H, W)  # 0 = padding
    cols = F.unfold(F.interpolate(ids, scale_factor=2.0, mode="nearest"), 3, padding=1)  # [nimg, 9, 2H*2W]
    cols = cols.reshape(nimg, 3, 3, 2 * H, 2 * W)
    rows, mrows = set(), set()
    for img in range(nimg):
        for cls in range(4):
            py, px = cls >> 1, cls & 1
            for y in range(H):
                for x in range(W):
                    oy, ox = 2 * y + py, 2 * x + px
                    r = out_row(cls, img, y, x, H, W)
                    assert r == (img * 2 * H + oy) * 2 * W + ox
                    rows.add(r)
                    mrows.add(gemm_row(cls, img, y, x, nimg, H, W))
                    for a in (0, 1):
                        for b in (0, 1):
                            t = tap_pixel(cls, y, x, a, b, H, W)
                            want = 0 if t is None else 1 + (img * H + t[0]) * W + t[1]
                            for ky in S[py, a]:
                                for kx in S[px, b]:
                                    assert int(cols[img, ky, kx, oy, ox]) == want, (img, cls, y, x, a, b, ky, kx)
    assert rows == set(range(nimg * 4 * H * W))
    assert len(mrows) == nimg * 4 * H * W and max(mrows) < 4 * ALIGN


def test_folded_weights_give_the_upsampled_conv_in_fp32():
    """Four 2x2 convs at the map's offsets on tap-summed weights equal interpolate + conv3x3 (fp32, no rounding)."""
    g = torch.Generator().manual_seed(0)
    x, w = torch.randn(2, 5, 3, 4, generator=g), torch.randn(6, 5, 3, 3, generator=g)
    ref = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, padding=1)
    out = torch.zeros_like(ref)
    for cls in range(4):
        py, px = cls >> 1, cls & 1
        wf = torch.stack([torch.stack([sum(w[:, :, ky, kx] for ky in S[py, a] for kx in S[px, b]) for b in (0, 1)], -1)
                          for a in (0, 1)], -2)  # [Co, C, a, b]
        # tap (a, b) reads (y + py + a - 1, x + px + b - 1): pad (1 - px, px) in x and (1 - py, py) in y
        out[:, :, py::2, px::2] = F.conv2d(F.pad(x, (1 - px, px, 1 - py, py)), wf)
    assert torch.allclose(out, ref, rtol=1e-5, atol=1e-5)


def test_entry_refusals():
    """Every call returns before any launch: the pointers are never dereferenced (no GPU needed)."""
    from video_style_transfer_amd import _lib
    P, I = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES["vst_conv3x3_up_folded"] == (I, [P, I, I, P, I, I, I, I, P, I, I, P, P, P, P, I, P])
    assert _lib.SIGNATURES["vst_fold_upsample_weight"] == (I, [P, I, I, P, P])
    f = _lib.load().vst_conv3x3_up_folded
    X, WF, O, X2 = 4096, 65536, 1 << 20, 8192

    def call(x=X, ldx=64, C=64, x2=None, C2=0, nimg=2, H=7, W=5, wf=WF, ldwf=256, Cout=320, bias=None, rb=None, R=None,
             out=O, ldc=320):
        return f(x, ldx, C, x2, C2, nimg, H, W, wf, ldwf, Cout, bias, rb, R, out, ldc, None)

    ARG, UNS = 1, 3
    assert call(x2=X2, C2=64) == UNS and call(C2=64) == UNS          # a second source
    assert call(C=96, ldx=96, ldwf=384) == UNS                       # C % 64 != 0
    assert call(rb=X2) == UNS and call(R=X2) == UNS                  # row bias / residual
    assert call(Cout=4, ldc=8) == UNS
    assert call(ldwf=4 * 64 - 8) == ARG and call(ldwf=4 * 64 + 4) == ARG  # folded weight rows not [2][2][C] views
    assert call(ldc=312) == ARG and call(ldc=324) == ARG             # ldc too small / not a multiple of 8
    assert call(ldx=56) == ARG
    assert call(x=None) == ARG and call(wf=None) == ARG and call(out=None) == ARG
    assert call(nimg=0) == ARG and call(H=0) == ARG
    g = _lib.load().vst_fold_upsample_weight
    assert g(None, 8, 64, O, None) == ARG and g(X, 8, 64, None, None) == ARG and g(X, 0, 64, O, None) == ARG
    assert g(X, 8, 60, O, None) == UNS
    assert _lib.load().vst_gemm_kernel_name(1024, 320, 256, 4, 0, 0, 0) == b"gemm_ring<128x128,upfold>"
    assert _lib.load().vst_gemm_kernel_name(16384, 320, 256, 4, 0, 0, 0) == b"gemm_p8<128x320,upfold>"
    assert _lib.load().vst_gemm_kernel_name(4 * 8192, 1280, 4 * 1280, 4, 0, 0, 0) == b"gemm_p8<128x320,upfold>"


def test_python_wrapper_refuses_host_tensors():
    from video_style_transfer_amd import _lib, kernels as K
    import pytest
    x = torch.zeros(2 * 7 * 5, 64, dtype=torch.bfloat16)
    wf = torch.zeros(4 * 320, 4 * 64, dtype=torch.bfloat16)
    with pytest.raises(_lib.VstError, match="device tensor"):
        K.conv3x3_up_folded(x, 2, 7, 5, wf, None)
    with pytest.raises(_lib.VstError, match="device tensor"):
        K.fold_upsample_weight(torch.zeros(320, 9 * 64, dtype=torch.bfloat16))
    assert K.conv3x3_up_folded_applies(64, 320) and not K.conv3x3_up_folded_applies(96, 320)
    assert not K.conv3x3_up_folded_applies(64, 4)
