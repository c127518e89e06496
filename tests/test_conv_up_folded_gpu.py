"""The nearest-2x upsample conv as four 2x2 sub-pixel convs on folded weights (vst_fold_upsample_weight,
vst_conv3x3_up_folded; gemm_common.h conv_row_folded): the fold bit for bit, the conv against fp32 torch on the ORIGINAL
3x3 weights within the kernel suite's bar (rel_l2 5e-3, rel_max 1e-2), the 8-phase kernel against the ring kernel bit for
bit, row invariance over the number of images, strided views inside guard bands, and the model-level switch."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def K():
    from video_style_transfer_amd import kernels
    return kernels


def rnd(*shape, scale=1.0, gen=None):
    return (torch.randn(*shape, generator=gen) * scale).to(BF)


def to_nhwc(x):  # (N,C,H,W) -> [N*H*W, C]
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def wflat(w):  # (Cout,Cin,3,3) -> [Cout, 9*Cin] (ky,kx,ci)
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def measure(out, ref, name):
    out, ref = out.float().cpu(), ref.float().cpu()
    assert out.shape == ref.shape, (name, out.shape, ref.shape)
    assert torch.isfinite(out).all(), name
    err = out - ref
    l2 = (err.norm() / ref.norm().clamp_min(1e-12)).item()
    mx = (err.abs().max() / ref.abs().max().clamp_min(1e-12)).item()
    print(f"[up_folded] {name}: rel_l2={l2:.3e} rel_max={mx:.3e}")
    return l2, mx


def check(out, ref, rel_l2=5e-3, rel_max=1e-2, name=""):
    l2, mx = measure(out, ref, name)
    assert l2 <= rel_l2 and mx <= rel_max, f"{name}: rel_l2={l2:.3e} rel_max={mx:.3e}"


S = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}  # tap set S(parity, a)


def fold_ref(w):
    """w (Cout,C,3,3) bf16 -> [4*Cout, 4*C] bf16: the same fp32 sums, ascending (ky, kx), rounded once."""
    co, c = w.shape[:2]
    wf = torch.empty(4, co, 2, 2, c, dtype=BF)
    for py in (0, 1):
        for px in (0, 1):
            for a in (0, 1):
                for b in (0, 1):
                    acc = None
                    for ky in S[py, a]:
                        for kx in S[px, b]:
                            t = w[:, :, ky, kx].float()
                            acc = t if acc is None else acc + t
                    wf[2 * py + px, :, a, b] = acc.to(BF)
    return wf.reshape(4 * co, 4 * c)


def case(n, C, Co, H, W, seed=None):
    g = torch.Generator().manual_seed(seed if seed is not None else 7 * C + Co + 13 * H + W + n)
    x = rnd(n, C, H, W, gen=g)
    w = rnd(Co, C, 3, 3, scale=(9 * C) ** -0.5, gen=g)
    b = torch.randn(Co, generator=g) * 0.1
    ref = F.conv2d(F.interpolate(x.float(), scale_factor=2.0, mode="nearest"), w.float(), b, padding=1)
    return x, w, b, to_nhwc(ref)


def gemm_rows(K, n, H, W):
    return 4 * ((n * H * W + K.FOLD_ROW_ALIGN - 1) // K.FOLD_ROW_ALIGN * K.FOLD_ROW_ALIGN)


@pytest.mark.parametrize("Co,C", [(24, 64), (320, 128)])
def test_fold_bitwise(cuda, K, Co, C):
    g = torch.Generator().manual_seed(Co + C)
    w = rnd(Co, C, 3, 3, scale=(9 * C) ** -0.5, gen=g)
    wf = K.fold_upsample_weight(wflat(w).to(cuda))
    assert wf.shape == (4 * Co, 4 * C) and wf.dtype == BF
    assert torch.equal(wf.cpu(), fold_ref(w))


SHAPES = [
    (2, 64, 64, 1, 3),      # every tap row at a border
    (2, 64, 320, 7, 5),     # odd sizes; 70 rows per class, one partial 128-row tile per class
    (1, 64, 320, 3, 43),    # 129 rows per class; the second row tile holds one row
    (1, 128, 640, 16, 16),  # 256 rows per class: exact tiles
    (3, 128, 128, 8, 8),    # ring-kernel tile for Cout 128, the VAE's
]


@pytest.mark.parametrize("n,C,Co,H,W", SHAPES)
def test_folded_conv_against_fp32_torch(cuda, K, n, C, Co, H, W):
    x, w, b, ref = case(n, C, Co, H, W)
    wf = K.fold_upsample_weight(wflat(w).to(cuda))
    out = K.conv3x3_up_folded(to_nhwc(x).to(cuda), n, H, W, wf, b.to(cuda))
    check(out, ref, name=f"folded {n}x{C}->{Co} {H}x{W} {K.gemm_kernel_name(gemm_rows(K, n, H, W), Co, 4 * C, 4)}")
    # the 3x3 kernel path on the same operands, for the record of the fold's own rounding
    plain = K.conv3x3(to_nhwc(x).to(cuda), n, H, W, wflat(w).to(cuda), b.to(cuda), upsample=True)
    measure(out, plain, f"folded against the 3x3 path {n}x{C}->{Co} {H}x{W}")


P8_SHAPES = [  # n, C, Co, H, W, forced 8-phase tile width (0: the policy), the kernel's name
    (4, 64, 320, 32, 32, 0, "gemm_p8<128x320,upfold>"),
    (8, 64, 192, 32, 32, 0, "gemm_p8<256x192,upfold>"),
    (8, 64, 192, 32, 32, 256, "gemm_p8<256x256,upfold>"),
]


@pytest.mark.parametrize("n,C,Co,H,W,bn,name", P8_SHAPES)
def test_folded_conv_8phase_bitwise_equals_ring(cuda, K, n, C, Co, H, W, bn, name):
    """The smallest grids the policy gives to each 8-phase conv tile (half a wave of 256x256 tiles), folded mode: the
    8-phase kernel and the ring kernel agree bit for bit (same k order), and both hold the fp32 bar."""
    x, w, b, ref = case(n, C, Co, H, W)
    wf = K.fold_upsample_weight(wflat(w).to(cuda))
    args = (to_nhwc(x).to(cuda), n, H, W, wf, b.to(cuda))
    M = gemm_rows(K, n, H, W)
    with K.p8_tile_width(bn), K.p8_conv(True):
        assert K.gemm_kernel_name(M, Co, 4 * C, 4) == name
        p8 = K.conv3x3_up_folded(*args)
    with K.p8_conv(False):
        assert "gemm_ring" in K.gemm_kernel_name(M, Co, 4 * C, 4)
        ring = K.conv3x3_up_folded(*args)
    assert torch.equal(p8, ring)
    check(p8, ref, name=f"folded p8 {name}")


def test_row_invariance_over_images(cuda, K):
    """Image 1's rows of an nimg = 3 call are the bits of an nimg = 1 call on that image."""
    n, C, Co, H, W = 3, 64, 320, 7, 5
    x, w, b, _ = case(n, C, Co, H, W)
    wf = K.fold_upsample_weight(wflat(w).to(cuda))
    xd = to_nhwc(x).to(cuda)
    all3 = K.conv3x3_up_folded(xd, n, H, W, wf, b.to(cuda))
    one = K.conv3x3_up_folded(xd[H * W:2 * H * W], 1, H, W, wf, b.to(cuda))
    assert torch.equal(all3[4 * H * W:8 * H * W], one)


def test_views_and_guard_bands(cuda, K):
    """Output as a view with ldc = Cout + 8 inside a poisoned buffer with guard rows before and after, input as a
    row-strided view: the values are those of the packed call, the padding columns and guard rows stay intact (a wrong
    row map would scatter into them)."""
    n, C, Co, H, W = 2, 64, 320, 7, 5
    x, w, b, ref = case(n, C, Co, H, W)
    wf = K.fold_upsample_weight(wflat(w).to(cuda))
    xd, bd = to_nhwc(x).to(cuda), b.to(cuda)
    packed = K.conv3x3_up_folded(xd, n, H, W, wf, bd)
    M, G, POISON = n * 4 * H * W, 5, -7.0
    buf = torch.full((M + 2 * G, Co + 8), POISON, dtype=BF, device=cuda)
    xbuf = torch.full((n * H * W, C + 24), POISON, dtype=BF, device=cuda)
    xbuf[:, :C] = xd
    out = K.conv3x3_up_folded(xbuf[:, :C], n, H, W, wf, bd, out=buf[G:G + M, :Co])
    assert out.data_ptr() == buf[G:G + M, :Co].data_ptr()
    assert torch.equal(buf[G:G + M, :Co], packed)
    assert (buf[:G] == POISON).all() and (buf[G + M:] == POISON).all() and (buf[:, Co:] == POISON).all()
    check(packed, ref, name="folded views")


def test_model_level_switch(cuda, K):
    """Upsample2D.run takes the folded path: against K.conv3x3(upsample=True) on the same weights within rel_l2 5e-3 /
    rel_max 1.6e-2 (the CPU emulation of the fold's rounding measured 2.5e-3 / 6.4e-3); the fold is launched once (a
    second call records none), and a captured graph of the call holds one kernel: the captured region makes one
    library call, the folded conv, whose plan is a single launch."""
    from video_style_transfer_amd.unet_motion import Upsample2D, f32
    n, C, H, W = 2, 64, 8, 8
    g = torch.Generator().manual_seed(5)
    up = Upsample2D(C)
    with torch.no_grad():
        up.conv.weight.copy_(rnd(C, C, 3, 3, scale=(9 * C) ** -0.5, gen=g).float())
        up.conv.bias.copy_(torch.randn(C, generator=g) * 0.1)
    up = up.to(cuda).requires_grad_(False)
    x = rnd(n * H * W, C, gen=g).to(cuda)
    K.profile_launches(True)
    try:
        y, OH, OW = up.run(x, n, H, W)
        first = [r[0] for r in K.collect_launches()]
        K.profile_launches(True)
        y2, *_ = up.run(x, n, H, W)
        second = [r[0] for r in K.collect_launches()]
    finally:
        K.profile_launches(False)
    assert (OH, OW) == (2 * H, 2 * W)
    assert first == ["fold_upsample_weight", "conv3x3"] and second == ["conv3x3"]
    assert torch.equal(y, y2)
    plain = K.conv3x3(x, n, H, W, up.conv.kernel_weight(), f32(up.conv.bias), upsample=True)
    check(y, plain, rel_l2=5e-3, rel_max=1.6e-2, name="Upsample2D.run folded against the 3x3 kernel path")
    # a captured graph of the call: the captured region makes exactly one library call, the folded conv (no fold, no
    # copy), whose plan is a single kernel (the folded conv never splits K: no reduce launch behind it)
    from video_style_transfer_amd import _lib
    assert "splitk" not in K.gemm_kernel_name(gemm_rows(K, n, H, W), C, 4 * C, 4)
    calls, real = [], _lib.call

    def counting(name, *a):
        calls.append(name)
        return real(name, *a)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        up.run(x, n, H, W)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    _lib.call = counting
    try:
        with torch.cuda.graph(graph):
            yg, *_ = up.run(x, n, H, W)
    finally:
        _lib.call = real
    assert calls == ["vst_conv3x3_up_folded"], calls
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(yg, y)
