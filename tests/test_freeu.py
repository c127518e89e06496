"""FreeU on the host: the closed form of fourier_filter(x, threshold=1, scale) against its torch.fft
definition and against three analytic cases, apply_freeu_reference's channel split and stages, and every refusal that
needs no GPU (values, the denoiser's arguments, the library's argument checks, training)."""
import math
import types

import pytest
import torch

SHAPES = [(2, 2), (2, 3), (3, 5), (4, 4), (7, 4), (6, 9), (8, 12), (16, 16), (32, 32)]
SCALES = [0.9, 0.6, 0.2, 1.0]


def fft_filter(x, scale, threshold=1):
    """diffusers.utils.torch_utils.fourier_filter restated: fp32 FFT over the last two axes, fftshift, the
    2 threshold x 2 threshold block around index (H // 2, W // 2) times `scale`, shift back, inverse, real part."""
    dtype = x.dtype
    x = x.to(torch.float32)
    H, W = x.shape[-2:]
    X = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones(x.shape, dtype=torch.float32)
    crow, ccol = H // 2, W // 2
    mask[..., crow - threshold:crow + threshold, ccol - threshold:ccol + threshold] = scale
    X = X * mask
    return torch.fft.ifftn(torch.fft.ifftshift(X, dim=(-2, -1)), dim=(-2, -1)).real.to(dtype)


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_closed_form_equals_fft(H, W, dtype):
    from video_style_transfer_amd.freeu import fourier_filter_reference
    g = torch.Generator().manual_seed(100 * H + W)
    x = torch.randn(2, 3, H, W, generator=g)
    for s in SCALES:
        got = fourier_filter_reference(x, s, dtype)
        assert got.dtype == dtype and got.shape == x.shape
        d = (got.double() - fft_filter(x, s).double()).abs().max().item()
        bound = 2e-6 * max(1.0, x.abs().max().item())
        print(f"[freeu] {H}x{W} s={s} {dtype}: max |closed form - fft| = {d:.2e}")
        assert d <= bound, (H, W, s, d)


def test_analytic_cases():
    from video_style_transfer_amd.freeu import fourier_filter_reference
    for H, W in ((3, 5), (6, 9), (16, 16), (7, 4)):
        h = torch.arange(H, dtype=torch.float64)[:, None].expand(H, W)
        for s in (0.9, 0.2):
            const = torch.full((H, W), 1.75, dtype=torch.float64)
            assert torch.allclose(fourier_filter_reference(const, s), s * const, rtol=0, atol=1e-12)
            f1 = torch.cos(2 * math.pi * h / H)   # the +-1 pair: only the -1 bin is scaled
            assert torch.allclose(fourier_filter_reference(f1, s), (1 + s) / 2 * f1, rtol=0, atol=1e-12)
            if H >= 5:
                f2 = torch.cos(2 * math.pi * 2 * h / H)
                assert torch.allclose(fourier_filter_reference(f2, s), f2, rtol=0, atol=1e-12)
    for shape in ((1, 4), (4, 1), (1, 1)):
        with pytest.raises(ValueError):
            fourier_filter_reference(torch.zeros(shape), 0.5)


def test_apply_freeu_reference():
    from video_style_transfer_amd.freeu import apply_freeu_reference, fourier_filter_reference
    g = torch.Generator().manual_seed(1)
    hidden, skip = torch.randn(2, 10, 4, 6, generator=g), torch.randn(2, 6, 4, 6, generator=g)
    vals = dict(s1=0.9, s2=0.2, b1=1.3, b2=1.4)
    for stage, (s, b) in enumerate(((0.9, 1.3), (0.2, 1.4))):
        h, k = apply_freeu_reference(stage, hidden, skip, **vals)
        assert torch.equal(h[:, :5], hidden[:, :5] * b) and torch.equal(h[:, 5:], hidden[:, 5:])   # C_h // 2 of 10
        assert k.dtype == skip.dtype
        assert torch.equal(k, fourier_filter_reference(skip, s).to(skip.dtype))
        assert (k - fft_filter(skip, s)).abs().max() <= 2e-6 * max(1.0, skip.abs().max().item())
    h, k = apply_freeu_reference(0, hidden[:, :7], skip, **vals)   # the split follows the tensor given: 7 // 2 = 3
    assert torch.equal(h[:, :3], hidden[:, :3] * 1.3) and torch.equal(h[:, 3:], hidden[:, 3:7])
    for stage in (2, 3):
        h, k = apply_freeu_reference(stage, hidden, skip, **vals)
        assert torch.equal(h, hidden) and torch.equal(k, skip)
    assert torch.equal(hidden, hidden.clone())


BAD = [(float("nan"), 0.2, 1.3, 1.4), (0.9, float("inf"), 1.3, 1.4), (0.9, 0.2, 0.0, 1.4), (0.9, 0.2, 1.3, -1.0),
       (0.9, 0.2, 1.3, "x"), (0.9, 0.2, 1.3, None), (-0.0, 0.2, 1.3, 1.4)]


def test_values_are_checked_before_anything_is_allocated():
    from video_style_transfer_amd.freeu import FreeU, as_freeu, check_freeu
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser
    assert check_freeu(0.9, 0.2, 1.3, 1.4) == (0.9, 0.2, 1.3, 1.4)
    for vals in BAD:
        with pytest.raises(ValueError, match="freeu"):
            check_freeu(*vals)
        with pytest.raises(ValueError, match="freeu"):
            FreeU(*vals, device="cpu")
        with pytest.raises(ValueError, match="freeu"):   # refused with the other arguments, before `unet` is touched
            AnimateDiffDenoiser(None, 4, 64, 64, freeu=vals)
    for arg in ((0.9, 0.2, 1.3), 0.9, "sdxl"):
        with pytest.raises(ValueError, match="freeu"):
            AnimateDiffDenoiser(None, 4, 64, 64, freeu=arg)
        with pytest.raises(ValueError, match="freeu"):
            as_freeu(arg, "cpu")
    with pytest.raises(ValueError, match="UNetMotionModel"):   # good values pass on to the next check
        AnimateDiffDenoiser(None, 4, 64, 64, freeu=(0.9, 0.2, 1.3, 1.4))
    fu = FreeU(0.9, 0.2, 1.3, 1.4, device="cpu")
    tab = fu.table
    assert torch.equal(tab, torch.tensor([[0.9, 1.3], [0.2, 1.4]]))      # (s, b) per stage
    with pytest.raises(ValueError):
        fu.set(0.9, 0.2, 1.3, float("nan"))
    assert torch.equal(tab, torch.tensor([[0.9, 1.3], [0.2, 1.4]]))      # a refused set leaves the table alone
    fu.set(0.6, 0.4, 1.1, 1.2)
    assert fu.table is tab and torch.equal(tab, torch.tensor([[0.6, 1.1], [0.4, 1.2]]))
    assert as_freeu(fu) is fu and as_freeu(None) is None


def test_kernel_wrapper_has_no_cpu_path():
    from video_style_transfer_amd import _lib, kernels as K
    x = torch.zeros(2 * 16, 64, dtype=torch.bfloat16)
    with pytest.raises(_lib.VstError):
        K.freeu(x, x.clone(), 2, 4, 4, torch.ones(2, 2), 0)


def test_library_refuses_bad_arguments_without_gpu():
    """vst_freeu returns VST_ERR_ARG (1) before any launch; the pointers are never dereferenced."""
    from video_style_transfer_amd import _lib
    lib = _lib.load()
    X, S, XO, SO, T = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20

    def call(x=X, ldx=64, Cx=64, skip=S, lds=64, Cs=64, x_out=XO, ldxo=64, skip_out=SO, ldso=64, nimg=2, H=4, W=4,
             table=T, stage=0):
        return lib.vst_freeu(x, ldx, Cx, skip, lds, Cs, x_out, ldxo, skip_out, ldso, nimg, H, W, table, stage, None)

    bad = [dict(H=1), dict(W=1), dict(H=0), dict(Cs=60), dict(Cs=4), dict(Cx=72, ldx=72, ldxo=72), dict(Cx=8),
           dict(stage=2), dict(stage=-1), dict(nimg=0),
           dict(x=None), dict(skip=None), dict(x_out=None), dict(skip_out=None), dict(table=None),
           dict(skip_out=S), dict(skip_out=S + 64), dict(skip_out=S - 64),      # overlaps skip
           dict(skip_out=X), dict(skip_out=XO), dict(x_out=S),                   # ... or another operand
           dict(x_out=X + 128), dict(x_out=X, ldxo=72, ldx=64),                  # x_out over x but not x itself
           dict(lds=56), dict(ldso=60), dict(ldx=68, ldxo=68),                   # stride < channels / not 16 bytes
           dict(skip=S + 2), dict(skip_out=SO + 8), dict(x=X + 4)]               # base alignment
    for kw in bad:
        assert call(**kw) == 1, kw
    # every pointer NULL: refused like everything else
    assert lib.vst_freeu(None, 64, 64, None, 64, 64, None, 64, None, 64, 2, 4, 4, None, 0, None) == 1
    for kw in (dict(H=1), dict(Cs=60), dict(Cx=72), dict(stage=2)):   # ... and so is each size with NULL pointers
        args = dict(ldx=64, Cx=64, lds=64, Cs=64, ldxo=64, ldso=64, nimg=2, H=4, W=4, stage=0)
        args.update(kw)
        assert call(x=None, skip=None, x_out=None, skip_out=None, table=None, **args) == 1
    assert call(H=4000, W=200) == 3   # H + W past the trig table: unsupported, not a bad argument


def test_training_refuses_freeu():
    from video_style_transfer_amd.autograd import refuse_freeu, unet_train_tokens
    from video_style_transfer_amd.config import UNetMotionConfig
    from video_style_transfer_amd.train import TrainStep
    from video_style_transfer_amd.unet_motion import UNetMotionModel
    with torch.device("meta"):
        unet = UNetMotionModel(UNetMotionConfig.tiny())
    assert unet.freeu is None
    refuse_freeu(unet)
    with pytest.raises(NotImplementedError, match="freeu"):
        unet_train_tokens(unet, None, 2, 4, 16, 16, None, None, freeu=(0.9, 0.2, 1.3, 1.4))
    unet.freeu = types.SimpleNamespace(values=(0.9, 0.2, 1.3, 1.4))   # what enable_freeu leaves (no device here)
    with pytest.raises(NotImplementedError, match="freeu"):
        unet_train_tokens(unet, None, 2, 4, 16, 16, None, None)
    step = TrainStep(unet, None, None)
    with pytest.raises(NotImplementedError, match="freeu"):
        step._loss(torch.zeros(1, 4, 4, 16, 16), None, None, None, None)
    unet.disable_freeu()
    assert unet.freeu is None
