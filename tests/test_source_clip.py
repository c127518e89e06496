"""Video-to-video, host side: the start index of a source-clip run and the wrappers' refusals.
Needs the built library but no GPU."""
import numpy as np
import pytest
import torch


@pytest.mark.parametrize("n,strength,want", [(50, 0.3, 35), (50, 0.5, 25), (50, 0.58, 22), (50, 1.0, 0),
                                             (50, 0.02, 49), (10, 0.7, 3), (10, 0.3, 7), (4, 0.75, 1)])
def test_start_index_table(n, strength, want):
    from video_style_transfer_amd.scheduler import start_index
    assert start_index(n, strength) == want


@pytest.mark.parametrize("n,strength", [(50, 0.0), (50, -0.3), (50, 1.0000001), (50, 2.0), (50, float("nan")),
                                        (50, float("inf")), (50, 0.01), (4, 0.2)])
def test_start_index_refusals(n, strength):
    from video_style_transfer_amd.scheduler import start_index
    with pytest.raises(ValueError):
        start_index(n, strength)


def test_start_index_never_leaves_the_table():
    from video_style_transfer_amd.scheduler import start_index
    for n in (1, 4, 10, 50):
        for k in range(1, 1001):
            try:
                t = start_index(n, k / 1000)
            except ValueError:
                assert int(n * (k / 1000)) == 0
                continue
            assert 0 <= t <= n - 1 and n - t == min(int(n * (k / 1000)), n)


def test_wrappers_refuse_cpu_tensors():
    from video_style_transfer_amd import _lib, kernels as K
    z = torch.zeros(1, 4, 2, 3, 3)
    sig = torch.ones(5)
    step = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(_lib.VstError):
        K.noise_latents(z, z.clone(), sig, step)
    with pytest.raises(_lib.VstError):
        K.euler_cfg_step_masked(torch.zeros(2 * 18, 4, dtype=torch.bfloat16), z, sig, step, z.clone(), z.clone(),
                                torch.ones(1, 2, 3, 3))
    with pytest.raises(_lib.VstError):
        K.euler_cfg_step(torch.zeros(2 * 18, 4, dtype=torch.bfloat16), z, sig, step)
    with pytest.raises(_lib.VstError):
        K.u8_to_frames(torch.zeros(1, 2, 2, 3, dtype=torch.uint8))


def test_entries_refuse_null_and_empty_without_gpu():
    from video_style_transfer_amd import _lib
    lib = _lib.load()
    assert lib.vst_noise_latents(None, 1, 1, 1, 1, 8, None) == 1
    assert lib.vst_noise_latents(1, 1, 1, None, 1, 8, None) == 1  # no step counter
    assert lib.vst_noise_latents(1, 1, 1, 1, 1, 0, None) == 1  # empty
    ok = dict(noise=1, ncopy=2, g=7.5, lat=1, B=2, Cl=4, F=3, HW=35, sig=1, step=1, z0=1, eps=1, mask=1, mc=2)

    def masked(**kw):
        a = dict(ok, **kw)
        return lib.vst_euler_cfg_step_masked(a["noise"], a["ncopy"], a["g"], a["lat"], a["B"], a["Cl"], a["F"],
                                             a["HW"], a["sig"], a["step"], a["z0"], a["eps"], a["mask"], a["mc"], None)
    for bad in (dict(noise=None), dict(lat=None), dict(sig=None), dict(step=None), dict(z0=None), dict(eps=None),
                dict(mask=None), dict(ncopy=3), dict(ncopy=0), dict(B=0), dict(Cl=0), dict(F=-1), dict(HW=0),
                dict(mc=3), dict(mc=0)):
        assert masked(**bad) == 1, bad

    def plain(**kw):
        a = dict(ok, **kw)
        return lib.vst_euler_cfg_step(a["noise"], a["ncopy"], a["g"], a["lat"], a["B"], a["Cl"], a["F"], a["HW"],
                                      a["sig"], a["step"], None)
    for bad in (dict(noise=None), dict(lat=None), dict(sig=None), dict(step=None), dict(ncopy=3), dict(ncopy=0),
                dict(B=0), dict(Cl=0), dict(F=-1), dict(HW=0)):
        assert plain(**bad) == 1, bad
    assert lib.vst_u8_to_frames(None, 1, 3, 4, 1, 3, None) == 1
    assert lib.vst_u8_to_frames(1, 1, 3, 4, None, 3, None) == 1
    assert lib.vst_u8_to_frames(1, 0, 3, 4, 1, 3, None) == 1
    assert lib.vst_u8_to_frames(1, 1, 3, 0, 1, 3, None) == 1
    assert lib.vst_u8_to_frames(1, 1, 3, 4, 1, 2, None) == 1  # ldd < C


def test_u8_normalisation_expression_is_ieee():
    """The kernel evaluates (v / 255 - 0.5) / 0.5 with IEEE fp32 operations (a correctly rounded division, an exact
    subtraction, an exact doubling).  numpy's float32 arithmetic is the same chain; it must give torch's values for
    all 256 inputs, so no table is needed."""
    v = np.arange(256, dtype=np.float32)
    x = (v / np.float32(255) - np.float32(0.5)) / np.float32(0.5)
    ref = (torch.arange(256, dtype=torch.uint8).float() / 255 - 0.5) / 0.5
    assert np.array_equal(x, ref.numpy())
