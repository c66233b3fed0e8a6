"""CPU-only tests of the MTF-GLP baselines: the float64 host definitions ``metrics.pan_lowpass_bands``, ``glp_moments`` and
``mtf_glp`` (modes "glp", "cbd", "hpm") and ``tiling.classical_fuse`` on host arrays.  Unpinned: the Pansharpening Toolbox is not
available, so the definition is held to its own algebra and to a scene on which the method must help.

The file also holds what the GPU test (tests/test_gpu_glp.py) needs: the shapes, the inputs and a float32 restatement of the
low-pass stage (``lowpass_float32``).

The low-pass of the definition is centred, L_c = mean(P) + LP_c(P - mean(P)), because the plain chain LP_c does not reproduce
constants: ``mtf_kernel`` sums to one, but the toolbox's 23 interpolation taps sum to 0.999999999596, so an interpolated sample
of a constant image is low by 4.04e-10 per pass and by up to 1.21e-9 at x4 (test_lowpass_of_a_constant).  With the plain chain
the three properties below hold only to that level -- measured then: affine invariance with a shift of 0.3 to 2.0e-10 .. 3.6e-10
where 1e-10 is asked, the two orders of equalising and filtering to 2.9e-10 where 1e-12 is asked, and a constant PAN of 0.5
gave finite bands (var(L_c) = 5e-20) where NaN is asked.  With the centred chain they are exact up to rounding;
test_centred_against_plain_chain holds the distance between the two chains to the bound that follows from the tap sum."""
import numpy as np
import pytest
import torch

from tmdiff_amd import metrics as M

U = 2.0 ** -24
# [B, C, H, W], ratio, sensor or gains: the smallest shapes that reach every path of the device kernels
GLP_CASES = [
    ((2, 4, 72, 100), 4, "QB"),                 # LR 18 x 25: two ragged 16-tiles per axis, W % 4 == 0
    ((1, 8, 64, 64), 4, "WV3"),                 # one full tile, the WV3 gains
    ((1, 3, 36, 70), 2, ((0.3, 0.25, 0.35), 0.15)),   # T = 3, W % 4 != 0: the scalar path
    ((1, 1, 8, 8), 4, ((0.29,), 0.15)),         # one band, an image smaller than a tile
]
POLY23_SUM = 2.0 * sum(M.POLY23_TAPS)           # 0.999999999596: what an interpolated sample of a constant image becomes


def glp_inputs(seed, b, c, h, w):
    """(ms_exp, pan) float32 tensors: bands uniform in [0.1, 0.9], the PAN a fixed positive mix of them plus noise (it stays
    in [0.1, 0.9] too, so every low-pass band stays above 0.05 and hpm's division is benign)."""
    g = torch.Generator().manual_seed(seed)
    ms = 0.1 + 0.8 * torch.rand(b, c, h, w, generator=g)
    wts = torch.arange(1, c + 1, dtype=torch.float32)
    wts = 0.8 * wts / wts.sum()
    pan = (ms * wts[None, :, None, None]).sum(1, keepdim=True) + 0.2 * (0.1 + 0.8 * torch.rand(b, 1, h, w, generator=g))
    return ms.contiguous(), pan.contiguous()


def fma32(a, b, c):
    """fma(a, b, c) of float32 arrays rounded once: the product of two float32 is exact in float64, and the float64 sum is rounded
    to float32 (a double rounding that differs from the fused operation in rare ties only)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def lowpass_float32(pan, gains, ratio):
    """pan_lowpass_bands in float32 in the device's documented orders: the filter as one chain of fused multiply-adds from 0 over
    the taps in row-major order (csrc/mtf.hip), then ``upsample_poly23`` stage by stage, H then W, each interpolated sample
    one chain from 0 over j = 5 .. 0 of acc = fma(a_j, x[lo - j] + x[lo + 1 + j], acc) with the pair added in float32 first
    (csrc/resample.hip).  pan float32 [B, 1, H, W] -> float32 [B, C, H, W]."""
    pan = np.asarray(pan, dtype=np.float32)
    b, _, h, w = pan.shape
    taps = np.stack([M.mtf_kernel(g, ratio) for g in gains]).astype(np.float32)
    k, rad, o = taps.shape[-1], taps.shape[-1] // 2, ratio // 2
    ho, wo = h // ratio, w // ratio
    xp = np.pad(pan[:, 0], ((0, 0), (rad, rad), (rad, rad)), mode="edge")
    low = np.zeros((b, len(gains), ho, wo), np.float32)
    for u in range(k):
        for v in range(k):
            win = xp[:, None, o + u:o + u + ratio * (ho - 1) + 1:ratio, o + v:o + v + ratio * (wo - 1) + 1:ratio]
            low = fma32(np.broadcast_to(taps[None, :, u, v, None, None], low.shape), np.broadcast_to(win, low.shape), low)
    y = low
    a32 = np.asarray(M.POLY23_TAPS, dtype=np.float32)
    for p in ((1, 0) if ratio == 4 else (1,)):
        for axis in (-2, -1):
            y = np.moveaxis(y, axis, -1)
            n = y.shape[-1]
            lo = np.arange(n) - p
            acc = np.zeros(y.shape, np.float32)
            for j in range(5, -1, -1):
                acc = fma32(np.broadcast_to(a32[j], y.shape), y[..., (lo - j) % n] + y[..., (lo + 1 + j) % n], acc)
            up = np.empty(y.shape[:-1] + (2 * n,), np.float32)
            up[..., p::2] = y
            up[..., 1 - p::2] = acc
            y = np.moveaxis(up, -1, axis)
    return y


def _scene(c=4, n=64, seed=0):
    """A c-band n x n scene: ONE smooth field with a gain and an offset per band plus white detail shared across the bands with a
    weight per band; the PAN is the band mean."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:n, 0:n] / float(n)
    field = np.sin(2 * np.pi * yy) * np.cos(2 * np.pi * 1.5 * xx)
    detail = 0.08 * rng.standard_normal((n, n))
    wts = np.array([1.0, 0.8, 1.2, 0.9, 1.1, 0.7, 1.3, 1.0])[:c]
    scene = np.stack([0.5 + 0.05 * k + (0.2 - 0.03 * k) * field + wts[k] * detail for k in range(c)])
    return scene, scene.mean(0)


@pytest.fixture(scope="module")
def pair():
    """(scene, pan, ms_exp) of the QB sanity scene: the MS is Wald's degradation of the scene, interpolated back."""
    scene, pan = _scene()
    return scene, pan, M.upsample_poly23(M.mtf_degrade(scene, "QB"))


def test_moment_fields_and_values():
    assert M.GLP_MOMENT_FIELDS == ("mean_ms", "mean_lp", "mean_pan", "var_ms", "var_lp", "cov_ms_lp", "var_pan")
    assert M.GLP_MODES == ("glp", "cbd", "hpm")
    rng = np.random.default_rng(1)
    m, lp, p = rng.random((2, 3, 8, 12)), rng.random((2, 3, 8, 12)), rng.random((2, 1, 8, 12))
    mo = M.glp_moments(m, p, lp)
    assert mo.shape == (2, 3, 7)
    for b in range(2):
        for c in range(3):
            cov = np.cov(m[b, c].ravel(), lp[b, c].ravel(), bias=True)
            want = [m[b, c].mean(), lp[b, c].mean(), p[b, 0].mean(), cov[0, 0], cov[1, 1], cov[0, 1], p[b, 0].var()]
            np.testing.assert_allclose(mo[b, c], want, rtol=1e-12, atol=0)
    assert np.array_equal(M.glp_moments(m[0], p[0, 0], lp[0]), mo[0])          # pan as [H, W]


def _plain_chain(pan, gain, ratio):
    return M.upsample_poly23(M.fir_decimate(pan, M.mtf_kernel(gain, ratio), ratio), ratio)


def test_pan_lowpass_bands_is_the_stated_chain():
    rng = np.random.default_rng(2)
    pan = rng.random((2, 1, 16, 24))
    got = M.pan_lowpass_bands(pan, "QB", 4)
    assert got.shape == (2, 4, 16, 24)
    first = pan[:, 0, :1, :1]
    mean = first + (pan[:, 0] - first).mean((1, 2), keepdims=True)
    for c, g in enumerate(M.MTF_GAINS["QB"][0]):
        assert np.array_equal(got[:, c], mean + _plain_chain(pan[:, 0] - mean, g, 4))
    # the MS gains, not the PAN gain: pan_lowpass is another image
    assert np.abs(got[:, :1] - M.pan_lowpass(pan, "QB")).max() > 1e-3
    assert M.pan_lowpass_bands(pan[0, 0], (0.3, 0.2), 2, ratio=2).shape == (2, 16, 24)


def test_centred_against_plain_chain():
    """LP_c is linear, so mean + LP_c(P - mean) - LP_c(P) = mean (1 - LP_c(1)): at most 3 (1 - POLY23_SUM) |mean| at x4 and one
    two passes' worth at x2 (and the rounding of two 1681-term sums of values below one, 2 * 1681 * 2^-53 < 4e-13)."""
    rng = np.random.default_rng(4)
    pan = 0.1 + 0.8 * rng.random((16, 24))
    for ratio, passes in ((4, 3.0), (2, 2.0)):
        got = M.pan_lowpass_bands(pan, (0.3,), 1, ratio)[0]
        err = np.abs(got - _plain_chain(pan, 0.3, ratio)).max()
        assert 0.0 < err <= passes * (1.0 - POLY23_SUM) * pan.mean() + 4e-13, (ratio, err)


def test_cbd_gain_is_the_least_squares_slope(pair):
    _, pan, ms = pair
    lp = M.pan_lowpass_bands(pan, "QB", 4)
    mo = M.glp_moments(ms, pan, lp)
    for c in range(4):
        a = np.sqrt(mo[c, 3] / mo[c, 4])
        plc = a * (lp[c] - mo[c, 2]) + mo[c, 0]
        slope = np.polyfit(plc.ravel(), ms[c].ravel(), 1)[0]
        gain = mo[c, 5] / (a * mo[c, 4])
        assert abs(gain - slope) <= 1e-12 * abs(slope), (c, gain, slope)
        # ... and it is the gain the definition injects with
        f = M.mtf_glp(ms, pan, "QB", mode="cbd", pan_lp=lp)[c]
        pc = a * (pan - mo[c, 2]) + mo[c, 0]
        np.testing.assert_allclose(f, ms[c] + slope * (pc - plc), rtol=1e-11, atol=0)


@pytest.mark.parametrize("mode", M.GLP_MODES)
@pytest.mark.parametrize("alpha, beta", [(3.0, 0.0), (2.5, 0.3), (0.5, -0.1), (1.0, 0.2)])
def test_affine_invariance(pair, mode, alpha, beta):
    """alpha * pan + beta (alpha > 0) in place of pan leaves the result unchanged to 1e-10 of its largest value: the
    equalisation removes the map, the centred low-pass commutes with it."""
    _, pan, ms = pair
    want = M.mtf_glp(ms, pan, "QB", mode=mode)
    got = M.mtf_glp(ms, alpha * pan + beta, "QB", mode=mode)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"affine invariance {mode} alpha={alpha} beta={beta}: {err:.3e}")
    assert err <= 1e-10


def _equalised_both_ways(pair):
    _, pan, ms = pair
    gains = M.band_gains("QB", 4)
    lp = M.pan_lowpass_bands(pan, gains, 4)
    mo = M.glp_moments(ms, pan, lp)
    for c in range(4):
        a = np.sqrt(mo[c, 3] / mo[c, 4])
        pc = a * (pan - mo[c, 2]) + mo[c, 0]
        toolbox = M.pan_lowpass_bands(pc, (gains[c],), 1)[0]                  # filter the equalised PAN with the band's filter
        here = a * (lp[c] - mo[c, 2]) + mo[c, 0]
        yield c, np.abs(toolbox - here).max(), abs(mo[c, 0] - a * mo[c, 2])


def test_equalisation_equivalence(pair):
    """Filtering the equalised PAN per band (the Toolbox's order) equals this definition to 1e-12: the documented deviation
    changes nothing."""
    for c, err, _ in _equalised_both_ways(pair):
        print(f"equalisation both ways, band {c}: {err:.3e}")
        assert err <= 1e-12


def test_lowpass_of_a_constant():
    """The filter keeps a constant, the interpolator loses 1 - POLY23_SUM per pass; the centred low-pass keeps it exactly."""
    assert abs(POLY23_SUM - 0.999999999596) < 1e-12
    assert abs(M.mtf_kernel(0.3, 4).sum() - 1.0) < 1e-14
    lp = _plain_chain(np.ones((8, 8)), 0.3, 4)
    assert abs((1.0 - lp.min()) - 3.0 * (1.0 - POLY23_SUM)) < 1e-14 and lp.max() <= 1.0 + 1e-14     # 1.212e-9 at the worst sample
    assert abs(lp[2, 2] - 1.0) < 1e-14                                                    # a kept sample loses nothing
    for value in (1.0, 0.3, 1000.7):
        assert np.array_equal(M.pan_lowpass_bands(np.full((8, 8), value), (0.3, 0.2), 2), np.full((2, 8, 8), value))


@pytest.mark.parametrize("mode", ("glp", "cbd"))
def test_means(pair, mode):
    _, pan, ms = pair
    lp = M.pan_lowpass_bands(pan, "QB", 4)
    mo = M.glp_moments(ms, pan, lp)
    f = M.mtf_glp(ms, pan, "QB", mode=mode, pan_lp=lp)
    for c in range(4):
        a = np.sqrt(mo[c, 3] / mo[c, 4])
        g = mo[c, 5] / (a * mo[c, 4]) if mode == "cbd" else 1.0
        want = mo[c, 0] + g * a * (mo[c, 2] - mo[c, 1])
        assert abs(f[c].mean() - want) <= 1e-12, (c, f[c].mean(), want)


def test_constant_pan(pair):
    """A constant PAN gives non-finite output in every band and no exception: its low-pass is constant, var(L_c) is 0."""
    _, pan, ms = pair
    for mode in M.GLP_MODES:
        for value in (0.5, 0.3, 0.0):
            with np.errstate(all="ignore"):
                f = M.mtf_glp(ms, np.full_like(pan, value), "QB", mode=mode)
            assert f.shape == ms.shape and not np.isfinite(f).any(axis=(1, 2)).any(), (mode, value)


@pytest.mark.parametrize("mode", M.GLP_MODES)
def test_constant_lowpass(pair, mode):
    _, pan, ms = pair
    lp = M.pan_lowpass_bands(pan, "QB", 4)
    lp[2] = 0.4                                                                # one band's low-pass PAN is constant
    with np.errstate(all="ignore"):
        f = M.mtf_glp(ms, pan, "QB", mode=mode, pan_lp=lp)
    assert not np.isfinite(f[2]).any() and np.isfinite(f[[0, 1, 3]]).all()


def test_bad_arguments(pair):
    _, pan, ms = pair
    with pytest.raises(ValueError, match="mode"):
        M.mtf_glp(ms, pan, "QB", mode="gsa")
    with pytest.raises(ValueError, match="ratio"):
        M.mtf_glp(ms, pan, "QB", ratio=3)
    with pytest.raises(ValueError, match="ratio"):
        M.pan_lowpass_bands(pan, "QB", 4, ratio=8)
    with pytest.raises(ValueError, match="multiples"):
        M.mtf_glp(ms[:, :62], pan[:62], "QB")
    with pytest.raises(ValueError, match="multiples"):
        M.pan_lowpass_bands(pan[:, :63], "QB", 4)
    with pytest.raises(ValueError):
        M.mtf_glp(ms, pan, "WV3")                                              # eight gains for four bands
    with pytest.raises(ValueError):
        M.glp_moments(ms, pan[:32], ms)


def test_every_mode_beats_the_interpolated_ms(pair):
    """Sanity of the method: against the scene, every mode has a strictly lower ERGAS than ms_exp has.  Measured on this scene:
    ms_exp 3.4862, glp 0.9162, cbd 0.9163, hpm 0.9178."""
    scene, pan, ms = pair
    base = M.ergas(scene, ms, hwc=False)
    got = {mode: M.ergas(scene, M.mtf_glp(ms, pan, "QB", mode=mode), hwc=False) for mode in M.GLP_MODES}
    print(f"ERGAS: ms_exp {base:.4f}  " + "  ".join(f"{k} {v:.4f}" for k, v in got.items()))
    assert all(v < base for v in got.values()), (base, got)


def test_hwc_layout(pair):
    _, pan, ms = pair
    want = M.mtf_glp(ms, pan, "QB", mode="cbd")
    got = M.mtf_glp(np.moveaxis(ms, 0, -1), pan, "QB", mode="cbd", hwc=True)
    assert got.shape == (64, 64, 4) and np.array_equal(np.moveaxis(got, -1, 0), want)


def test_classical_fuse_on_host_arrays():
    from tmdiff_amd.tiling import classical_fuse, consistency_refine
    rng = np.random.default_rng(5)
    lr, pan = 0.1 + 0.8 * rng.random((2, 4, 8, 12)), 0.1 + 0.8 * rng.random((2, 1, 32, 48))
    for mode in M.GLP_MODES:
        want = M.mtf_glp(M.upsample_poly23(lr), pan, "QB", 4, mode)
        got = classical_fuse(lr, pan, "QB", mode=mode)
        assert isinstance(got, np.ndarray) and np.array_equal(got, want)
    got = classical_fuse(torch.from_numpy(lr), torch.from_numpy(pan), "QB", mode="glp")
    assert torch.is_tensor(got) and np.array_equal(got.numpy(), M.mtf_glp(M.upsample_poly23(lr), pan, "QB", 4, "glp"))
    refined = classical_fuse(lr, pan, "QB", consistency={"iters": 2})
    assert np.array_equal(refined, consistency_refine(M.mtf_glp(M.upsample_poly23(lr), pan, "QB"), lr, "QB", 4, iters=2))
    with pytest.raises(ValueError, match="score"):
        classical_fuse(lr, pan, "QB", score=True)
    with pytest.raises(ValueError, match="mode"):
        classical_fuse(lr, pan, "QB", mode="gsa")
    with pytest.raises(ValueError, match="pan"):
        classical_fuse(lr, pan[..., :40], "QB")


def test_validation_options_reach_baselines():
    from tmdiff_amd import evaluate
    from tmdiff_amd.train import validation_options
    assert evaluate.BASELINES == ("exp", "glp", "cbd", "hpm")
    assert validation_options({"full_resolution": True}) == {"full_resolution": True}
    assert validation_options({}) == {}
    assert validation_options({"full_resolution": "hqnr", "sensor": "QB", "baselines": ["exp", "hpm"]}) == \
        {"full_resolution": True, "protocol": "hqnr", "sensor": "QB", "baselines": ("exp", "hpm")}
    assert validation_options({"full_resolution": True, "baselines": ["glp"]}) == \
        {"full_resolution": True, "baselines": ("glp",), "sensor": None}
    with pytest.raises(ValueError, match="baselines"):
        validation_options({"baselines": ["glp"]})
    with pytest.raises(ValueError, match="baselines"):
        evaluate.val_dataset(None, "QB", [], "unused", baselines=("glp",))          # the host-metric mode
    with pytest.raises(ValueError, match="baselines"):
        evaluate.val_dataset(None, "QB", [], "unused", full_resolution=True, baselines=("gsa",))
    with pytest.raises(ValueError, match="sensor"):
        evaluate.val_dataset(None, "GF2", [], "unused", full_resolution=True, baselines=("glp",))


def test_float32_restatement_of_the_lowpass():
    """lowpass_float32 stays within the a-priori bound of its chains of the float64 definition: (K^2 + 2) u for the filter of
    positive data under all-but-positive taps, and per interpolation pass 8 u times the taps' absolute sum 1.63."""
    (b, c, h, w), ratio, sensor = GLP_CASES[2]
    _, pan = glp_inputs(7, b, c, h, w)
    gains = M.mtf_gains(sensor, c)[0]
    got = lowpass_float32(pan.numpy(), gains, ratio)
    want = M.pan_lowpass_bands(pan.numpy(), gains, c, ratio)
    assert got.dtype == np.float32 and np.abs(got - want).max() <= (41 * 41 + 2 + 2 * 8 * 1.63) * U * np.abs(want).max()
