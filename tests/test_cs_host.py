"""CPU-only tests of the component-substitution baselines: the float64 host definitions ``metrics.plane_moments``, ``cs_coeffs``,
``cs_inject`` and ``cs_fuse`` (methods "gs", "gsa", "brovey"), ``tiling.cs_fuse`` on host arrays and the ``cs-*`` names of
``evaluate.val_dataset(baselines=...)``.  Unpinned: the Pansharpening Toolbox is not available, so the definition is held to its
own algebra, to numpy's least squares and to a scene on which the method must help.

The file also holds what the GPU test (tests/test_gpu_cs.py) needs: the shapes and the inputs."""
import numpy as np
import pytest
import torch

from test_glp_host import GLP_CASES, _scene, glp_inputs
from tmdiff_amd import metrics as M

# [B, C, H, W], ratio, sensor or gains: GLP's four and three that the Gram kernel needs
CS_CASES = GLP_CASES + [
    ((2, 14, 9, 7), None, None),                # the widest tile; 63 pixels: a tail inside a K group and inside a 16-byte load
    ((1, 3, 17, 241), None, None),              # 4097 pixels: whole chunks plus one pixel
    ((1, 8, 64, 64), 4, "WV3"),                 # viewed 4 bytes off a 16-byte boundary by the GPU test: the scalar path
]


def cs_inputs(seed, b, c, h, w):
    """(ms_exp, pan) float32 tensors as ``glp_inputs`` makes them; the bands there are independent, so S is well conditioned."""
    return glp_inputs(seed, b, c, h, w)


def _pair(seed=0, b=2, c=4, h=32, w=48):
    """A float64 batch for the algebra: bands that share a component, and a PAN that mixes them unevenly plus noise."""
    rng = np.random.default_rng(seed)
    shared = rng.random((b, 1, h, w))
    ms = 0.1 + 0.4 * shared + 0.4 * rng.random((b, c, h, w))
    wts = np.arange(1, c + 1) / np.arange(1, c + 1).sum()
    pan = (ms * wts[None, :, None, None]).sum(1) + 0.05 * rng.random((b, h, w))
    return ms, pan


def test_plane_moments_against_numpy():
    assert M.CS_METHODS == ("gs", "gsa", "brovey")
    ms, pan = _pair(1, 2, 3, 8, 12)
    mo = M.plane_moments(ms, pan)
    assert mo.shape == (2, 4, 5)
    for b in range(2):
        planes = np.concatenate([ms[b], pan[b][None]]).reshape(4, -1)
        assert np.abs(mo[b, :, :4] - np.cov(planes, bias=True)).max() <= 1e-12
        assert np.abs(mo[b, :, 4] - planes.mean(1)).max() <= 1e-12
        assert np.array_equal(mo[b, :, :4], mo[b, :, :4].T)                          # exactly symmetric
    assert np.array_equal(M.plane_moments(ms, pan[:, None]), mo)                      # pan as [..., 1, H, W]
    assert np.array_equal(M.plane_moments(ms[0], pan[0]), mo[0])
    ms[1, 1] = 0.3                                                                    # a constant plane: exact zeros
    mo = M.plane_moments(ms, pan)
    assert (mo[1, 1, :4] == 0.0).all() and (mo[1, :, 1] == 0.0).all() and mo[1, 1, 4] == 0.3 and (mo[0, :, :4] != 0.0).all()


def _gsa_case(seed=2, c=5, h=24, w=24):
    """Reduced-scale bands that are a shared component plus independent noise of the same size, and a PAN."""
    rng = np.random.default_rng(seed)
    shared = rng.standard_normal((1, h, w))
    m = 0.5 + 0.1 * (shared + rng.standard_normal((c, h, w)))
    p = (m * np.linspace(0.5, 1.5, c)[:, None, None]).sum(0) / c + 0.02 * rng.standard_normal((h, w))
    return m, p


def test_gsa_weights_are_the_least_squares_regression():
    m, p = _gsa_case()
    c = m.shape[0]
    low = M.plane_moments(m, p)
    cond = np.linalg.cond(low[:c, :c])
    print(f"gsa: cond(S_lr) = {cond:.2f}")
    assert cond < 100.0
    coef = M.cs_coeffs(low, low, "gsa")
    assert coef.shape == (2 * c + 3,)
    alpha = coef[:c]
    a_mat = np.concatenate([m.reshape(c, -1).T, np.ones((p.size, 1))], 1)
    want = np.linalg.lstsq(a_mat, p.ravel(), rcond=None)[0]
    assert np.abs(alpha - want[:c]).max() <= 1e-9 * np.abs(alpha).max()
    # the residual of the regression (with its intercept) is orthogonal to every centred band
    mc = m.reshape(c, -1) - m.reshape(c, -1).mean(1, keepdims=True)
    res = (p.ravel() - p.mean()) - alpha @ mc
    assert np.abs(mc @ res / p.size).max() <= 1e-12
    # full == low here, so the constants follow from the regression: mean_I = alpha . mu, mean_P as given
    assert abs(coef[2 * c + 1] - alpha @ m.reshape(c, -1).mean(1)) <= 1e-12 and coef[2 * c + 2] == low[c, c + 1]


def test_gsa_singular_system_is_nan():
    m, p = _gsa_case(3, 4)
    m[2] = m[0]                                                                       # a duplicated band: a pivot of exactly 0
    low = M.plane_moments(m, p)
    full = M.plane_moments(*_gsa_case(4, 4))
    assert np.isnan(M.cs_coeffs(full, low, "gsa")).all()
    both = M.cs_coeffs(np.stack([full, full]), np.stack([low, full]), "gsa")          # ... of that image only
    assert np.isnan(both[0]).all() and np.isfinite(both[1]).all()
    assert np.isfinite(M.cs_coeffs(full, None, "gs")).all()


def _fused(method, ms, pan, sensor="QB"):
    return M.cs_fuse(ms, pan, sensor, 4, method)


def _constants(method, ms, pan, sensor="QB"):
    low = M.plane_moments(*M.cs_reduced_pair(ms, pan, sensor, 4)) if method == "gsa" else None
    return M.cs_coeffs(M.plane_moments(ms, pan), low, method)


@pytest.mark.parametrize("method", M.CS_METHODS)
def test_identities(method):
    ms, pan = _pair()
    c = ms.shape[1]
    f = _fused(method, ms, pan)
    coef = _constants(method, ms, pan)
    assert f.shape == ms.shape and np.isfinite(f).all()
    assert np.array_equal(f, M.cs_inject(ms, pan, coef, method))
    alpha = coef[:, :c, None, None]
    inten = (alpha * ms).sum(1)
    pi = coef[:, 2 * c, None, None] * (pan - coef[:, 2 * c + 2, None, None]) + coef[:, 2 * c + 1, None, None]
    scale = np.abs(f).max()
    if method != "brovey":
        assert np.abs(f.mean((2, 3)) - ms.mean((2, 3))).max() <= 1e-12 * scale        # the injection has zero mean
        assert abs((coef[:, :c] * coef[:, c:2 * c]).sum(1) - 1.0).max() <= 1e-12      # sum_c alpha_c g_c = 1
        assert np.abs((alpha * f).sum(1) - pi).max() <= 1e-12 * scale                 # the fused intensity is P_I
    else:
        assert np.abs((alpha * f).sum(1) - inten * pi / (inten + 2.0 ** -52)).max() <= 1e-12 * scale
    if method != "gsa":
        assert np.array_equal(coef[:, :c], np.full((2, c), 1.0 / c))


@pytest.mark.parametrize("method", M.CS_METHODS)
@pytest.mark.parametrize("s, t", [(3.0, 0.0), (0.5, -0.1), (2.5, 0.3)])
def test_affine_invariance(method, s, t):
    ms, pan = _pair(5)
    want, got = _fused(method, ms, pan), _fused(method, ms, s * pan + t)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"affine invariance {method} s={s} t={t}: {err:.3e}")
    assert err <= 1e-12


def test_constant_pan_is_not_finite():
    ms, pan = _pair(6, 1, 4, 16, 16)
    for method in M.CS_METHODS:
        for value in (0.5, 0.0):
            with np.errstate(all="ignore"):
                f = _fused(method, ms, np.full_like(pan, value))
            assert f.shape == ms.shape and not np.isfinite(f).any(), (method, value)


@pytest.mark.parametrize("ratio", (4, 2))
def test_reduced_scale_ms_is_the_raw_ms(ratio):
    rng = np.random.default_rng(7)
    lr = rng.random((2, 3, 8, 12))
    ms_exp = M.upsample_poly23(lr, ratio)
    pan = rng.random((2, 8 * ratio, 12 * ratio))
    low_ms, low_pan = M.cs_reduced_pair(ms_exp, pan, ((0.3, 0.3, 0.3), 0.15), ratio)
    assert np.array_equal(low_ms, lr)                                                 # bit for bit
    assert np.array_equal(low_pan, M.mtf_degrade(pan[:, None], 0.15, ratio)[:, 0])
    sensor = ((0.3, 0.3, 0.3), 0.15)
    assert np.array_equal(M.cs_fuse(ms_exp, pan, sensor, ratio, "gsa"), M.cs_fuse(ms_exp, pan, sensor, ratio, "gsa", lr_ms=lr))


def test_every_method_beats_the_interpolated_ms():
    """Sanity of the method on the scene of test_glp_host: against the scene, every method has a strictly lower ERGAS than
    ms_exp has; all three methods are in the assertion.  Measured on this scene: ms_exp 3.4862, gs 1.7659, gsa 1.7628, brovey
    1.7534."""
    scene, pan = _scene()
    ms = M.upsample_poly23(M.mtf_degrade(scene, "QB"))
    base = M.ergas(scene, ms, hwc=False)
    got = {m: M.ergas(scene, M.cs_fuse(ms, pan, "QB", 4, m), hwc=False) for m in M.CS_METHODS}
    print(f"ERGAS: ms_exp {base:.4f}  " + "  ".join(f"{k} {v:.4f}" for k, v in got.items()))
    assert all(v < base for v in got.values()), (base, got)


def test_hwc_layout():
    ms, pan = _pair(8, 1, 4, 16, 24)
    want = M.cs_fuse(ms[0], pan[0], "QB", 4, "gsa")
    got = M.cs_fuse(np.moveaxis(ms[0], 0, -1), pan[0], "QB", 4, "gsa", hwc=True)
    assert got.shape == (16, 24, 4) and np.array_equal(np.moveaxis(got, -1, 0), want)
    assert np.array_equal(M.cs_fuse(np.moveaxis(ms[0], 0, -1), pan[0][..., None], "QB", 4, "gs", hwc=True),
                          np.moveaxis(M.cs_fuse(ms[0], pan[0], None, 4, "gs"), 0, -1))


def test_bad_arguments():
    ms, pan = _pair(9, 1, 4, 16, 16)
    with pytest.raises(ValueError, match="C <= 14"):
        M.cs_fuse(np.zeros((15, 8, 8)), np.zeros((8, 8)), method="gs")
    with pytest.raises(ValueError, match="ratio"):
        M.cs_fuse(ms, pan, "QB", ratio=3)
    with pytest.raises(ValueError, match="multiples"):
        M.cs_fuse(ms[..., :14], pan[..., :14], "QB")
    with pytest.raises(ValueError, match="belong"):
        M.cs_fuse(ms, pan[..., :12], "QB")
    with pytest.raises(ValueError, match="method"):
        M.cs_fuse(ms, pan, "QB", method="hpm")
    with pytest.raises(ValueError, match="sensor"):
        M.cs_fuse(ms, pan)
    with pytest.raises(ValueError, match="lr_ms"):
        M.cs_fuse(ms, pan, "QB", lr_ms=np.zeros((1, 4, 5, 4)))
    with pytest.raises(ValueError, match="low"):
        M.cs_coeffs(M.plane_moments(ms, pan), None, "gsa")
    with pytest.raises(ValueError, match="coef"):
        M.cs_inject(ms, pan, np.zeros((1, 10)), "gs")


def test_tiling_cs_fuse_on_host_arrays():
    from tmdiff_amd.tiling import classical_fuse, consistency_refine, cs_fuse
    rng = np.random.default_rng(5)
    lr, pan = 0.1 + 0.8 * rng.random((2, 4, 8, 12)), 0.1 + 0.8 * rng.random((2, 1, 32, 48))
    for method in M.CS_METHODS:
        want = M.cs_fuse(M.upsample_poly23(lr), pan, "QB", 4, method)
        got = cs_fuse(lr, pan, "QB", method=method)
        assert isinstance(got, np.ndarray) and np.array_equal(got, want)
    got = cs_fuse(torch.from_numpy(lr), torch.from_numpy(pan), method="gs")
    assert torch.is_tensor(got) and np.array_equal(got.numpy(), M.cs_fuse(M.upsample_poly23(lr), pan, None, 4, "gs"))
    refined = cs_fuse(lr, pan, "QB", consistency={"iters": 2})
    assert np.array_equal(refined, consistency_refine(M.cs_fuse(M.upsample_poly23(lr), pan, "QB"), lr, "QB", 4, iters=2))
    with pytest.raises(ValueError, match="score"):
        cs_fuse(lr, pan, "QB", score=True)
    with pytest.raises(ValueError, match="method"):
        cs_fuse(lr, pan, "QB", method="hpm")
    with pytest.raises(ValueError, match="sensor"):
        cs_fuse(lr, pan)
    with pytest.raises(ValueError, match="pan"):
        cs_fuse(lr, pan[..., :40], "QB")
    with pytest.raises(ValueError, match="mode"):
        classical_fuse(lr, pan, "QB", mode="gsa")                                     # the GLP entry point keeps its modes


def test_baseline_names_and_validation_options():
    from tmdiff_amd import evaluate
    from tmdiff_amd.train import validation_options
    assert evaluate.CS_BASELINES == ("cs-gs", "cs-gsa", "cs-brovey")
    assert evaluate.CS_BASELINES == tuple("cs-" + m for m in M.CS_METHODS)
    assert evaluate.BASELINES == ("exp", "glp", "cbd", "hpm")
    assert validation_options({"full_resolution": "hqnr", "sensor": "QB", "baselines": ["exp", "cs-gsa"]}) == \
        {"full_resolution": True, "protocol": "hqnr", "sensor": "QB", "baselines": ("exp", "cs-gsa")}
    with pytest.raises(ValueError, match="baselines"):
        evaluate.val_dataset(None, "QB", [], "unused", full_resolution=True, baselines=("cs-nope",))
    with pytest.raises(ValueError, match="baselines"):
        evaluate.val_dataset(None, "QB", [], "unused", full_resolution=True, baselines=("cs-gsa", "cs-gsa"))
    with pytest.raises(ValueError, match="baselines"):
        evaluate.val_dataset(None, "QB", [], "unused", baselines=("cs-gsa",))          # the host-metric mode
