"""CPU-only tests of Wald's consistency as a solve: the float64 definition ``metrics.consistency_solve`` (CGLS per plane on the
correction d = f - f0), ``tiling.consistency_solve`` on host data, and the option dictionaries of the fuse functions and of the
sampler.

The definition is held to what was measured when it was proposed (on the 48 x 48 white-noise scene of
tests/test_mtf_adjoint_host.py the residual falls strictly, ends below 0.1 of its start after 8 iterations and below a third of
what 8 Landweber steps leave) and to the dense operator of ``metrics.fir_decimate`` at 24 x 24: the pseudo-inverse solution with
damp = 0, the solution of the normal equations with damp > 0.

The file also holds what the GPU test (tests/test_gpu_consistency_cg.py) is measured against: its cases (``CG_CASES``) and a
float32 restatement of the device's arithmetic (``solve_float32``): float32 vectors, A and A^T in the kernels' summation orders
(``fir_float32``, ``adjoint_float32``), float64 dots of the float32 vectors, alpha and beta formed in float64 and rounded to
float32 once, one fused multiply-add per element.  The fp32 and fp64 recurrences drift apart with the iteration count and no
bound on that drift can be derived, so the restatement's distance from the definition is measured here, on the correction d,
as max |d32 - d64| / max |d64| in units of u = 2^-24 (``CG_RESTATEMENT_U``), and the device is held to 4 times the figure,
rounded up -- the margin of the adjoint's tests, for the same reason (the restatement's fused multiply-add is emulated)."""
import numpy as np
import pytest
import torch

from test_mtf_adjoint_host import adjoint_float32
from test_mtf_host import U, fir_float32

# name -> (sensor or explicit band gains, ratio, (B, C, H, W)); 8 iterations, damp 0 each, and the first once more with damp
CG_CASES = {
    "QB x4 48": ("QB", 4, (1, 4, 48, 48)),                    # every adjoint tile is a border tile
    "3 bands x4 200x136": ((0.34, 0.29, 0.22), 4, (2, 3, 200, 136)),   # interior tiles, several partial sums per plane, a batch
    "WV3 x2 70": ("WV3", 2, (1, 8, 70, 70)),
    "QB x1 40x24": ("QB", 1, (1, 4, 40, 24)),
}
CG_ITERS = 8
CG_DAMP = 1e-3
# worst |d32 - d64| / max |d64| of solve_float32 against the definition in u, as test_float32_restatement measures it (and holds
# it to); "damp": the first case with damp = CG_DAMP
CG_RESTATEMENT_U = {"QB x4 48": 256.949, "3 bands x4 200x136": 397.538, "WV3 x2 70": 115.871, "QB x1 40x24": 180.404, "damp": 227.850}
# the gap of the dense check, measured once: max |f - closed form| / max |closed form correction|
DENSE_GAP = {"pinv": 2.103e-14, "damped": 3.090e-14}


def cg_scene(name):
    """(f0, lr) float32 arrays of a case: lr = A(white-noise truth), f0 = ``upsample_poly23(lr)`` (ratio 1: lr itself)."""
    from tmdiff_amd import metrics
    sensor, ratio, shape = CG_CASES[name]
    truth = np.random.default_rng(shape[2] * 1000 + shape[3]).random(shape)
    lr = metrics.mtf_degrade(truth, sensor, ratio).astype(np.float32)
    f0 = (metrics.upsample_poly23(lr, ratio) if ratio > 1 else lr).astype(np.float32)
    return f0, lr


def cg_tol_u(key):
    """The GPU test's tolerance in u: 4 x the restatement's figure, rounded up."""
    return float(np.ceil(4.0 * CG_RESTATEMENT_U[key]))


def correction_error_u(f, f0, want, want0):
    """max |d - d_want| / max |d_want| in u, d = f - f0 formed in float64 (exact for float32 f and f0 within a binade or two)."""
    d, dw = np.asarray(f, dtype=np.float64) - np.asarray(f0, dtype=np.float64), want - want0
    return float(np.abs(d - dw).max() / np.abs(dw).max() / U)


def solve_float32(f0, lr, sensor, ratio, iters, damp=0.0, return_d=False):
    """The device's arithmetic on the host (see the module's docstring); the taps are the float64 tables rounded to float32."""
    from tmdiff_amd import metrics
    f32, f64 = np.float32, np.float64
    f0, lr = np.asarray(f0, dtype=f32), np.asarray(lr, dtype=f32)
    taps = np.stack([metrics.mtf_kernel(g, ratio) for g in metrics.band_gains(sensor, f0.shape[1])]).astype(f32)
    hw = f0.shape[2:]
    dot = lambda a, b: (a.astype(f64) * b.astype(f64)).sum(axis=(2, 3), keepdims=True)
    coef = lambda num, den: np.divide(num, den, out=np.zeros_like(num), where=den != 0.0).astype(f32).astype(f64)
    fma = lambda a, x, y: (a * x.astype(f64) + y.astype(f64)).astype(f32)
    r = (lr.astype(f64) - fir_float32(f0, taps, ratio).astype(f64)).astype(f32)
    d = np.zeros_like(f0)
    if iters:
        p = adjoint_float32(r, taps, hw, ratio)
        gamma = pp = dot(p, p)
    for k in range(iters):
        q = fir_float32(p, taps, ratio)
        alpha = coef(gamma, dot(q, q) + f64(damp) * pp if damp else dot(q, q))
        d = (alpha * p.astype(f64)).astype(f32) if k == 0 else fma(alpha, p, d)
        r = fma(-alpha, q, r)
        if k + 1 < iters:
            s = adjoint_float32(r, taps, hw, ratio)
            if damp:
                s = fma(f64(f32(-damp)), d, s)
            new = dot(s, s)
            p = fma(coef(new, gamma), p, s)
            gamma, pp = new, dot(p, p)
    f = (f0.astype(f64) + d.astype(f64)).astype(f32) if iters else f0.copy()
    return (f, d) if return_d else f


def _noise_scene(sensor, bands, ratio):
    from tmdiff_amd import metrics
    hr = np.random.default_rng(48).random((1, bands, 48, 48))
    lr = metrics.mtf_degrade(hr, sensor, ratio)
    return lr, metrics.upsample_poly23(lr, ratio)


def _residual(f, lr, sensor, ratio):
    from tmdiff_amd import metrics
    return float(np.sqrt(np.mean((metrics.mtf_degrade(f, sensor, ratio) - lr) ** 2)))


@pytest.mark.parametrize("sensor,bands,ratio", [("QB", 4, 4), ("WV3", 8, 2)])
def test_conditions_measured_when_it_was_proposed(sensor, bands, ratio):
    from tmdiff_amd import metrics
    from tmdiff_amd.tiling import consistency_refine, consistency_solve
    lr, start = _noise_scene(sensor, bands, ratio)
    f, info = metrics.consistency_solve(start, lr, sensor, ratio, iters=8, return_info=True)
    assert info.shape == (1, bands, 9)
    assert (info[..., 1:] < info[..., :-1]).all()                      # strictly decreasing, every plane
    r0 = _residual(start, lr, sensor, ratio)
    cg, lw = _residual(f, lr, sensor, ratio) / r0, _residual(consistency_refine(start, lr, sensor, ratio, iters=8), lr, sensor, ratio) / r0
    print(f"{sensor} x{ratio}: residual ratio after 8 iterations: CGLS {cg:.4f}, Landweber {lw:.4f}; trace "
          + " ".join(f"{v:.4f}" for v in np.sqrt(info.sum(1)[0] / info.sum(1)[0, 0])))
    assert cg < 0.1
    assert cg < lw / 3.0
    # the recurrence's residual is the true one
    true = ((lr - metrics.mtf_degrade(f, sensor, ratio)) ** 2).sum(axis=(2, 3))
    assert np.abs(info[..., -1] - true).max() <= 1e-12 * true.max()
    assert np.array_equal(consistency_solve(start, lr, sensor, ratio, iters=8), f)          # tiling: the definition on host data
    t = consistency_solve(torch.from_numpy(start), torch.from_numpy(lr), sensor, ratio, iters=2)
    assert torch.is_tensor(t) and t.dtype == torch.float64 and np.array_equal(t.numpy(), metrics.consistency_solve(start, lr, sensor, ratio, 2))


def test_damped_solve_settles():
    from tmdiff_amd import metrics
    for sensor, bands, ratio, lo, hi in (("QB", 4, 4, 0.05, 0.2), ("WV3", 8, 2, 0.01, 0.05)):
        lr, start = _noise_scene(sensor, bands, ratio)
        r0 = _residual(start, lr, sensor, ratio)
        a = _residual(metrics.consistency_solve(start, lr, sensor, ratio, iters=32, damp=1e-3), lr, sensor, ratio) / r0
        b = _residual(metrics.consistency_solve(start, lr, sensor, ratio, iters=48, damp=1e-3), lr, sensor, ratio) / r0
        print(f"{sensor} x{ratio}, damp 1e-3: residual ratio {a:.4f} after 32 iterations, {b:.4f} after 48")
        assert lo < b < hi and abs(a - b) < 0.02 * b


def test_against_the_dense_operator():
    """24 x 24 at x4: 36 equations per plane.  damp = 0 -> f0 + pinv(A)(lr - A f0); damp > 0 -> the normal equations."""
    from tmdiff_amd import metrics
    rng = np.random.default_rng(24)
    gains, ratio, n = (0.3, 0.2), 4, 24
    dense = []
    for g in gains:
        taps = metrics.mtf_kernel(g, ratio)
        dense.append(np.stack([metrics.fir_decimate(e.reshape(n, n), taps, ratio).ravel() for e in np.eye(n * n)], axis=1))
    assert dense[0].shape == (36, n * n)
    f0 = rng.random((1, 2, n, n))
    lr = metrics.mtf_degrade(rng.random((1, 2, n, n)), gains, ratio) + 0.01 * rng.standard_normal((1, 2, 6, 6))
    for key, damp, iters in (("pinv", 0.0, 60), ("damped", 1e-3, 60)):
        f = metrics.consistency_solve(f0, lr, gains, ratio, iters=iters, damp=damp)
        worst = 0.0
        for c, a in enumerate(dense):
            res = lr[0, c].ravel() - a @ f0[0, c].ravel()
            d = np.linalg.pinv(a) @ res if damp == 0.0 else np.linalg.solve(a.T @ a + damp * np.eye(n * n), a.T @ res)
            worst = max(worst, float(np.abs(f[0, c].ravel() - f0[0, c].ravel() - d).max() / np.abs(d).max()))
        print(f"dense check, {key}: max |d - closed form| / max |closed form| = {worst:.3e}")
        assert worst <= 10.0 * DENSE_GAP[key]


def test_guards_and_arguments():
    from tmdiff_amd import metrics
    from tmdiff_amd.tiling import consistency_solve
    lr, start = _noise_scene("QB", 4, 4)
    lr = lr.copy()
    lr[0, 1] = metrics.mtf_degrade(start, "QB", 4)[0, 1]               # band 1 is consistent already
    f, info = metrics.consistency_solve(start, lr, "QB", 4, iters=5, return_info=True)
    assert np.isfinite(f).all() and np.isfinite(info).all()
    assert np.array_equal(f[0, 1], start[0, 1]) and not info[0, 1].any()
    alone = metrics.consistency_solve(start[:, 2:3], lr[:, 2:3], (metrics.band_gains("QB", 4)[2],), 4, iters=5)
    assert np.array_equal(f[0, 2], alone[0, 0])
    same, info0 = metrics.consistency_solve(start, lr, "QB", 4, iters=0, return_info=True)
    assert np.array_equal(same, start) and same is not start and info0.shape == (1, 4, 1)
    assert np.array_equal(consistency_solve(start, lr, "QB", 4, iters=0), start)
    for fn in (metrics.consistency_solve, consistency_solve):
        for bad in (dict(iters=-1), dict(iters=1.5), dict(damp=-1e-3), dict(damp=float("nan"))):
            with pytest.raises(ValueError):
                fn(start, lr, "QB", 4, **bad)
        with pytest.raises(ValueError):
            fn(start, lr[..., :-1], "QB", 4)                            # not the degradation's extent
        with pytest.raises(ValueError):
            fn(start[:, :3], lr[:, :3], "QB", 4)                        # 4 gains, 3 bands


def test_option_dictionaries():
    from tmdiff_amd import metrics
    from tmdiff_amd.diffusion_general import GeneralDiffusion
    from tmdiff_amd.tiling import bdsd_fuse, classical_fuse, cs_fuse, fuse_scene
    lr, pan = torch.rand(1, 4, 12, 12, dtype=torch.float64), torch.rand(1, 1, 48, 48, dtype=torch.float64)
    # "method" defaults to "landweber": today's path bit for bit
    plain = classical_fuse(lr, pan, "QB", consistency={"iters": 2, "relax": 0.9})
    assert torch.equal(plain, classical_fuse(lr, pan, "QB", consistency={"method": "landweber", "iters": 2, "relax": 0.9}))
    cg = classical_fuse(lr, pan, "QB", consistency={"method": "cg", "iters": 3, "damp": 1e-4})
    base = classical_fuse(lr, pan, "QB")
    assert np.array_equal(cg.numpy(), metrics.consistency_solve(base.numpy(), lr.numpy(), "QB", 4, 3, 1e-4))
    res = lambda f: float((metrics.mtf_degrade(f.numpy(), "QB", 4) - lr.numpy()).std())
    assert res(cg) < res(plain) < res(base)
    for fuse in (classical_fuse, lambda *a, **k: cs_fuse(*a, method="gs", **k), bdsd_fuse):
        assert torch.is_tensor(fuse(lr, pan, "QB", consistency={"method": "cg", "iters": 1}))
        for bad in ({"method": "cg", "relax": 1.0}, {"method": "landweber", "damp": 0.1}, {"damp": 0.1}, {"method": "sor"},
                    {"method": "cg", "in_loop": True}, {"method": "cg", "iters": -1}, {"method": "cg", "damp": -1.0}, {"steps": 2}):
            with pytest.raises(ValueError):
                fuse(lr, pan, "QB", consistency=bad)
    zl, zp = torch.zeros(1, 4, 12, 12), torch.zeros(1, 1, 48, 48)
    for bad in ({"method": "cg", "relax": 1.0}, {"damp": 0.1}, {"in_loop": True}, {"method": "cg", "iters_post": 2}):
        with pytest.raises(ValueError):
            fuse_scene(None, zl, zp, "QB", sensor="QB", consistency=bad)
    with pytest.raises(ValueError, match="fused tile mode"):           # the independent-tile mode
        fuse_scene(None, zl, zp, "QB", sensor="QB", consistency={"method": "cg", "in_loop": True})
    with pytest.raises(ValueError, match="sensor"):
        fuse_scene(None, zl, zp, "QB", consistency={"method": "cg"})
    with pytest.raises(ValueError, match="dpmsolver"):                 # the DDPM loop has no data prediction to project
        GeneralDiffusion.sample(None, {}, "QB", method="ddpm", consistency={"lr_ms": zl, "sensor": "QB"})
    x_in = {"MS": torch.zeros(1, 4, 48, 48)}
    for bad in ({"sensor": "QB"}, {"lr_ms": zl}, {"lr_ms": zl, "sensor": "QB", "relax": 1.0}, {"lr_ms": zl[..., :-1], "sensor": "QB"},
                {"lr_ms": zl, "sensor": "QB", "iters": -1}, {"lr_ms": zl, "sensor": "QB", "ratio": 3}, "cg"):
        with pytest.raises(ValueError):
            GeneralDiffusion._consistency_projection(x_in, bad)


def test_c_entry_points_check_their_arguments():
    """Nothing is launched: the pointers are never touched."""
    from tmdiff_amd._lib import lib
    parts = lib.tmdiff_plane_dots_partials
    assert [parts(n) for n in (0, 1, 4096, 4097, 1024 * 1024, 1024 * 1024 + 1, 2 ** 31 - 1)] == [1, 1, 1, 2, 256, 205, 256]
    assert parts(200 * 136) == 7 and parts(-1) == 0
    assert lib.tmdiff_plane_dots(None, None, 2 ** 20, None, None, None, 0, None, 2 ** 12, None) == -2
    assert "plane_dots: " in lib.tmdiff_last_error_string().decode()
    assert lib.tmdiff_plane_dots(None, None, 16, None, None, None, 0, None, 0, None) == 0          # no plane
    assert lib.tmdiff_plane_dots(None, None, 16, None, None, None, 0, None, 2, None) == -1         # null tensors
    assert lib.tmdiff_plane_totals(None, None, 2, 257, 1, 0, None) == -2
    assert lib.tmdiff_plane_totals(None, None, 2, 3, 1, 0, None) == -1
    assert lib.tmdiff_cg_step(None, None, None, None, None, None, None, -1.0, None, 2, 16, 4, 1, None) == -2
    assert "damp" in lib.tmdiff_last_error_string().decode()
    assert lib.tmdiff_cg_step(None, None, None, None, None, None, None, 0.0, None, 2, 16, 4, 1, None) == -1
    assert lib.tmdiff_cg_direction(None, None, None, None, None, -1, 16, None) == -2
    assert lib.tmdiff_cg_direction(None, None, None, None, None, 2, 16, None) == -1


def test_float32_restatement():
    """Measures the working bound of the GPU test: the device's arithmetic in float32 against the definition."""
    from tmdiff_amd import metrics
    got = {}
    for key in list(CG_CASES) + ["damp"]:
        name = "QB x4 48" if key == "damp" else key
        damp = CG_DAMP if key == "damp" else 0.0
        sensor, ratio, _ = CG_CASES[name]
        f0, lr = cg_scene(name)
        want = metrics.consistency_solve(f0, lr, sensor, ratio, CG_ITERS, damp)
        f, d = solve_float32(f0, lr, sensor, ratio, CG_ITERS, damp, return_d=True)
        dw = want - f0.astype(np.float64)
        got[key] = float(np.abs(d - dw).max() / np.abs(dw).max() / U)
    print("solve_float32, worst |d32 - d64| / max |d64| in u: " + "  ".join(f"{k}: {v:.3f}" for k, v in got.items()))
    for key, v in got.items():
        assert v <= CG_RESTATEMENT_U[key] + 5e-4, (key, v)
