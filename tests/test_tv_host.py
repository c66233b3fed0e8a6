"""CPU-only tests of TV pansharpening: the float64 host definitions ``metrics.tv_grad`` / ``tv_grad_adjoint`` / ``tv_norm`` /
``tv_pd_step`` / ``tv_step_sizes`` / ``tv_pansharpen`` and ``tiling.tv_fuse`` on host data.

The definitions are held to independent statements: the transpose identity with the masked column and row filled, closed-form
values of the vector total variation, the Landweber iteration the scheme reduces to without the coupling (lam = 0, gamma = 0, one
band: ``tiling.consistency_refine``), and, on a 2-band 16 x 24 scene, the minimum that L-BFGS-B finds on the cost with
sqrt(. + 1e-10) in place of the norm.

The file also holds what the GPU test (tests/test_gpu_tv.py) is measured against: its cases (``TV_CASES``) and a float32
restatement of the device's loop (``solve_float32``): float32 storage, A and A^T in the kernels' summation orders
(``fir_float32``, ``adjoint_float32``), the step of the adjoint as the kernel applies it (alpha rounded to float32, the product
rounded, then one addition), and ``metrics.tv_pd_step(storage=np.float32)`` for the coupled part.  The fp32 and fp64 iterations
drift apart with the iteration count and no bound on that drift can be derived, so the restatement's distance from the float64
run is measured here, as max |x32 - x64| / max |x64 - x0| in units of u = 2^-24 (``TV_RESTATEMENT_U``), and the device is held
to 4 times the figure, rounded up -- the margin the CG tests give a device that sums in another order."""
import ctypes

import numpy as np
import pytest
import torch

from test_mtf_adjoint_host import adjoint_float32
from test_mtf_host import U, fir_float32

# name -> sensor or band gains, ratio, (B, C, H, W) at the full scale, weights ([C + 1] or per image), lam, gamma
TV_CASES = {
    "2 bands x4 16x24": dict(gains=(0.3, 0.25), ratio=4, shape=(1, 2, 16, 24), weights=(0.6, 0.4, 0.02), lam=1e-3, gamma=1.0),
    # three tiles down and three across, ragged on both axes
    "QB x4 40x72": dict(gains="QB", ratio=4, shape=(1, 4, 40, 72), weights=(0.2, 0.3, 0.3, 0.2, -0.01), lam=2e-3, gamma=0.5),
    # a batch with weights per image, ratio 2, a tile edge one pixel inside the image on both axes
    "3 bands x2 34x66": dict(gains=(0.34, 0.29, 0.22), ratio=2, shape=(2, 3, 34, 66),
                             weights=((0.5, 0.3, 0.2, 0.01), (0.2, 0.2, 0.6, -0.02)), lam=1e-3, gamma=1.0),
}
TV_ITERS = 30
# worst |x32 - x64| / max |x64 - x0| of solve_float32 against the float64 run in u, as test_float32_restatement measures it (and
# holds it to)
TV_RESTATEMENT_U = {"2 bands x4 16x24": 27.404, "QB x4 40x72": 34.012, "3 bands x2 34x66": 88.432}
# the cap on mean |x - truth| after 400 iterations over the start's in test_convergence_on_the_small_scene: a quarter; measured
# there: 0.151 (0.0474 -> 0.0071), beside J 0.65227 -> 0.017584642 against 0.017584662 at the L-BFGS-B minimiser of the smoothed
# cost, a gap of -3e-8 of J(start) - J_ref (the iteration ends below the smoothed minimiser)
MAE_CAP = 0.25


def tv_scene(name):
    """(lr, pan, x0, truth) of a case: a piecewise-constant truth with a ramp and a little noise, pan = the case's weighted sum of
    its bands plus the offset, lr = A(truth), all float32; x0 = the float64 ``upsample_poly23(lr)`` rounded to float32."""
    from tmdiff_amd import metrics
    case = TV_CASES[name]
    b, c, h, w = case["shape"]
    rng = np.random.default_rng(1000 * h + w)
    yy, xx = np.mgrid[:h, :w]
    truth = np.empty(case["shape"])
    for i in range(b):
        for k in range(c):
            blocks = rng.random((h // 8 + 1, w // 8 + 1))[yy // 8, xx // 8]
            truth[i, k] = 0.15 + 0.5 * blocks + 0.2 * (xx + (k + 1) * yy) / (w + (k + 1) * h) + 0.02 * rng.random((h, w))
    wt = metrics.tv_weights(case["weights"], b, c)
    pan = (wt[:, :c, None, None] * truth).sum(axis=1, keepdims=True) + wt[:, c, None, None, None]
    lr = metrics.mtf_degrade(truth, case["gains"], case["ratio"]).astype(np.float32)
    x0 = metrics.upsample_poly23(lr, case["ratio"]).astype(np.float32)
    return lr, pan.astype(np.float32), x0, truth


def tv_tol_u(name):
    """The GPU test's tolerance in u: 4 x the restatement's figure, rounded up."""
    return float(np.ceil(4.0 * TV_RESTATEMENT_U[name]))


def tv_error_u(x, want, x0):
    """max |x - want| / max |want - x0| in u, the differences formed in float64."""
    x, want, x0 = (np.asarray(a, dtype=np.float64) for a in (x, want, x0))
    return float(np.abs(x - want).max() / np.abs(want - x0).max() / U)


def solve_float32(name, iters):
    """The device's loop on the host (see the module's docstring), started from the case's x0."""
    from tmdiff_amd import metrics
    case = TV_CASES[name]
    f32, f64 = np.float32, np.float64
    lr, pan, x, _ = tv_scene(name)
    b, c, h, w = case["shape"]
    ratio = case["ratio"]
    gains = metrics.band_gains(case["gains"], c)
    taps = np.stack([metrics.mtf_kernel(g, ratio) for g in gains]).astype(f32)
    wt = metrics.tv_weights(case["weights"], b, c)
    tau, sigma = metrics.tv_step_sizes(gains, ratio, wt, case["gamma"])
    alpha = f64(f32(-tau))
    ph, pv = np.zeros_like(x), np.zeros_like(x)
    for _ in range(iters):
        r = (fir_float32(x, taps, ratio).astype(f64) - lr.astype(f64)).astype(f32)
        step = (alpha * adjoint_float32(r, taps, (h, w), ratio).astype(f64)).astype(f32)
        u = (x.astype(f64) + step.astype(f64)).astype(f32)
        x, ph, pv = metrics.tv_pd_step(u, x, ph, pv, pan, wt, tau, sigma, case["lam"], case["gamma"], storage=f32)
    return x


def definition(name, iters=TV_ITERS):
    """The float64 definition's result from the case's (float32) inputs and start."""
    from tmdiff_amd import metrics
    case = TV_CASES[name]
    lr, pan, x0, _ = tv_scene(name)
    return metrics.tv_pansharpen(lr, pan, case["gains"], case["ratio"], iters, case["lam"], case["gamma"], case["weights"], x0=x0)


# ---- the differences and the norm -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 1, 1, 4)])
def test_adjoint_identity(shape):
    from tmdiff_amd import metrics
    rng = np.random.default_rng(sum(shape))
    x, ph, pv = rng.standard_normal(shape), rng.standard_normal(shape), rng.standard_normal(shape)
    assert ph[..., :, -1].all() and pv[..., -1, :].all()                              # the masked column and row hold something
    dh, dv = metrics.tv_grad(x)
    assert not dh[..., :, -1].any() and not dv[..., -1, :].any()
    lhs, rhs = (dh * ph + dv * pv).sum(), (x * metrics.tv_grad_adjoint(ph, pv)).sum()
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), (np.abs(dh * ph) + np.abs(dv * pv)).sum())
    other_h, other_v = ph.copy(), pv.copy()
    other_h[..., :, -1], other_v[..., -1, :] = np.nan, np.inf                         # never read, whatever they hold
    assert np.array_equal(metrics.tv_grad_adjoint(other_h, other_v), metrics.tv_grad_adjoint(ph, pv))


def test_tv_norm_values():
    from tmdiff_amd import metrics
    assert np.array_equal(metrics.tv_norm(np.full((2, 3, 6, 5), 0.7)), np.zeros(2))
    h, w, c, a = 6, 9, 4, 0.25
    step = np.zeros((1, c, h, w))
    step[..., 5:] = a                                                                 # a vertical edge of height a in every band
    assert abs(metrics.tv_norm(step)[0] - h * a * np.sqrt(c)) <= 1e-14
    rng = np.random.default_rng(3)
    row, col = rng.random((2, 3, 1, 8)), rng.random((1, 2, 7, 1))
    assert np.allclose(metrics.tv_norm(row), np.sqrt((np.diff(row, axis=3) ** 2).sum(axis=1)).sum(axis=(1, 2)), rtol=1e-14, atol=0)
    assert np.allclose(metrics.tv_norm(col), np.sqrt((np.diff(col, axis=2) ** 2).sum(axis=1)).sum(axis=(1, 2)), rtol=1e-14, atol=0)
    assert np.array_equal(metrics.tv_norm(np.ones((1, 1, 1, 1))), np.zeros(1))


def test_step_sizes():
    from tmdiff_amd import metrics
    gains, wt = (0.3, 0.25), np.array([[0.6, 0.4, 0.02], [0.1, 0.9, 5.0]])
    tau, sigma = metrics.tv_step_sizes(gains, 4, wt, 2.0)
    lf = 1.01 * (max(metrics.mtf_opnorm2(g, 4) for g in gains) + 2.0 * 0.82)           # 0.1^2 + 0.9^2: the offset does not count
    assert abs(tau * lf - 1.0) <= 1e-15 and abs(sigma - lf / 16.0) <= 1e-15 * sigma
    assert 1.0 / tau - 8.0 * sigma >= lf / 2.0 * (1.0 - 1e-15)
    with pytest.raises(ValueError):
        metrics.tv_step_sizes(gains, 4, wt[:, :2], 1.0)


# ---- lam = 0 ------------------------------------------------------------------------------------------------------------------------
def test_without_the_regulariser():
    from tmdiff_amd import metrics
    from tmdiff_amd.tiling import consistency_refine
    name = "2 bands x4 16x24"
    case = TV_CASES[name]
    lr, pan, x0, _ = tv_scene(name)
    wt = metrics.tv_weights(case["weights"], 1, 2)
    tau, sigma = metrics.tv_step_sizes(case["gains"], 4, wt, 1.0)
    zero = np.zeros(x0.shape)
    x1, ph, pv = metrics.tv_pd_step(x0, x0, zero, zero, pan, wt, tau, sigma, 0.0, 1.0)
    assert not ph.any() and not pv.any() and not np.array_equal(x1, x0)                # p stays 0
    start = metrics.tv_objective(x0, lr, pan, case["gains"], 4, 0.0, 1.0, wt)
    _, info = metrics.tv_pansharpen(lr, pan, case["gains"], 4, 20, 0.0, 1.0, wt, x0=x0, return_info=True)
    trace = np.concatenate([start[:, None], info], axis=1)
    assert (trace[:, 1:] <= trace[:, :-1]).all() and trace[0, -1] < 0.5 * trace[0, 0]  # f does not increase
    # one band, no PAN term: the Landweber iteration of consistency_refine with relax = tau ||A||^2
    gain = (0.3,)
    tau1, _ = metrics.tv_step_sizes(gain, 4, np.array([1.0, 0.0]), 0.0)
    got = metrics.tv_pansharpen(lr[:, :1], pan, gain, 4, 5, 0.0, 0.0, x0=x0[:, :1])
    want = consistency_refine(x0[:, :1].astype(np.float64), lr[:, :1], gain, 4, iters=5, relax=tau1 * metrics.mtf_opnorm2(0.3, 4))
    assert np.abs(got - want).max() <= 1e-12


# ---- convergence ------------------------------------------------------------------------------------------------------------------
def _dense_degradation(gains, ratio, h, w):
    """A as one dense matrix per band, [C, h' w', h w]: the definition applied to the unit images in one call."""
    from tmdiff_amd import metrics
    units = np.eye(h * w).reshape(h * w, h, w)
    return np.stack([metrics.fir_decimate(units, metrics.mtf_kernel(g, ratio), ratio).reshape(h * w, -1).T for g in gains])


def test_convergence_on_the_small_scene():
    """J after 400 iterations exceeds J_ref, the cost at the L-BFGS-B minimiser of the 1e-10-smoothed cost, by at most 0.1 % of
    J(start) - J_ref; the mean absolute error to the truth falls below a quarter of the start's (cap: see the assertion)."""
    from scipy.optimize import minimize
    from tmdiff_amd import metrics
    name = "2 bands x4 16x24"
    case = TV_CASES[name]
    lr, pan, x0, truth = tv_scene(name)
    lr, pan, x0 = (a.astype(np.float64) for a in (lr, pan, x0))
    (b, c, h, w), ratio, lam, gamma = case["shape"], case["ratio"], case["lam"], case["gamma"]
    wt = metrics.tv_weights(case["weights"], b, c)
    cost = lambda x: float(metrics.tv_objective(x, lr, pan, case["gains"], ratio, lam, gamma, wt)[0])
    a = _dense_degradation(case["gains"], ratio, h, w)
    assert np.abs(np.einsum("cij,cj->ci", a, x0[0].reshape(c, -1)) - metrics.mtf_degrade(x0, case["gains"], ratio)[0].reshape(c, -1)).max() <= 1e-13

    def smoothed(v):
        x = v.reshape(1, c, h, w)
        r = np.einsum("cij,cj->ci", a, x[0].reshape(c, -1)) - lr[0].reshape(c, -1)
        s = (wt[:, :c, None, None] * x).sum(axis=1, keepdims=True) + wt[0, c] - pan
        dh, dv = metrics.tv_grad(x)
        n = np.sqrt((dh * dh + dv * dv).sum(axis=1, keepdims=True) + 1e-10)
        val = 0.5 * (r * r).sum() + 0.5 * gamma * (s * s).sum() + lam * n.sum()
        grad = np.einsum("cij,ci->cj", a, r).reshape(x.shape) + gamma * wt[:, :c, None, None] * s + lam * metrics.tv_grad_adjoint(dh / n, dv / n)
        return val, grad.ravel()
    best = minimize(smoothed, x0.ravel(), jac=True, method="L-BFGS-B", options={"maxiter": 20000, "maxfun": 40000, "ftol": 1e-15, "gtol": 1e-9})
    j_ref, j0 = cost(best.x.reshape(x0.shape)), cost(x0)
    x = metrics.tv_pansharpen(lr, pan, case["gains"], ratio, 400, lam, gamma, wt, x0=x0)
    j400 = cost(x)
    gap = (j400 - j_ref) / (j0 - j_ref)
    mae0, mae = np.abs(x0 - truth).mean(), np.abs(x - truth).mean()
    print(f"TV on {name}: J start {j0:.6g}, after 400 iterations {j400:.8g}, L-BFGS-B {j_ref:.8g} ({best.nit} iterations): "
          f"gap {100 * gap:.4f} % of J(start) - J_ref; mean |x - truth| {mae0:.4f} -> {mae:.4f} ({mae / mae0:.3f} of the start)")
    assert j_ref < j0 and gap <= 1e-3
    assert mae <= MAE_CAP * mae0


# ---- the float32 restatement ----------------------------------------------------------------------------------------------------------
def test_float32_restatement():
    """Measures the working bound of the GPU test: the device's loop in float32 against the float64 run from the same start."""
    got = {}
    for name in TV_CASES:
        _, _, x0, _ = tv_scene(name)
        got[name] = tv_error_u(solve_float32(name, TV_ITERS), definition(name), x0)
    print("solve_float32, worst |x32 - x64| / max |x64 - x0| in u: " + "  ".join(f"{k}: {v:.3f}" for k, v in got.items()))
    for name, v in got.items():
        assert v <= TV_RESTATEMENT_U[name] + 5e-4, (name, v)


def test_storage_rounds_once_per_iteration():
    from tmdiff_amd import metrics
    name = "2 bands x4 16x24"
    case = TV_CASES[name]
    lr, pan, x0, _ = tv_scene(name)
    x = metrics.tv_pansharpen(lr, pan, case["gains"], 4, 3, case["lam"], case["gamma"], case["weights"], x0=x0, storage=np.float32)
    assert x.dtype == np.float32 and tv_error_u(x, definition(name, 3), x0) < 64.0
    assert np.array_equal(metrics.tv_pansharpen(lr, pan, case["gains"], 4, 0, x0=x0), x0)          # iters = 0 returns the start
    assert np.array_equal(metrics.tv_pansharpen(lr, pan, case["gains"], 4, 0), metrics.upsample_poly23(lr, 4))


# ---- arguments and users ------------------------------------------------------------------------------------------------------------
def test_arguments():
    from tmdiff_amd import metrics
    from tmdiff_amd.tiling import tv_fuse
    lr, pan, x0, _ = tv_scene("2 bands x4 16x24")
    zero = np.zeros_like(x0)
    for call in (lambda: metrics.tv_pansharpen(lr, pan, (0.3, 0.25), 4, -1),
                 lambda: metrics.tv_pansharpen(lr, pan, (0.3, 0.25), 4, 2, lam=-1.0),
                 lambda: metrics.tv_pansharpen(lr, pan, (0.3, 0.25), 3),
                 lambda: metrics.tv_pansharpen(lr, pan[..., :-1], (0.3, 0.25), 4),
                 lambda: metrics.tv_pansharpen(lr, pan, (0.3, 0.25), 4, 2, weights=(1.0, 2.0)),
                 lambda: metrics.tv_pansharpen(lr, pan, (0.3, 0.25), 4, 2, x0=x0[..., :-1]),
                 lambda: metrics.tv_pd_step(x0, x0, zero, zero[..., :-1], pan, None, 1.0, 1.0, 1.0, 1.0),
                 lambda: metrics.tv_pd_step(x0, x0, zero, zero, pan, None, 0.0, 1.0, 1.0, 1.0),
                 lambda: metrics.tv_norm(np.zeros((1, 17, 4, 4))),
                 lambda: tv_fuse(lr, pan, None),
                 lambda: tv_fuse(lr, pan, (0.3, 0.25), weights="gsa"),
                 lambda: tv_fuse(lr, pan, (0.3, 0.25), score=True)):
        with pytest.raises(ValueError):
            call()


def test_tv_fuse_on_host_data():
    from tmdiff_amd import metrics
    from tmdiff_amd.tiling import tv_fuse, tv_regress_weights
    lr, pan, x0, _ = tv_scene("2 bands x4 16x24")
    gains = (0.3, 0.25)
    got = tv_fuse(torch.from_numpy(lr), torch.from_numpy(pan), (gains, 0.15), iters=3)
    assert torch.is_tensor(got) and got.dtype == torch.float64
    assert np.array_equal(got.numpy(), metrics.tv_pansharpen(lr, pan, gains, 4, 3))
    wt = tv_regress_weights(lr, pan, (gains, 0.15), 4)
    low = metrics.mtf_degrade(pan.astype(np.float64), 0.15, 4)
    design = np.concatenate([lr[0].astype(np.float64).reshape(2, -1), np.ones((1, lr[0][0].size))])
    assert wt.shape == (1, 3) and np.abs(design @ design.T @ wt[0] - design @ low.ravel()).max() <= 1e-10      # the normal equations
    assert np.array_equal(tv_fuse(lr, pan, (gains, 0.15), iters=2, weights="regress"), tv_fuse(lr, pan, (gains, 0.15), iters=2, weights=wt))


def test_c_entry_points_check_their_arguments():
    from tmdiff_amd._lib import lib
    assert lib.tmdiff_tv_supported(1, 16, 1, 1) == 1 and lib.tmdiff_tv_supported(1, 17, 8, 8) == 0
    assert lib.tmdiff_tv_supported(2, 4, 0, 8) == 0 and lib.tmdiff_tv_supported(1, 16, 16384, 8192) == 0     # 2^31 elements
    assert lib.tmdiff_tv_norm_workspace_bytes(2, 3, 17, 33) == 2 * 4 * 8 and lib.tmdiff_tv_norm_workspace_bytes(1, 0, 4, 4) == 0
    scal = [ctypes.c_double(v) for v in (1.0, 1.0, 1.0, 1.0)]
    assert lib.tmdiff_tv_pd_step(*[None] * 6, *scal, *[None] * 3, 1, 17, 4, 4, None) != 0                     # C = 17
    assert lib.tmdiff_tv_pd_step(*[None] * 6, *scal, *[None] * 3, 1, 2, 4, 4, None) == -1                      # null tensors
    assert lib.tmdiff_tv_pd_step(*[None] * 6, ctypes.c_double(0.0), *scal[1:], *[None] * 3, 1, 2, 4, 4, None) == -1   # tau = 0
    assert lib.tmdiff_tv_pd_step(*[None] * 6, *scal, *[None] * 3, 0, 2, 4, 4, None) == 0                       # an empty batch
    fake = [0x10000 * (i + 1) for i in range(9)]                                                                 # never dereferenced
    assert lib.tmdiff_tv_pd_step(*fake[:6], *scal, fake[0], *fake[7:], 1, 2, 4, 4, None) == -1                 # x' on u: refused
    assert lib.tmdiff_tv_pd_step(*fake[:6], *scal, fake[6], fake[7], fake[7], 1, 2, 4, 4, None) == -1          # ph' on pv'
    assert lib.tmdiff_tv_norm(None, 1, 2, 4, 4, None, None, 0, None) == -1
