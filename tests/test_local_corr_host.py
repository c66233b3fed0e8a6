"""The local PAN-correlation index and loss, float64 host definitions (tmdiff_amd.metrics.local_corr / local_corr_loss / d_rho)
and tiling.structure_refine on the host, held to independent statements; no GPU."""
import os
import re

import numpy as np
import pytest
import torch

from local_corr_refs import U, random_pair, smooth_scene, triple_loop
from tmdiff_amd import metrics, tiling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("tmdiff_local_corr_loss_supported", "tmdiff_local_corr_loss_workspace_bytes", "tmdiff_local_corr_loss")


@pytest.mark.parametrize("win", [2, 3, 4, 7, 8])
def test_local_corr_is_the_triple_loop(win):
    """Two statements of the same two-pass sums in different orders: 1e-13 absolute on |rho| <= 1 (a window's sums carry at most
    about n u = 64 * 2^-53 relative error each)."""
    x, pan = random_pair(1, (2, 3, 11, 13))
    got = metrics.local_corr(x, pan, win)
    assert got.dtype == np.float64 and got.shape == (2, 3, 11 - win + 1, 13 - win + 1)
    assert np.abs(got - triple_loop(x.numpy(), pan.numpy(), win)).max() <= 1e-13
    assert np.abs(got).max() <= 1.0 + 1e-15


@pytest.mark.parametrize("win", [2, 3, 4, 7, 8])
def test_constant_windows_give_exact_zeros(win):
    x, pan = random_pair(2, (2, 3, 11, 13))
    flat_band = x.clone()
    flat_band[:, 1] = 0.3                                     # (0.3 is not a dyadic number: n v / n == v is what makes this exact)
    rho = metrics.local_corr(flat_band, pan, win)
    assert np.all(rho[:, 1] == 0.0) and np.all(rho[:, 0] != 0.0)
    flat_pan = torch.full_like(pan, 0.7)
    assert np.all(metrics.local_corr(x, flat_pan, win) == 0.0)
    # a patch that is constant only inside some windows: exactly the windows that lie inside it are zero
    patch = x.clone()
    patch[0, 2, 1:1 + win + 1, 2:2 + win + 2] = 0.1
    rho = metrics.local_corr(patch, pan, win)
    inside = np.zeros(rho.shape[2:], dtype=bool)
    inside[1:3, 2:5] = True
    assert np.all(rho[0, 2][inside] == 0.0) and np.all(rho[0, 2][~inside] != 0.0)
    loss, mean_rho, grad = metrics.local_corr_loss(flat_band, pan, win)
    assert np.all(grad[:, 1] == 0.0) and np.isfinite(grad).all() and np.isfinite(loss)


@pytest.mark.parametrize("win", [2, 3, 4, 8])
def test_affine_images_of_the_pan_score_zero_and_two(win):
    _, pan = random_pair(3, (2, 3, 11, 13))
    p = pan.double()
    up = torch.cat([0.5 * p + 0.25, 2.0 * p - 0.5, 0.125 * p], 1)
    down = torch.cat([-0.5 * p + 0.75, -2.0 * p + 1.5, -0.125 * p + 1.0], 1)
    assert np.abs(metrics.d_rho(up, p, win)).max() < 1e-12
    assert np.abs(metrics.d_rho(down, p, win) - 2.0).max() < 1e-12
    loss, mean_rho, _ = metrics.local_corr_loss(up, p, win)
    assert abs(loss - float(metrics.d_rho(up, p, win).mean())) < 1e-15 and abs(mean_rho - 1.0) < 1e-12


@pytest.mark.parametrize("win", [2, 4, 8])
def test_rho_is_invariant_to_positive_affine_changes_exactly_on_the_grid(win):
    """Inputs on the grid of multiples of 2^-10; x -> 4 x + 3 and pan -> 0.5 pan + 1 stay on a dyadic grid where every sum is
    exact, the centred values scale by exact powers of two, and so do S_xx S_pp and S_xp: rho is the same bits."""
    from local_corr_refs import grid_pair
    x, pan = grid_pair(4, (2, 3, 11, 13))
    x, pan = x.double(), pan.double()
    base = metrics.local_corr(x, pan, win)
    assert np.array_equal(metrics.local_corr(4.0 * x + 3.0, pan, win), base)
    assert np.array_equal(metrics.local_corr(x, 0.5 * pan + 1.0, win), base)
    assert np.array_equal(metrics.local_corr(2.0 * x + 0.25, 8.0 * pan + 2.0, win), base)


@pytest.mark.parametrize("rho_max", [None, 0.5], ids=["rho_max-none", "rho_max-0.5"])
@pytest.mark.parametrize("win", [3, 4])
def test_closed_form_gradient_against_central_differences(win, rho_max):
    """g_k against (L(x + h e_k) - L(x - h e_k)) / 2h with h = 5e-7 on [2, 3, 11, 13], every element.

    The bound, from the step.  Along e_k a window's rho is f(t) = a(t) / r(t) with a linear, |a'| <= 1, |a| <= r, and
    r = sqrt(S_xx), |r'| <= 1, |r''| <= 1 / r, |r'''| <= 3 / r^2, which gives |f'''| <= 24 / r^3.  An element lies in at most n =
    win^2 of the N windows, so the truncation error of the central difference is at most (h^2 / 6)(n / N) 24 / r_min^3 =
    4 h^2 n / (N r_min^3), r_min the least sqrt(S_xx) of the input (asserted to be far above h).  The two loss values each carry
    a rounding error of at most (2 n + 10) u times the largest hinge, 2 (two-pass sums of n terms, the square root, the
    divisions and the mean), so the quotient adds (2 n + 10) 2 u / h.  No fitted constant.
    The step keeps every window on its side of the kink: |d rho / d x_k| <= 2 / r_min, and the test asserts that no window lies
    within 1e-6 of rho_max and that the nearest one is further away than 2 h / r_min (seed 1 holds both: r_min = 0.40, so a step
    moves rho by at most 2.5e-6, and the nearest window is 4e-4 from 0.5 and 0.05 from 1)."""
    h = 5e-7
    x, pan = random_pair(1, (2, 3, 11, 13))
    x, pan = x.double().numpy(), pan.double().numpy()
    rmax = 1.0 if rho_max is None else rho_max
    rho = metrics.local_corr(x, pan, win)
    nearest = float(np.abs(rho - rmax).min())
    assert nearest > 1e-6
    if rho_max is not None:
        assert (rho < rmax).any() and (rho > rmax).any()      # both sides of the kink are present
    sxx = metrics._lc_moments(x, pan, win)[2]
    r_min = float(np.sqrt(sxx.min()))
    assert r_min > 1e3 * h and 2.0 * h / r_min < nearest
    n, count = win * win, rho.size
    tol = 4.0 * h * h * n / (count * r_min ** 3) + (2 * n + 10) * 2.0 * U / h
    loss, _, grad = metrics.local_corr_loss(x, pan, win, rho_max)
    fd = np.zeros_like(x)
    flat, out = x.reshape(-1), fd.reshape(-1)
    for k in range(flat.size):
        keep = flat[k]
        flat[k] = keep + h
        up = metrics.local_corr_loss(x, pan, win, rho_max)[0]
        flat[k] = keep - h
        dn = metrics.local_corr_loss(x, pan, win, rho_max)[0]
        flat[k] = keep
        out[k] = (up - dn) / (2.0 * h)
    worst = float(np.abs(grad - fd).max())
    print(f"win={win} rho_max={rho_max}: loss {loss:.12g}, max|g| {np.abs(grad).max():.3e}, worst difference {worst:.3e}, bound {tol:.3e}")
    assert np.abs(grad).max() > 1e3 * tol                     # the bound is small against what it checks
    assert worst <= tol


def test_rho_max_per_band_and_weight():
    x, pan = random_pair(6, (2, 3, 9, 10))
    l3, m3, g3 = metrics.local_corr_loss(x, pan, 4, (0.2, 0.5, 1.0))
    parts = [metrics.local_corr_loss(x[:, c:c + 1], pan, 4, r) for c, r in enumerate((0.2, 0.5, 1.0))]
    assert abs(l3 - np.mean([p[0] for p in parts])) < 1e-15 and abs(m3 - np.mean([p[1] for p in parts])) < 1e-15
    for c, p in enumerate(parts):
        assert np.allclose(g3[:, c:c + 1], p[2] / 3.0, rtol=0, atol=1e-16)
    assert np.allclose(metrics.local_corr_loss(x, pan, 4, 0.5, weight=0.25)[2], 0.25 * metrics.local_corr_loss(x, pan, 4, 0.5)[2],
                       rtol=1e-15, atol=0)
    with pytest.raises(ValueError, match="rho_max"):
        metrics.local_corr_loss(x, pan, 4, (0.2, 0.5))
    with pytest.raises(ValueError, match="window"):
        metrics.local_corr(x, pan, 10)
    with pytest.raises(ValueError, match="pan"):
        metrics.local_corr(x, x, 4)


def test_structure_refine_on_the_host_lowers_the_loss_every_step():
    """[1, 4, 48, 48]: bands of 3 x 3 box-smoothed noise, a PAN that is their mean plus noise (local_corr_refs.smooth_scene).
    step = 1e-3, found on the CPU: the loss (4 x 4 windows, rho_max None) goes 0.576169 -> 0.463288 -> 0.371580 -> 0.299424 ->
    0.243256.  (3e-3 still descends, 0.576 -> 0.067; 1e-4 moves it by 2 % a step.)"""
    x, pan = smooth_scene()
    f = x.double().numpy()
    losses = [metrics.local_corr_loss(f, pan, 4)[0]]
    for _ in range(4):
        f = tiling.structure_refine(f, pan.numpy(), 1e-3, iters=1)
        losses.append(metrics.local_corr_loss(f, pan, 4)[0])
    print("losses", [f"{v:.6f}" for v in losses])
    assert all(b < a for a, b in zip(losses, losses[1:]))
    assert abs(losses[0] - 0.576169) < 5e-6 and abs(losses[-1] - 0.243256) < 5e-6
    # four steps in one call are the four calls; a tensor comes back as a tensor; iters = 0 is the identity
    once = tiling.structure_refine(x, pan, 1e-3, iters=4)
    assert torch.is_tensor(once) and once.dtype == torch.float64 and np.array_equal(once.numpy(), f)
    assert np.array_equal(tiling.structure_refine(x, pan, 1e-3, iters=0).numpy(), x.double().numpy())
    # with lr_ms each step is followed by one Landweber step
    lr = metrics.mtf_degrade(x.double().numpy(), metrics.band_gains("GF2", 4), 4)
    both = tiling.structure_refine(x, pan, 1e-3, iters=1, lr_ms=lr, sensor="GF2")
    by_hand = tiling.consistency_refine(tiling.structure_refine(x, pan, 1e-3, iters=1), lr, "GF2", 4, 1)
    assert np.array_equal(both.numpy(), by_hand.numpy())


def test_option_checks_of_structure_refine_and_fuse_scene():
    x, pan = smooth_scene(shape=(1, 4, 16, 16))
    lr = torch.zeros(1, 4, 4, 4)
    for bad in ({"iters": 2}, {"step": 1e-3, "relax": 1.0}, {"step": 1e-3, "win": 9}, {"step": 1e-3, "win": 1},
                {"step": 1e-3, "iters": -1}, {"step": 1e-3, "iters": 1.5}, {"step": -1.0}, {"step": None}, "fast", 3):
        with pytest.raises(ValueError, match="structure"):
            tiling.fuse_scene(None, lr, pan, "WV3", structure=bad)
    for kw in ({"win": 9}, {"win": 1}, {"win": 2.5}, {"iters": -1}, {"iters": 0.5}, {"iters": None}, {"iters": "4"}, {"win": None},
               {"win": "4"}, {"iters": True}):
        with pytest.raises(ValueError, match="structure_refine"):
            tiling.structure_refine(x, pan, 1e-3, **kw)
    for step in (-1e-3, float("inf"), float("nan"), None):
        with pytest.raises(ValueError, match="step"):
            tiling.structure_refine(x, pan, step)
    with pytest.raises(ValueError, match="step"):
        tiling.structure_refine(x, pan, "1e-3")
    with pytest.raises(TypeError):
        tiling.structure_refine(x, pan)                       # step has no default
    # numpy numbers are numbers
    a = tiling.structure_refine(x, pan, np.float32(1e-3), iters=np.int64(1), win=np.int32(4))
    assert np.array_equal(a.numpy(), tiling.structure_refine(x, pan, float(np.float32(1e-3)), iters=1, win=4).numpy())
    with pytest.raises(ValueError, match="pan"):
        tiling.structure_refine(x, x, 1e-3)
    with pytest.raises(ValueError, match="window"):
        tiling.structure_refine(x[..., :3, :], pan[..., :3, :], 1e-3)
    with pytest.raises(ValueError, match="sensor"):
        tiling.structure_refine(x, pan, 1e-3, lr_ms=lr)


def test_the_three_exports_are_declared_and_built():
    import ctypes
    from tmdiff_amd import _lib
    with open(os.path.join(ROOT, "include", "tmdiff_hip.h")) as f:
        header = f.read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in EXPORTS:
        assert re.search(r"\b(int|size_t)\s+%s\(" % name, header), f"{name} is not declared in include/tmdiff_hip.h"
        assert name in _lib.SIGNATURES, name
        assert getattr(raw, name) is not None
    with open(os.path.join(ROOT, "tmdiff_amd", "csrc", "local_corr.hip")) as f:
        src = f.read()
    assert "atomic" not in src.replace("No atomics", "")


@pytest.mark.parametrize("b,c,h,w,win,ok", [(1, 1, 2, 2, 2, True), (1, 16, 8, 8, 8, True), (3, 4, 37, 70, 7, True), (1, 17, 8, 8, 4, False),
                                            (1, 4, 8, 8, 9, False), (1, 4, 8, 8, 1, False), (1, 4, 3, 8, 4, False), (1, 4, 8, 3, 4, False),
                                            (0, 4, 8, 8, 4, False), (1, 16, 16384, 8192, 4, False), (1, 16, 16384, 8191, 4, True)])
def test_supported_and_workspace_at_the_documented_limits(b, c, h, w, win, ok):
    from tmdiff_amd import ops
    from tmdiff_amd._lib import lib
    assert ops.local_corr_loss_supported(b, c, h, w, win) is ok
    th, tw = ops.LOCAL_CORR_TILE
    want = 16 * b * (-(-h // th)) * (-(-w // tw)) if ok else 0
    assert lib.tmdiff_local_corr_loss_workspace_bytes(b, c, h, w, win) == want


def test_entry_point_refuses_without_launching():
    """Unsupported extents, window or weight: TMDIFF_E_UNSUPPORTED before any pointer is looked at (all are NULL)."""
    from tmdiff_amd import _lib
    call = _lib.lib.tmdiff_local_corr_loss
    unsupported, invalid = -2, -1            # TMDIFF_E_UNSUPPORTED, TMDIFF_E_INVALID (include/tmdiff_hip.h)
    for win, wt, dims in ((9, 1.0, (1, 4, 16, 16)), (1, 1.0, (1, 4, 16, 16)), (4, 1.0, (1, 17, 16, 16)), (4, 1.0, (1, 4, 3, 16)),
                          (4, -1.0, (1, 4, 16, 16)), (4, float("nan"), (1, 4, 16, 16)), (4, float("inf"), (1, 4, 16, 16))):
        assert call(None, None, None, None, win, wt, 0, None, None, None, None, 0, *dims, None) == unsupported, (win, wt, dims)
    assert call(None, None, None, None, 4, 1.0, 0, None, None, None, None, 0, 1, 4, 16, 16, None) == invalid   # null tensors


def test_the_rho_max_table_cache_is_bounded():
    """_rho_max_table keeps the last few tables (the CPU stands in for the device: nothing touches the GPU)."""
    from tmdiff_amd import ops
    keep = dict(ops._LCORR_RHO_MAX)
    ops._LCORR_RHO_MAX.clear()
    try:
        for k in range(3 * ops._LCORR_RHO_MAX_TABLES):
            t = ops._rho_max_table(0.5 + 0.01 * k, 3, "cpu")
            assert t.dtype == torch.float64 and t.tolist() == [0.5 + 0.01 * k] * 3
            assert ops._rho_max_table(0.5 + 0.01 * k, 3, "cpu") is t
        assert len(ops._LCORR_RHO_MAX) == ops._LCORR_RHO_MAX_TABLES
        assert ops._rho_max_table(None, 3, "cpu") is None
    finally:
        ops._LCORR_RHO_MAX.clear()
        ops._LCORR_RHO_MAX.update(keep)
