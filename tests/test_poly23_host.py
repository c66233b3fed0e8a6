"""CPU-only tests of the 23-tap polynomial interpolator (the Pansharpening Toolbox's interp23tap, which makes the ``lms`` of the
PanCollection files): the float64 host definition ``metrics.upsample_poly23`` against an independent statement -- explicit zero
insertion and the full 23-tap circular correlation, along H then W, as np.roll sums -- its structural properties, the argument
checks of the C entry point, of ``ops.upsample_poly23`` and of ``fuse_scene(interp=...)``, and ``LRHRDataset`` on a file
without ``lms``.

The file also holds what the GPU test (tests/test_gpu_poly23.py) is measured against: its inputs (``poly23_input``) and a
float32 restatement of the kernel's arithmetic order (``poly23_float32``), whose error against the float64 definition sets that
test's tolerance.  Measured here over POLY23_GPU_SHAPES, in units of eps m (eps = 2^-24, m = max|x|): 1.725 at x2 (either phase),
2.071 at x4; the GPU test allows 7 and 9 (4 x, rounded up), far inside the worst-case bounds of 40 and 200."""
import numpy as np
import pytest
import torch

# c_0 .. c_11 of the half-band kernel; h[d] = 2 c_|d|, d = -11 .. 11
HALF_BAND = (0.5, 0.305334091185, 0, -0.072698593239, 0, 0.021809577942, 0, -0.005192756653, 0, 0.000807762146, 0, -0.000060081482)
SHAPES = [(1, 1), (2, 3), (5, 7), (16, 16), (17, 33)]
CASES = [(2, 1), (2, 0), (4, 1)]          # (ratio, phase)

# the GPU test's inputs: below the reach (coordinates wrap more than once), exactly one 16 x 16 input tile, tile remainders,
# several tiles of the x4 output on one axis only
POLY23_GPU_SHAPES = [(1, 1), (2, 3), (5, 7), (16, 16), (17, 33), (40, 24)]
EPS = 2.0 ** -24
# max error of poly23_float32 against metrics.upsample_poly23 over POLY23_GPU_SHAPES, in eps m, as measured by
# test_float32_restatement_error (which holds the figures to these values): x2 (either phase), x4
RESTATEMENT_EPS = {2: 1.725, 4: 2.071}
# the GPU test's tolerance: 4 x the measured figure, rounded up; never above the worst-case bounds 40 (x2) and 200 (x4) eps m
GPU_TOL_EPS = {2: 7.0, 4: 9.0}
WORST_CASE_EPS = {2: 40.0, 4: 200.0}


def poly23_input(h, w):
    return torch.randn(2, 3, h, w, generator=torch.Generator().manual_seed(2300 + 100 * h + w))


def stage_statement(x, phase, axis):
    """Zero insertion (the samples at the outputs of parity ``phase``), then u[n] = sum_d h[d] z[(n + d) mod 2L]."""
    x = np.moveaxis(np.asarray(x, dtype=np.float64), axis, -1)
    z = np.zeros(x.shape[:-1] + (2 * x.shape[-1],))
    z[..., phase::2] = x
    u = sum(2.0 * HALF_BAND[abs(d)] * np.roll(z, -d, axis=-1) for d in range(-11, 12))
    return np.moveaxis(u, -1, axis)


def poly23_statement(x, ratio, phase=1):
    y = np.asarray(x, dtype=np.float64)
    for p in ((1, 0) if ratio == 4 else (phase,)):
        y = stage_statement(stage_statement(y, p, -2), p, -1)
    return y


def poly23_float32(x, ratio, phase=1):
    """The kernel's arithmetic in float32 on the host: per stage H then W; an interpolated output is the six pair sums
    x[lo - j] + x[lo + 1 + j] (one rounding each) run through fused multiply-adds from j = 5 down to 0, starting from 0 (a fused
    multiply-add is the float64 product and sum, both exact or correctly rounded, rounded once more to float32); a copied
    output is a move."""
    from tmdiff_amd.metrics import POLY23_TAPS
    taps = [np.float32(a) for a in POLY23_TAPS]
    y = np.asarray(x, dtype=np.float32)
    for p in ((1, 0) if ratio == 4 else (phase,)):
        for axis in (-2, -1):
            y = np.moveaxis(y, axis, -1)
            n = y.shape[-1]
            lo = np.arange(n) - p
            acc = np.zeros(y.shape, dtype=np.float32)
            for j in range(5, -1, -1):
                pair = y[..., (lo - j) % n] + y[..., (lo + 1 + j) % n]
                assert pair.dtype == np.float32
                acc = (np.float64(taps[j]) * pair.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
            u = np.empty(y.shape[:-1] + (2 * n,), dtype=np.float32)
            u[..., p::2] = y
            u[..., 1 - p::2] = acc
            y = np.moveaxis(u, -1, axis)
    return y


def test_coefficients():
    from tmdiff_amd.metrics import POLY23_TAPS
    assert POLY23_TAPS == tuple(2.0 * c for c in HALF_BAND[1::2]) and len(POLY23_TAPS) == 6
    assert abs(2.0 * sum(POLY23_TAPS) - 0.999999999596) < 1e-12
    assert 2.0 * HALF_BAND[0] == 1.0 and not any(HALF_BAND[2::2])


@pytest.mark.parametrize("h,w", SHAPES)
@pytest.mark.parametrize("ratio,phase", CASES)
def test_host_poly23_against_the_statement(h, w, ratio, phase):
    from tmdiff_amd import metrics
    x = np.random.default_rng(100 * h + w).standard_normal((2, 3, h, w))
    got, want = metrics.upsample_poly23(x, ratio, phase), poly23_statement(x, ratio, phase)
    assert got.shape == want.shape == (2, 3, ratio * h, ratio * w) and got.dtype == np.float64
    err = np.abs(got - want).max() / np.abs(x).max()
    print(f"poly23 x{ratio} phase {phase} {h} x {w}: max error {err:.3e} m")
    assert err <= 1e-13


@pytest.mark.parametrize("h,w", SHAPES)
def test_host_poly23_structure(h, w):
    from tmdiff_amd import metrics
    up = metrics.upsample_poly23
    x = np.random.default_rng(7 * h + w).standard_normal((2, 3, h, w))
    y4, y2, y20 = up(x, 4), up(x, 2), up(x, 2, 0)
    # the samples survive as exact copies, registered to the PAN
    assert np.array_equal(y4[..., 2::4, 2::4], x) and np.array_equal(y2[..., 1::2, 1::2], x) and np.array_equal(y20[..., ::2, ::2], x)
    # x4 is the phase-1 stage followed by the phase-0 stage
    assert np.array_equal(y4, up(y2, 2, 0))
    # a constant image stays constant
    for ratio, phase in CASES:
        c = up(np.full((h, w), 3.25), ratio, phase)
        assert np.abs(c / 3.25 - 1.0).max() <= 1e-8
    # circular: rolling the input by (a, b) rolls the output by (ratio a, ratio b)
    for ratio, phase in CASES:
        rolled = up(np.roll(x, (3, 5), axis=(-2, -1)), ratio, phase)
        assert np.array_equal(rolled, np.roll(up(x, ratio, phase), (3 * ratio, 5 * ratio), axis=(-2, -1)))


def test_host_poly23_accepted_inputs():
    from tmdiff_amd import metrics
    x = np.random.default_rng(3).standard_normal((1, 2, 5, 7)).astype(np.float32)
    want = metrics.upsample_poly23(x)
    assert want.shape == (1, 2, 20, 28) and want.dtype == np.float64
    assert np.array_equal(metrics.upsample_poly23(torch.from_numpy(x)), want)
    assert np.array_equal(metrics.upsample_poly23(x[0]), want[0]) and np.array_equal(metrics.upsample_poly23(x[0, 1]), want[0, 1])
    for bad in (dict(ratio=3), dict(ratio=4, phase=0), dict(ratio=2, phase=2)):
        with pytest.raises(ValueError):
            metrics.upsample_poly23(x, **bad)
    with pytest.raises(ValueError):
        metrics.upsample_poly23(np.zeros(5))


def test_float32_restatement_error():
    """What float32 costs in the kernel's order of operations, which sets the GPU test's tolerance (4 x, rounded up)."""
    from tmdiff_amd import metrics
    worst = {2: 0.0, 4: 0.0}
    for h, w in POLY23_GPU_SHAPES:
        x = poly23_input(h, w).numpy()
        m = float(np.abs(x).max())
        for ratio, phase in CASES:
            err = np.abs(poly23_float32(x, ratio, phase).astype(np.float64) - metrics.upsample_poly23(x, ratio, phase)).max() / (EPS * m)
            print(f"float32 restatement x{ratio} phase {phase} {h} x {w}: {err:.3f} eps m")
            worst[ratio] = max(worst[ratio], err)
    print(f"float32 restatement, worst: {worst}")
    for ratio in (2, 4):
        assert worst[ratio] <= RESTATEMENT_EPS[ratio] <= WORST_CASE_EPS[ratio]
        assert GPU_TOL_EPS[ratio] == np.ceil(4.0 * RESTATEMENT_EPS[ratio]) <= WORST_CASE_EPS[ratio]
    # the restatement keeps the copies and the composition exactly, as the kernel must
    x = poly23_input(17, 33).numpy()
    assert np.array_equal(poly23_float32(x, 4)[..., 2::4, 2::4], x)
    assert np.array_equal(poly23_float32(x, 4), poly23_float32(poly23_float32(x, 2, 1), 2, 0))


def test_entry_point_is_declared_exported_and_bound():
    import ctypes
    import os
    import re
    from conftest import ROOT
    from tmdiff_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmdiff_hip.h")).read(), flags=re.S)
    name = "tmdiff_upsample_poly23"
    assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in include/tmdiff_hip.h"
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and len(_lib.SIGNATURES[name][1]) == 8
    assert _lib.ABI_VERSION == 6


def test_entry_point_refuses_what_it_does_not_take():
    """Argument checks come before any launch and before the null-pointer check, so they run without a GPU."""
    from tmdiff_amd import _lib
    lib = _lib.lib
    msg = lambda: lib.tmdiff_last_error_string().decode()
    up = lib.tmdiff_upsample_poly23
    assert up(None, None, 1, 8, 8, 3, 1, None) == -2 and "2 or 4" in msg()            # ratio
    assert up(None, None, 1, 8, 8, 8, 1, None) == -2
    assert up(None, None, 1, 8, 8, 2, 2, None) == -2 and "phase" in msg()             # phase
    assert up(None, None, 1, 8, 8, 2, -1, None) == -2
    assert up(None, None, 1, 8, 8, 4, 0, None) == -2 and "1 at ratio 4" in msg()      # phase 0 at ratio 4
    assert up(None, None, 8, 8192, 8192, 2, 1, None) == -2 and "2^31" in msg()        # 2^31 outputs
    assert up(None, None, 8, 4096, 4096, 4, 1, None) == -2 and "2^31" in msg()
    assert up(None, None, -1, 8, 8, 4, 1, None) == -2 and "planes" in msg()           # extents
    assert up(None, None, 1, 0, 8, 4, 1, None) == -2 and up(None, None, 1, 8, -3, 2, 0, None) == -2
    assert up(None, None, 0, 8, 8, 4, 1, None) == 0 and up(None, None, 0, 8, 8, 2, 0, None) == 0
    assert up(None, None, 1, 8, 8, 4, 1, None) == -1 and "null" in msg()
    assert up(None, None, 1, 8, 8, 2, 0, None) == -1 and "null" in msg()


def test_ops_refuses_before_the_library_is_called():
    from tmdiff_amd import ops
    assert callable(ops.upsample_poly23)
    with pytest.raises(ValueError):
        ops.upsample_poly23(torch.zeros(1, 1, 8, 8))                  # a host tensor
    for bad in (dict(ratio=3), dict(ratio=4, phase=0), dict(ratio=2, phase=2)):
        with pytest.raises(ValueError):
            ops.upsample_poly23(torch.zeros(1, 1, 8, 8), **bad)


def test_dataset_makes_lms_when_the_file_has_none():
    from tmdiff_amd import metrics
    from tmdiff_amd.data import LRHRDataset
    g = np.random.default_rng(0)
    raw = {"ms": g.integers(0, 2047, (2, 4, 5, 6)).astype(np.float64), "pan": g.integers(0, 2047, (2, 1, 20, 24)).astype(np.float64)}
    ds = LRHRDataset(raw)
    want = metrics.upsample_poly23((raw["ms"] / 2047.0).astype(np.float32), 4)
    assert ds.has_gt is False and len(ds) == 2
    for i in range(2):
        item = ds[i]
        assert item["MS"].dtype == torch.float32 and tuple(item["MS"].shape) == (4, 20, 24)
        assert torch.equal(item["MS"], torch.from_numpy(want[i]).float()) and torch.equal(item["HR"], item["MS"])
        assert torch.equal(item["MS"][:, 2::4, 2::4], item["LR"])
    half = LRHRDataset({"ms": raw["ms"], "pan": raw["pan"][..., ::2, ::2], "gt": g.integers(0, 2047, (2, 4, 10, 12))})
    assert half.has_gt is True
    assert torch.equal(half[1]["MS"], torch.from_numpy(metrics.upsample_poly23((raw["ms"][1] / 2047.0).astype(np.float32), 2)).float())
    # a file that carries lms is read as before
    lms = g.integers(0, 2047, (2, 4, 20, 24)).astype(np.float64)
    kept = LRHRDataset({**raw, "lms": lms})
    assert torch.equal(kept[1]["MS"], torch.from_numpy((lms[1].astype(np.float32) / 2047.0)))
    assert torch.equal(kept[1]["HR"], kept[1]["MS"]) and torch.equal(kept[1]["LR"], ds[1]["LR"])


def test_fuse_scene_refuses_an_unknown_interpolator():
    from tmdiff_amd.tiling import fuse_scene
    with pytest.raises(ValueError, match="interp"):
        fuse_scene(None, torch.zeros(1, 4, 8, 8), torch.zeros(1, 1, 32, 32), "WV3", interp="cubic")
