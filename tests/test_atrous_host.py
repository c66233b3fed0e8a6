"""CPU-only tests of a-trous wavelet pansharpening: the float64 host definitions ``metrics.atrous_lowpass`` / ``awlp_inject`` /
``awlp``, ``tiling.awlp_fuse`` on host data, and the argument checks of the C entry points.

The low-pass is held to independent statements: a direct 25-tap dilated double loop with clamped indices written here, the
closed-form response to an impulse, exact reproduction of constants and of affine maps on a dyadic grid, the 1-D filter on a
1 x W plane, and the chain of single levels.  The fusion is pinned to code that is already tested: in its additive form it is
``metrics.mtf_glp(mode="glp")`` with the one low-pass plane given to every band.

The file also holds what the GPU test (tests/test_gpu_atrous.py) is measured against: its cases (``AWLP_CASES``) and the
tolerance of the whole chain.  The device keeps every level of the low-pass PAN and the result in float32, which
``metrics.awlp(storage=np.float32)`` restates; the distance of that run from the float64 run is measured here, as
max |F32 - F64| in float32 ulps of max |F64| (``AWLP_RESTATEMENT_U``), and the device is held to 4 times the figure, rounded up
-- the rule of ``tv_tol_u``."""
import numpy as np
import pytest
import torch

# name -> (B, C, H, W), ratio, mode: ragged tiles in both axes, a batch, both ratios, both modes
AWLP_CASES = {
    "4 bands x4 40x72 awlp": dict(shape=(1, 4, 40, 72), ratio=4, mode="awlp"),
    "3 bands x2 34x66 awlp": dict(shape=(2, 3, 34, 66), ratio=2, mode="awlp"),
    "8 bands x4 36x44 atwt": dict(shape=(1, 8, 36, 44), ratio=4, mode="atwt"),
}
# worst |F32 - F64| / ulp32(max |F64|) of metrics.awlp(storage=np.float32) against the float64 run, as test_awlp_tolerance measures
# it (and holds it to)
AWLP_RESTATEMENT_U = {"4 bands x4 40x72 awlp": 1.129, "3 bands x2 34x66 awlp": 1.192, "8 bands x4 36x44 atwt": 1.572}


def awlp_scene(name):
    """(ms_exp, pan) of a case, float32: smooth bands of different contrast plus noise, and a PAN that is their mean plus detail."""
    b, c, h, w = AWLP_CASES[name]["shape"]
    rng = np.random.default_rng(1000 * h + w)
    yy, xx = np.mgrid[:h, :w]
    ms = np.empty((b, c, h, w))
    for i in range(b):
        for k in range(c):
            ms[i, k] = 0.2 + (0.1 + 0.05 * k) * np.sin(0.11 * (k + 1) * xx + 0.07 * yy + i) + 0.3 * xx / w + 0.05 * rng.random((h, w))
    pan = ms.mean(axis=1, keepdims=True) + 0.1 * rng.random((b, 1, h, w))
    return ms.astype(np.float32), pan.astype(np.float32)


def awlp_error_u(f, want):
    """max |f - want| in float32 ulps of max |want|, the differences formed in float64."""
    f, want = np.asarray(f, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(f - want).max() / np.spacing(np.float32(np.abs(want).max())))


def awlp_tol_u(name):
    """The GPU test's tolerance for the whole chain in u: 4 x the restatement's figure, rounded up."""
    return float(np.ceil(4.0 * AWLP_RESTATEMENT_U[name]))


def lowpass_direct(x, levels):
    """The independent restatement: level by level, the 25 taps of the dilated 5 x 5 kernel at clamped indices."""
    taps = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
    c = np.asarray(x, dtype=np.float64)
    h, w = c.shape
    for level in range(1, levels + 1):
        d = 2 ** (level - 1)
        nxt = np.zeros((h, w))
        for i in range(h):
            for j in range(w):
                acc = 0.0
                for p in range(5):
                    for q in range(5):
                        acc += taps[p] * taps[q] * c[min(max(i + (p - 2) * d, 0), h - 1), min(max(j + (q - 2) * d, 0), w - 1)]
                nxt[i, j] = acc
        c = nxt
    return c


# ---- the low-pass -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (7, 20), (13, 13)])
def test_lowpass_against_the_direct_restatement(shape):
    from tmdiff_amd import metrics
    x = np.random.default_rng(shape[0] * 100 + shape[1]).random(shape)
    for levels in (1, 2, 3):
        assert np.abs(metrics.atrous_lowpass(x, levels) - lowpass_direct(x, levels)).max() <= 1e-13


def test_lowpass_impulse_response():
    from tmdiff_amd import metrics
    x = np.zeros((31, 31))
    x[15, 15] = 1.0
    line = np.array([1, 4, 10, 20, 31, 40, 44, 40, 31, 20, 10, 4, 1]) / 256.0
    want = np.zeros((31, 31))
    want[9:22, 9:22] = np.outer(line, line)
    assert np.array_equal(metrics.atrous_lowpass(x, 2), want)
    assert metrics.ATROUS_TAPS == (1 / 16, 4 / 16, 6 / 16, 4 / 16, 1 / 16) and sum(metrics.ATROUS_TAPS) == 1.0
    assert metrics.ATROUS_MAX_LEVELS == 3 and metrics.ATROUS_MODES == ("atwt", "awlp")


def test_lowpass_exact_properties():
    from tmdiff_amd import metrics
    rng = np.random.default_rng(5)
    for levels in (1, 2, 3):
        # constants: exact for a value of at most 49 significant bits, every float32 among them (the partial sums are 5, 11, 15
        # and 16 sixteenths of it); a full float64 mantissa is reproduced to an ulp
        flat = np.full((2, 9, 11), np.float64(np.float32(0.37)))
        assert np.array_equal(metrics.atrous_lowpass(flat, levels), flat)
        assert np.abs(metrics.atrous_lowpass(np.full((2, 9, 11), 0.37), levels) - 0.37).max() <= 2.0 ** -53
        x = rng.integers(0, 256, (2, 9, 11)) / 256.0                                                                     # a dyadic grid
        assert np.array_equal(metrics.atrous_lowpass(0.5 * x + 0.25, levels), 0.5 * metrics.atrous_lowpass(x, levels) + 0.25)
        # a 1 x W plane is the 1-D filter: the column pass of a one-row plane sums the taps of one value, exactly
        row = rng.integers(0, 256, (1, 23)).astype(np.float64)
        want = row
        for level in range(levels):
            idx = [np.clip(np.arange(23) + (j - 2) * 2 ** level, 0, 22) for j in range(5)]
            want = sum(t * want[:, i] for t, i in zip(metrics.ATROUS_TAPS, idx))
        assert np.array_equal(metrics.atrous_lowpass(row, levels), want)
        assert np.array_equal(metrics.atrous_lowpass(row.T, levels), want.T)
        # constant along an axis stays constant along it
        col = np.broadcast_to(rng.random((9, 1)), (9, 11))
        got = metrics.atrous_lowpass(col, levels)
        assert np.array_equal(got, np.broadcast_to(got[:, :1], (9, 11)))
        got = metrics.atrous_lowpass(col.T, levels)
        assert np.array_equal(got, np.broadcast_to(got[:1, :], (11, 9)))


def test_lowpass_levels_chain_and_storage():
    from tmdiff_amd import metrics
    x = np.random.default_rng(6).random((2, 3, 17, 9)).astype(np.float32)
    # three levels at once are three single levels, through `first` and through a chain written here
    chain = x
    for first in (1, 2, 3):
        chain = metrics.atrous_lowpass(chain, 1, first=first)
    assert np.array_equal(metrics.atrous_lowpass(x, 3), chain)
    assert np.array_equal(metrics.atrous_lowpass(metrics.atrous_lowpass(x, 1), 2, first=2), chain)
    assert np.array_equal(chain[0, 0], lowpass_chain(x[0, 0], 3))
    chain = x
    for first in (1, 2, 3):
        chain = metrics.atrous_lowpass(chain, 1, storage=np.float32, first=first)
    assert np.array_equal(metrics.atrous_lowpass(x, 3, storage=np.float32), chain)
    one = metrics.atrous_lowpass(x, 1, storage=np.float32)
    assert one.dtype == np.float32 and np.array_equal(one, metrics.atrous_lowpass(x, 1).astype(np.float32))
    three = metrics.atrous_lowpass(x, 3, storage=np.float32)
    assert three.dtype == np.float32 and np.abs(three.astype(np.float64) - metrics.atrous_lowpass(x, 3)).max() <= 3 * 2.0 ** -24
    for bad in (0, 4, 1.5, True):
        with pytest.raises(ValueError):
            metrics.atrous_lowpass(x, bad)
    for levels, first in ((1, 0), (1, 4), (2, 3), (3, 2)):
        with pytest.raises(ValueError):
            metrics.atrous_lowpass(x, levels, first=first)
    with pytest.raises(ValueError):
        metrics.atrous_lowpass(np.zeros(5), 1)
    with pytest.raises(ValueError):
        metrics.atrous_lowpass(np.zeros((0, 5)), 1)


def lowpass_chain(x, levels):
    """``levels`` single levels, each written as one separable pass at its own dilation on the plane before."""
    from tmdiff_amd import metrics
    c = np.asarray(x, dtype=np.float64)
    h, w = c.shape
    for level in range(levels):
        d = 2 ** level
        r = sum(t * c[:, np.clip(np.arange(w) + (j - 2) * d, 0, w - 1)] for j, t in enumerate(metrics.ATROUS_TAPS))
        c = sum(t * r[np.clip(np.arange(h) + (j - 2) * d, 0, h - 1), :] for j, t in enumerate(metrics.ATROUS_TAPS))
    return c


def test_integer_images_are_exact_in_float32():
    """What the GPU test's torch.equal rests on: on 8-bit integer images two levels, and on binary images three, are exact in
    float32 at every level, so rounding the levels changes nothing.  (A level multiplies by 1 / 256: 8 + 8 + 8 = 24 bits.)"""
    from tmdiff_amd import metrics
    rng = np.random.default_rng(7)
    x8 = rng.integers(0, 256, (2, 37, 41)).astype(np.float64)
    x1 = rng.integers(0, 2, (2, 37, 41)).astype(np.float64)
    for x, levels in ((x8, 1), (x8, 2), (x1, 3)):
        want = metrics.atrous_lowpass(x, levels)
        got = metrics.atrous_lowpass(x, levels, storage=np.float32)
        assert np.array_equal(got.astype(np.float64), want)


# ---- the fusion ---------------------------------------------------------------------------------------------------------------------
def test_atwt_is_additive_glp_on_the_one_lowpass_plane():
    from tmdiff_amd import metrics
    for name, case in AWLP_CASES.items():
        ms, pan = awlp_scene(name)
        low = metrics.atrous_lowpass(pan, 1 if case["ratio"] == 2 else 2)
        want = metrics.mtf_glp(ms, pan, None, case["ratio"], mode="glp", pan_lp=np.broadcast_to(low, ms.shape))
        got = metrics.awlp(ms, pan, case["ratio"], "atwt")
        assert got.shape == ms.shape and np.abs(got - want).max() <= 1e-12
        assert np.array_equal(got, metrics.awlp_inject(ms, pan, low, metrics.plane_moments(ms, low), "atwt"))
    hwc = metrics.awlp(np.moveaxis(ms[0], 0, -1), pan[0, 0], 4, "awlp", hwc=True)
    assert np.array_equal(np.moveaxis(hwc, -1, 0), metrics.awlp(ms[0], pan[0], 4, "awlp"))


def test_awlp_properties():
    from tmdiff_amd import metrics
    rng = np.random.default_rng(8)
    pan = rng.random((1, 1, 24, 28))
    grey = np.broadcast_to(0.2 + 0.6 * rng.random((1, 1, 24, 28)), (1, 4, 24, 28))
    assert np.array_equal(metrics.awlp(grey, pan, 4, "awlp"), metrics.awlp(grey, pan, 4, "atwt"))      # M_c / I == 1 exactly
    # equal band variances, so equal a_c: the bands are one plane, flipped and transposed
    yy, xx = np.mgrid[:24, :24]
    base = 0.5 + 0.2 * np.sin(0.3 * xx + 0.2 * yy) + 0.02 * rng.random((24, 24))
    ms = np.stack([base, base[::-1], base[:, ::-1], base.T])[None]
    pan = ms.mean(axis=1, keepdims=True) + 0.02 * rng.random((1, 1, 24, 24))       # detail small against I: 1 + a D / I > 0
    fused = metrics.awlp(ms, pan, 4, "awlp")
    assert metrics.sam(np.moveaxis(ms[0], 0, -1), np.moveaxis(fused[0], 0, -1)) <= 1e-5                # degrees; acos near 1
    cosine = (ms * fused).sum(1) / np.sqrt((ms * ms).sum(1) * (fused * fused).sum(1))
    assert np.abs(cosine - 1.0).max() <= 1e-14
    # a pixel with I == 0 is returned unchanged and finite
    ms0 = ms.copy()
    ms0[0, :, 3, 5] = (0.25, -0.25, 0.5, -0.5)
    out = metrics.awlp(ms0, pan, 4, "awlp")
    assert np.isfinite(out).all() and np.array_equal(out[0, :, 3, 5], ms0[0, :, 3, 5])
    # a constant PAN: var(L) == 0, non-finite throughout
    for mode in metrics.ATROUS_MODES:
        assert not np.isfinite(metrics.awlp(ms, np.full((1, 1, 24, 24), 0.4), 4, mode)).any()


def test_awlp_tolerance():
    """Measures the working bound of the GPU test: the device's storage (float32 levels and result) against the float64 run."""
    from tmdiff_amd import metrics
    got = {}
    for name, case in AWLP_CASES.items():
        ms, pan = awlp_scene(name)
        f32 = metrics.awlp(ms, pan, case["ratio"], case["mode"], storage=np.float32)
        assert f32.dtype == np.float32
        got[name] = awlp_error_u(f32, metrics.awlp(ms, pan, case["ratio"], case["mode"]))
    print("awlp(storage=float32), worst |F32 - F64| in float32 ulps of max |F64|: " + "  ".join(f"{k}: {v:.3f}" for k, v in got.items()))
    for name, v in got.items():
        assert v <= AWLP_RESTATEMENT_U[name] + 5e-4, (name, v)
        assert awlp_tol_u(name) == np.ceil(4.0 * AWLP_RESTATEMENT_U[name])


# ---- arguments and users ------------------------------------------------------------------------------------------------------------
def test_arguments():
    from tmdiff_amd import metrics
    from tmdiff_amd.tiling import awlp_fuse
    ms, pan = awlp_scene("4 bands x4 40x72 awlp")
    low = metrics.atrous_lowpass(pan, 2)
    mo = metrics.plane_moments(ms, low)
    for call in (lambda: metrics.awlp(ms, pan, 3),
                 lambda: metrics.awlp(ms, pan, 4, "glp"),
                 lambda: metrics.awlp(ms, pan[..., :-1], 4),
                 lambda: metrics.awlp(np.zeros((1, 15, 8, 8)), np.zeros((1, 1, 8, 8)), 4),
                 lambda: metrics.awlp_inject(ms, pan, low, mo, "hpm"),
                 lambda: metrics.awlp_inject(ms, pan, low[..., :-1], mo, "awlp"),
                 lambda: metrics.awlp_inject(ms, pan, low, mo[:, :-1], "awlp"),
                 lambda: awlp_fuse(ms[..., ::4, ::4], pan, mode="cbd"),
                 lambda: awlp_fuse(ms[..., ::4, ::4], pan, score="qnr"),
                 lambda: awlp_fuse(ms[..., ::4, ::4], pan, score=True),                   # scores are made on the GPU
                 lambda: awlp_fuse(ms[..., ::4, ::4], pan, consistency={"iters": 2}),     # ... which needs the sensor
                 lambda: awlp_fuse(ms[..., ::4, ::4], pan[..., :-4], ratio=4)):
        with pytest.raises(ValueError):
            call()


def test_awlp_fuse_on_host_data():
    from tmdiff_amd import metrics
    from tmdiff_amd.tiling import awlp_fuse, consistency_refine
    ms, pan = awlp_scene("4 bands x4 40x72 awlp")
    lr = np.ascontiguousarray(ms[..., 2::4, 2::4])
    for mode in metrics.ATROUS_MODES:
        got = awlp_fuse(torch.from_numpy(lr), torch.from_numpy(pan), mode=mode)
        assert torch.is_tensor(got) and got.dtype == torch.float64
        want = metrics.awlp(metrics.upsample_poly23(lr, 4), pan, 4, mode)
        assert np.array_equal(got.numpy(), want) and np.array_equal(awlp_fuse(lr, pan, mode=mode), want)
    refined = awlp_fuse(lr, pan, "QB", consistency={"iters": 2})
    assert np.array_equal(refined, consistency_refine(metrics.awlp(metrics.upsample_poly23(lr, 4), pan, 4), lr, "QB", 4, iters=2))


def test_exports_are_declared_bound_and_exported():
    import os
    from tmdiff_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tmdiff_hip.h")).read()
    for name in ("tmdiff_atrous_supported", "tmdiff_atrous_lowpass", "tmdiff_awlp_inject"):
        assert f"int {name}(" in header and name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert _lib.ABI_VERSION == 6


def test_c_entry_points_check_their_arguments():
    from tmdiff_amd._lib import lib
    assert lib.tmdiff_atrous_supported(1, 1, 1, 1, 1, 1) == 1 and lib.tmdiff_atrous_supported(2, 40, 7, 9, 3, 1) == 1
    assert lib.tmdiff_atrous_supported(1, 1, 8, 8, 1, 3) == 1 and lib.tmdiff_atrous_supported(1, 1, 8, 8, 2, 2) == 1
    for bad in ((1, 1, 8, 8, 0, 1), (1, 1, 8, 8, 4, 1), (1, 1, 8, 8, 1, 0), (1, 1, 8, 8, 2, 3), (1, 1, 8, 8, 1, 4), (0, 1, 8, 8, 2, 1),
                (1, 0, 8, 8, 2, 1), (1, 1, 0, 8, 2, 1), (1, 1, 8, 0, 2, 1), (1, 16, 16384, 8192, 2, 1)):       # the last: 2^31 elements
        assert lib.tmdiff_atrous_supported(*bad) == 0, bad
        assert lib.tmdiff_atrous_lowpass(None, None, *bad, None) not in (0, -1), bad          # refused before the null-pointer check
    assert lib.tmdiff_atrous_lowpass(None, None, 1, 2, 4, 4, 2, 1, None) == -1               # null tensors
    fake = [0x100000 * (i + 1) for i in range(5)]                                            # never dereferenced
    assert lib.tmdiff_atrous_lowpass(fake[0], fake[0], 1, 2, 4, 4, 2, 1, None) == -1         # out on x: refused
    assert lib.tmdiff_atrous_lowpass(fake[0], fake[0] + 64, 1, 2, 4, 4, 2, 1, None) == -1    # ... and a partial overlap
    for bad in ((1, 15, 4, 4, 0), (1, 0, 4, 4, 0), (0, 2, 4, 4, 0), (1, 2, 0, 4, 1), (1, 2, 4, 0, 1), (1, 2, 4, 4, 2), (1, 2, 4, 4, -1),
                (1, 14, 16384, 16384, 1)):
        assert lib.tmdiff_awlp_inject(*[None] * 5, *bad, None) not in (0, -1), bad
    assert lib.tmdiff_awlp_inject(*[None] * 5, 1, 14, 4, 4, 1, None) == -1                   # null tensors
    assert lib.tmdiff_awlp_inject(*fake[:3], fake[3] + 4, fake[4], 1, 2, 4, 4, 1, None) == -1   # moments not 8-byte aligned
