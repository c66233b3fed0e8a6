"""CPU-only tests of MTF-matched filtering and decimation (Wald's protocol): the float64 host definitions ``metrics.mtf_gains``,
``metrics.mtf_kernel``, ``metrics.fir_decimate`` and ``metrics.mtf_degrade``, ``data.wald_pair`` through the host path,
``LRHRDataset(reduce=...)``, and the argument checks of the C entry point ``tmdiff_fir_decimate`` and of ``ops``.

``mtf_kernel`` is unpinned (the Pansharpening Toolbox is not available): it is held to values computed from the statement of
genMTF in its docstring.  ``fir_decimate`` is held to a direct four-loop restatement with ASYMMETRIC random taps.

The file also holds what the GPU test (tests/test_gpu_mtf.py) is measured against: its inputs and a float32 restatement of the
kernel's summation order (``fir_float32``: acc = 0, then one fused multiply-add per tap in row-major order), whose error against
the float64 definition sets that test's tolerance.  Errors are elementwise, in units of u S with u = 2^-24 and
S = |taps| correlated with |x| at the same pixel.  Measured here at ratio 1, whose pixels include those of every ratio and
offset (a pixel's sum does not depend on the ratio), over MTF_GPU_SHAPES and both tap periods:
    K = 1: 0.998   K = 3: 3.668   K = 7: 4.660   K = 41: 5.088   the real MTF kernels (K = 41, float64 taps rounded): 45.556
(randn taps and images cancel, all-positive MTF taps and images do not: there every partial sum is of the size of S).  The GPU
test allows 4 x that, rounded up -- 4, 15, 19, 21 and 183 u S -- but never more than the a-priori bound
(K^2 + 1) u / (1 - (K^2 + 1) u) S, which holds for any summation order and covers the rounding of the taps to float32:
2, 10, 50 and 1682 u S; so K = 1 is held to 2 u S and K = 3 to 10 u S."""
import math

import numpy as np
import pytest
import torch

U = 2.0 ** -24
# the GPU test's plane extents: one pixel; below the filter radius (coordinates clamp many times); exactly one 16 x 16 output tile
# per axis at x4; tile remainders on both axes and extents that are no multiples of the ratio; several tiles on one axis
MTF_GPU_SHAPES = [(1, 1), (3, 5), (64, 64), (67, 131), (40, 24)]
MTF_KS = (1, 3, 7, 41)
MTF_PERIODS = (3, 1)                       # 2 x 3 planes: a table per band, one table for all
MTF_OFFSETS = {1: [(0, 0)], 2: [(0, 0), (1, 1), (0, 1)], 4: [(0, 0), (1, 1), (2, 2), (3, 3), (1, 3)]}   # the diagonal + one pair off it
# (name, sensor or gains, ratio, pan, image shape) of the GPU test's real MTF kernels; WV3 has 8 bands: a tap period of 8
MTF_REAL_CASES = [("QB", "QB", 4, False, (2, 4, 67, 131)), ("WV3", "WV3", 4, False, (1, 8, 40, 24)),
                  ("0.34 x2", (0.34, 0.34, 0.34), 2, False, (2, 3, 40, 24)), ("QB pan", "QB", 4, True, (2, 1, 64, 64))]
# worst error of fir_float32 against metrics.fir_decimate in u S, as test_float32_restatement_error measures it (and holds it to)
RESTATEMENT_U = {1: 0.998, 3: 3.668, 7: 4.660, 41: 5.088, "mtf": 45.556}


def apriori_u(k):
    """The elementwise a-priori bound in u S: (K^2 + 1) u / (1 - (K^2 + 1) u), over u."""
    n = k * k + 1
    return n / (1.0 - n * U)


def gpu_tol_u(k):
    """The GPU test's tolerance in u S: 4 x the measured figure, rounded up (the margin is for the restatement's emulated fused
    multiply-add), and never above the a-priori bound.  ``k``: K, or "mtf" for the real MTF kernels."""
    return min(float(np.ceil(4.0 * RESTATEMENT_U[k])), apriori_u(41 if k == "mtf" else k))


def mtf_input(h, w, integer=False):
    g = torch.Generator().manual_seed(4100 + 100 * h + w)
    return torch.randint(-8, 9, (2, 3, h, w), generator=g).float() if integer else torch.randn(2, 3, h, w, generator=g)


def mtf_taps(t, k, integer=False):
    """Asymmetric taps [t, k, k]: a flip, a transpose or an offset off by one changes the result."""
    g = torch.Generator().manual_seed(41 * k + t)
    return torch.randint(-3, 4, (t, k, k), generator=g).float() if integer else torch.randn(t, k, k, generator=g)


def mtf_real_input(shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(shape[1] * 1000 + shape[2]))


def fir_float32(x, taps, ratio=1, offset=None):
    """The kernel's arithmetic in float32 on the host: acc = 0, then acc = fma(taps[u][v], x[..], acc) over the taps in
    row-major order (a fused multiply-add is the float64 product, which is exact, plus acc, rounded to float64 and once more to
    float32)."""
    from tmdiff_amd.metrics import fir_decimate_shape
    x = np.asarray(x, dtype=np.float32)
    taps = np.asarray(taps, dtype=np.float32)
    taps = taps[None] if taps.ndim == 2 else taps
    h, w = x.shape[-2:]
    planes, (t, k) = x.size // (h * w), taps.shape[:2]
    (ho, wo), (oy, ox) = fir_decimate_shape(h, w, ratio, offset)
    xp = np.pad(x.reshape(planes, h, w), ((0, 0), (k // 2,) * 2, (k // 2,) * 2), mode="edge").astype(np.float64)
    band = np.tile(taps, (planes // t, 1, 1)).astype(np.float64)
    acc = np.zeros((planes, ho, wo), dtype=np.float32)
    for u in range(k if ho and wo else 0):
        for v in range(k):
            xs = xp[:, oy + u:oy + u + ratio * (ho - 1) + 1:ratio, ox + v:ox + v + ratio * (wo - 1) + 1:ratio]
            acc = (band[:, u, v, None, None] * xs + acc.astype(np.float64)).astype(np.float32)
    return acc.reshape(x.shape[:-2] + (ho, wo))


def error_in_us(got, x, taps, ratio=1, offset=None):
    """(max |got - definition| / (u S), the definition): elementwise, S = |taps| correlated with |x|."""
    from tmdiff_amd import metrics
    x, taps = np.asarray(x, dtype=np.float64), np.asarray(taps, dtype=np.float64)
    want = metrics.fir_decimate(x, taps, ratio, offset)
    scale = metrics.fir_decimate(np.abs(x), np.abs(taps), ratio, offset)
    assert scale.min() > 0.0
    return float((np.abs(np.asarray(got, dtype=np.float64) - want) / (U * scale)).max()), want


def fir_four_loops(x, taps, ratio, oy, ox):
    """The definition written out, one output pixel and one tap at a time."""
    x, taps = np.asarray(x, dtype=np.float64), np.asarray(taps, dtype=np.float64)
    planes, h, w = x.shape
    t, k = taps.shape[:2]
    rad = (k - 1) // 2
    ho, wo = len(range(oy, h, ratio)), len(range(ox, w, ratio))
    y = np.zeros((planes, ho, wo))
    for p in range(planes):
        for i in range(ho):
            for j in range(wo):
                for u in range(k):
                    for v in range(k):
                        yy = min(max(ratio * i + oy - rad + u, 0), h - 1)
                        xx = min(max(ratio * j + ox - rad + v, 0), w - 1)
                        y[p, i, j] += taps[p % t, u, v] * x[p, yy, xx]
    return y


# gnyq, ratio -> alpha, h[20, 20], h[20, 21] at n = 41
KERNEL_TABLE = [(0.3, 4, 3.2221567797876807, 0.0388555507617376, 0.03439065516710319),
                (0.15, 4, 2.566892062190515, 0.024676649096210986, 0.02283592652096944),
                (0.34, 2, 6.807890919616176, 0.17239244844459312, 0.10069147763341763)]


@pytest.mark.parametrize("gnyq,ratio,alpha,centre,beside", KERNEL_TABLE)
def test_mtf_kernel_values_and_properties(gnyq, ratio, alpha, centre, beside):
    from tmdiff_amd import metrics
    h = metrics.mtf_kernel(gnyq, ratio)
    assert h.shape == (41, 41) and h.dtype == np.float64
    assert abs(math.sqrt((40 * (1.0 / ratio) / 2.0) ** 2 / (-2.0 * math.log(gnyq))) / alpha - 1.0) <= 1e-12
    assert abs(h[20, 20] / centre - 1.0) <= 1e-12 and abs(h[20, 21] / beside - 1.0) <= 1e-12
    assert abs(h.sum() - 1.0) <= 1e-15
    assert np.abs(h - h.T).max() <= 1e-16 and np.abs(h - h[::-1]).max() <= 1e-16 and np.abs(h - h[:, ::-1]).max() <= 1e-16
    assert np.count_nonzero(h) == 1257               # the window's disc
    gain = float((h * np.cos(np.pi * (np.arange(41) - 20) / ratio)[None, :]).sum())
    print(f"mtf_kernel({gnyq}, {ratio}): realised Nyquist gain {gain:.8f}, least tap {h.min():.3e}")
    assert gain < gnyq                               # the window lowers it; it is not corrected
    if (gnyq, ratio) == (0.3, 4):
        assert abs(gain - 0.28270711) <= 5e-9
    if (gnyq, ratio) == (0.34, 2):
        assert -1.6e-4 < h.min() < -1.4e-4           # negative outer taps
    assert np.array_equal(metrics.mtf_kernel(gnyq, ratio, n=41), h) and metrics.mtf_kernel(gnyq, ratio, n=7).shape == (7, 7)
    for bad in (dict(gnyq=0.0), dict(gnyq=1.0), dict(n=40), dict(ratio=0)):
        with pytest.raises(ValueError):
            metrics.mtf_kernel(**{**dict(gnyq=gnyq, ratio=ratio), **bad})


def test_mtf_gains_table():
    from tmdiff_amd.metrics import band_gains, mtf_gains
    assert mtf_gains("QB") == ((0.34, 0.32, 0.30, 0.22), 0.15)
    assert mtf_gains("IKONOS") == ((0.26, 0.28, 0.29, 0.28), 0.17)
    assert mtf_gains("GeoEye1") == ((0.23,) * 4, 0.16)
    assert mtf_gains("WV2") == ((0.35,) * 7 + (0.27,), 0.11)
    assert mtf_gains("WV3", 8) == ((0.325, 0.355, 0.360, 0.350, 0.365, 0.360, 0.335, 0.315), 0.14)
    for name, bands in (("GF2", 4), ("WV4", 4), ("none", 8), ("anything", 3)):
        assert mtf_gains(name, bands) == ((0.29,) * bands, 0.15)
    assert mtf_gains(([0.3, 0.25], 0.2)) == ((0.3, 0.25), 0.2) and mtf_gains(((0.3, 0.25), 0.2), 2) == ((0.3, 0.25), 0.2)
    for sensor, bands in (("QB", 8), ("WV3", 4), ("WV2", 4), (((0.3, 0.25), 0.2), 3)):       # never broadcast
        with pytest.raises(ValueError, match="bands"):
            mtf_gains(sensor, bands)
    for bad in ("GF2", 0.3, ((0.3, 1.5), 0.2), ((0.3,), 0.0)):
        with pytest.raises(ValueError):
            mtf_gains(bad)
    assert band_gains("QB", 1, pan=True) == (0.15,) and band_gains(0.3, 3) == (0.3,) * 3 and band_gains([0.2, 0.3], 2) == (0.2, 0.3)
    with pytest.raises(ValueError):
        band_gains([0.2, 0.3], 3)
    with pytest.raises(ValueError):
        band_gains("QB", 3)


@pytest.mark.parametrize("ratio", (1, 2, 4))
@pytest.mark.parametrize("k", (1, 3, 5))
def test_fir_decimate_against_four_loops(ratio, k):
    from tmdiff_amd import metrics
    g = np.random.default_rng(10 * k + ratio)
    x = g.standard_normal((2, 3, 6, 9))                      # neither extent a multiple of 4; below the radius of K = 5 at the edges
    for t in (3, 1, 6):
        taps = g.standard_normal((t, k, k))
        for oy in range(ratio):
            for ox in range(ratio):
                got = metrics.fir_decimate(x, taps, ratio, (oy, ox))
                want = fir_four_loops(x.reshape(6, 6, 9), taps, ratio, oy, ox)
                assert got.shape == (2, 3, -(-(6 - oy) // ratio), -(-(9 - ox) // ratio)) and got.dtype == np.float64
                assert np.abs(got.reshape(want.shape) - want).max() <= 1e-13
    # the default offset: ratio // 2 on both axes; a number serves both axes; a [K, K] table is a period of 1
    taps = g.standard_normal((k, k))
    assert np.array_equal(metrics.fir_decimate(x, taps, ratio), metrics.fir_decimate(x, taps[None], ratio, (ratio // 2, ratio // 2)))
    assert np.array_equal(metrics.fir_decimate(x, taps, ratio, ratio - 1), metrics.fir_decimate(x, taps, ratio, (ratio - 1, ratio - 1)))
    assert np.array_equal(metrics.fir_decimate(torch.from_numpy(x), torch.from_numpy(taps), ratio), metrics.fir_decimate(x, taps, ratio))
    assert np.array_equal(metrics.fir_decimate(x[0, 1], taps, ratio), metrics.fir_decimate(x, taps, ratio)[0, 1])


@pytest.mark.parametrize("ratio", (1, 2, 4))
def test_fir_decimate_delta_and_extents(ratio):
    from tmdiff_amd import metrics
    x = np.random.default_rng(ratio).standard_normal((3, 7, 11))
    for k in (1, 5, 41):
        delta = np.zeros((k, k))
        delta[k // 2, k // 2] = 1.0
        for oy in range(ratio):
            for ox in range(ratio):
                got = metrics.fir_decimate(x, delta, ratio, (oy, ox))
                assert np.array_equal(got, x[..., oy::ratio, ox::ratio])
                assert got.shape[-2:] == (math.ceil((7 - oy) / ratio), math.ceil((11 - ox) / ratio)) == \
                    metrics.fir_decimate_shape(7, 11, ratio, (oy, ox))[0]
    # an extent that does not reach the offset leaves no sample
    if ratio == 4:
        assert metrics.fir_decimate(x[:, :2, :3], delta, 4).shape == (3, 0, 1) and metrics.fir_decimate(x[:, :1, :1], delta, 4, (1, 3)).shape == (3, 0, 0)
        assert metrics.fir_decimate(x[:, :3, :3], delta, 4, (2, 3)).shape == (3, 1, 0)
    # an off-centre delta shifts, with the border replicated: tap (u, v) reads x[i - R + u, j - R + v]
    shift = np.zeros((3, 3))
    shift[0, 2] = 1.0
    want = np.pad(x, ((0, 0), (1, 0), (0, 1)), mode="edge")[:, :-1, 1:]
    assert np.array_equal(metrics.fir_decimate(x, shift), want)
    for bad in (dict(offset=ratio), dict(offset=(0, -1)), dict(ratio=0)):
        with pytest.raises(ValueError):
            metrics.fir_decimate(x, shift, **{**dict(ratio=ratio), **bad})
    for taps in (np.zeros((2, 2)), np.zeros((2, 3, 3)), np.zeros((3, 3, 5)), np.zeros(3)):
        with pytest.raises(ValueError):
            metrics.fir_decimate(x, taps)


def test_mtf_degrade_is_fir_decimate_with_the_band_kernels():
    from tmdiff_amd import metrics
    x = np.random.default_rng(5).random((2, 4, 12, 16))
    got = metrics.mtf_degrade(x, "QB", 4)
    assert got.shape == (2, 4, 3, 4)
    for c, g in enumerate((0.34, 0.32, 0.30, 0.22)):
        assert np.array_equal(got[:, c], metrics.fir_decimate(x[:, c], metrics.mtf_kernel(g, 4), 4, (2, 2)))
    assert np.array_equal(metrics.mtf_degrade(x, (0.34, 0.32, 0.30, 0.22)), got)
    assert np.array_equal(metrics.mtf_degrade(x[:, :1], "QB", 4, pan=True), metrics.mtf_degrade(x[:, :1], 0.15, 4))
    assert metrics.mtf_degrade(x, 0.34, 2).shape == (2, 4, 6, 8)
    with pytest.raises(ValueError):
        metrics.mtf_degrade(x, "WV3")                        # 8 gains, 4 bands


def test_wald_pair_host_path():
    from tmdiff_amd import metrics
    from tmdiff_amd.data import wald_pair
    g = torch.Generator().manual_seed(8)
    ms, pan = torch.rand(2, 4, 8, 12, generator=g), torch.rand(2, 1, 32, 48, generator=g)
    pair = wald_pair(ms, pan, "QB")
    assert set(pair) == {"LR", "PAN", "MS", "HR", "Res"}
    assert {k: tuple(v.shape) for k, v in pair.items()} == {"LR": (2, 4, 2, 3), "PAN": (2, 1, 8, 12), "MS": (2, 4, 8, 12),
                                                            "HR": (2, 4, 8, 12), "Res": (2, 4, 8, 12)}
    assert all(v.dtype == torch.float64 for v in pair.values())
    assert torch.equal(pair["HR"], ms.double()) and torch.equal(pair["Res"], pair["HR"] - pair["MS"])
    assert np.array_equal(pair["LR"].numpy(), metrics.mtf_degrade(ms, "QB", 4))
    assert np.array_equal(pair["PAN"].numpy(), metrics.mtf_degrade(pan, "QB", 4, pan=True))
    assert np.array_equal(pair["MS"].numpy(), metrics.upsample_poly23(pair["LR"], 4))
    assert torch.equal(pair["MS"][..., 2::4, 2::4], pair["LR"])                       # registered to the interpolator's grid
    # a constant image stays that constant; explicit gains; ratio 2
    flat = wald_pair(torch.full((1, 4, 8, 8), 0.375), torch.full((1, 1, 32, 32), 0.625), "QB")
    assert float((flat["LR"] - 0.375).abs().max()) <= 1e-12 and float((flat["PAN"] - 0.625).abs().max()) <= 1e-12
    assert torch.equal(wald_pair(ms, pan, ((0.34, 0.32, 0.30, 0.22), 0.15))["LR"], pair["LR"])
    half = wald_pair(ms, pan[..., ::2, ::2], "GF2", ratio=2)
    assert tuple(half["LR"].shape) == (2, 4, 4, 6) and tuple(half["PAN"].shape) == (2, 1, 8, 12)
    assert torch.equal(half["MS"][..., 1::2, 1::2], half["LR"])
    for bad in (lambda: wald_pair(ms, pan, "WV3"), lambda: wald_pair(ms[..., :7, :], pan[..., :28, :], "QB"),
                lambda: wald_pair(ms, pan[..., ::2, ::2], "QB"), lambda: wald_pair(ms, pan, "QB", ratio=3)):
        with pytest.raises(ValueError):
            bad()


def test_float32_restatement_error():
    """What float32 costs in the kernel's summation order, which sets the GPU test's tolerance (4 x, rounded up)."""
    from tmdiff_amd import metrics
    worst = {k: 0.0 for k in RESTATEMENT_U}
    for h, w in MTF_GPU_SHAPES:
        x = mtf_input(h, w).numpy()
        for k in MTF_KS:
            for t in MTF_PERIODS:
                taps = mtf_taps(t, k).numpy()
                err, _ = error_in_us(fir_float32(x, taps), x, taps)
                worst[k] = max(worst[k], err)
    for name, sensor, ratio, pan, shape in MTF_REAL_CASES:
        x = mtf_real_input(shape).numpy()
        taps = np.stack([metrics.mtf_kernel(g, ratio) for g in metrics.band_gains(sensor, shape[1], pan)])
        err, want = error_in_us(fir_float32(x, taps, ratio), x, taps, ratio)          # float32 taps against the float64 ones
        assert np.array_equal(want, metrics.mtf_degrade(x, sensor, ratio, pan))
        print(f"float32 restatement, {name}: {err:.3f} u S")
        worst["mtf"] = max(worst["mtf"], err)
    print(f"float32 restatement, worst in u S: {worst}")
    for k, figure in RESTATEMENT_U.items():
        bound = apriori_u(41 if k == "mtf" else k)
        assert worst[k] <= figure <= bound and figure <= gpu_tol_u(k) <= bound
    assert [gpu_tol_u(k) for k in (7, 41, "mtf")] == [19.0, 21.0, 183.0] and gpu_tol_u(1) == apriori_u(1) and gpu_tol_u(3) == apriori_u(3)
    # a pixel's sum does not depend on the ratio or the offset: the restatement at (ratio, offset) is the ratio-1 result sliced
    x, taps = mtf_input(40, 24).numpy(), mtf_taps(3, 7).numpy()
    full = fir_float32(x, taps)
    for ratio, offsets in MTF_OFFSETS.items():
        for oy, ox in offsets:
            assert np.array_equal(fir_float32(x, taps, ratio, (oy, ox)), full[..., oy::ratio, ox::ratio])
    # and in exact arithmetic (integer taps and images, every partial sum below 2^24) it equals the definition
    xi, ti = mtf_input(40, 24, integer=True).numpy(), mtf_taps(3, 41, integer=True).numpy()
    assert np.array_equal(fir_float32(xi, ti, 4).astype(np.float64), metrics.fir_decimate(xi, ti, 4))


def test_entry_point_is_declared_exported_and_bound():
    import ctypes
    import os
    import re
    from conftest import ROOT
    from tmdiff_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmdiff_hip.h")).read(), flags=re.S)
    name = "tmdiff_fir_decimate"
    assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in include/tmdiff_hip.h"
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and len(_lib.SIGNATURES[name][1]) == 12
    assert _lib.ABI_VERSION == 6


def test_entry_point_refuses_what_it_does_not_take():
    """Argument checks come before any launch and before the null-pointer check, so they run without a GPU.  Order: K, ratio,
    offsets, extents, the tap period, the 32-bit limit."""
    from tmdiff_amd import _lib
    lib = _lib.lib
    msg = lambda: lib.tmdiff_last_error_string().decode()

    def fir(planes=6, period=3, h=8, w=8, k=41, ratio=4, oy=2, ox=2):
        return lib.tmdiff_fir_decimate(None, None, None, planes, period, h, w, k, ratio, oy, ox, None)

    for k in (0, -1, 2, 40, 43):
        assert fir(k=k) == -2 and f"K={k}" in msg()
    for ratio in (0, 3, 8, -2):
        assert fir(ratio=ratio) == -2 and f"ratio={ratio} " in msg()
    for oy, ox in ((4, 0), (0, 4), (-1, 0), (0, -1)):
        assert fir(oy=oy, ox=ox) == -2 and "offset" in msg()
    assert fir(ratio=2, oy=2, ox=0) == -2 and "offset" in msg() and fir(ratio=1, oy=0, ox=1) == -2 and "offset" in msg()
    for kw in (dict(h=0), dict(w=0), dict(h=-3), dict(planes=-3)):
        assert fir(**kw) == -2 and "extents" in msg()
    for kw in (dict(period=0), dict(period=-1), dict(period=4), dict(planes=3, period=6)):
        assert fir(**kw) == -2 and "taps_period=" in msg()
    assert fir(planes=8, period=8, h=16384, w=16384) == -2 and "exceeds" in msg()
    assert fir(planes=2, period=1, h=32768, w=32768) == -2 and "exceeds" in msg()
    # the order: each call breaks one rule and every later one
    assert fir(k=2, ratio=3, oy=9, h=0, period=0) == -2 and "K=2" in msg()
    assert fir(ratio=3, oy=9, h=0, period=0) == -2 and "ratio=3 " in msg()
    assert fir(oy=9, h=0, period=0) == -2 and "offset" in msg()
    assert fir(h=0, period=0) == -2 and "extents" in msg()
    assert fir(planes=7, period=2, h=32768, w=32768) == -2 and "taps_period=" in msg()
    # nothing to do; then the null check
    assert fir(planes=0) == 0 and fir(planes=0, period=5, k=1, ratio=1, oy=0, ox=0) == 0
    assert fir(h=2) == 0 and fir(w=1, ox=1) == 0             # no sample at o + ratio * i inside the image
    assert fir() == -1 and "null" in msg()
    assert fir(planes=1, period=1, h=1, w=1, k=1, ratio=1, oy=0, ox=0) == -1 and "null" in msg()


def test_ops_refuses_before_the_library_is_called():
    from tmdiff_amd import ops
    x, taps = torch.zeros(1, 3, 8, 8), torch.zeros(3, 3, 3)
    with pytest.raises(ValueError):
        ops.fir_decimate(x, taps)                                    # host tensors
    with pytest.raises(ValueError):
        ops.mtf_degrade(x, 0.3)
    with pytest.raises(ValueError):
        ops.mtf_degrade(x, "QB", pan=True)
    for bad in (dict(ratio=3), dict(ratio=8)):
        with pytest.raises(ValueError, match="ratio"):
            ops.fir_decimate(x, taps, **bad)
        with pytest.raises(ValueError):
            ops.mtf_degrade(x, 0.3, **bad)
    assert ops.fir_decimate_shape(67, 131, 4, None) == (17, 33) and ops.fir_decimate_shape(67, 131, 4, (3, 0)) == (16, 33)
    assert ops.fir_decimate_shape(8, 8, 1, None) == (8, 8) and ops.fir_decimate_shape(7, 7, 2, 1) == (3, 3)
    with pytest.raises(ValueError):
        ops.fir_decimate_shape(8, 8, 4, 4)


def test_dataset_reduces_a_raw_scene():
    from tmdiff_amd import metrics
    from tmdiff_amd.data import LRHRDataset, create_dataset
    g = np.random.default_rng(0)
    raw = {"ms": g.integers(0, 2047, (2, 4, 8, 12)).astype(np.float64), "pan": g.integers(0, 2047, (2, 1, 32, 48)).astype(np.float64)}
    ds = LRHRDataset(raw, reduce="QB")
    assert ds.has_gt is True and len(ds) == 2
    ms32, pan32 = (raw["ms"] / 2047.0).astype(np.float32), (raw["pan"] / 2047.0).astype(np.float32)
    lr, low_pan = metrics.mtf_degrade(ms32, "QB", 4), metrics.mtf_degrade(pan32, "QB", 4, pan=True)
    for i in range(2):
        item = ds[i]
        assert {k: (tuple(v.shape), v.dtype) for k, v in item.items()} == {
            "LR": ((4, 2, 3), torch.float32), "PAN": ((1, 8, 12), torch.float32), "MS": ((4, 8, 12), torch.float32),
            "HR": ((4, 8, 12), torch.float32), "Res": ((4, 8, 12), torch.float32)}
        assert torch.equal(item["HR"], torch.from_numpy(ms32[i])) and torch.equal(item["Res"], item["HR"] - item["MS"])
        assert torch.equal(item["MS"][:, 2::4, 2::4], item["LR"])
        # float32 on either path (the host definitions here, the device operators where there is a GPU)
        assert np.abs(item["LR"].double().numpy() - lr[i]).max() <= 1e-5 and np.abs(item["PAN"].double().numpy() - low_pan[i]).max() <= 1e-5
    # the option key; without `reduce` the same mapping is the full-resolution set it was before
    assert torch.equal(create_dataset({"dataroot": raw, "data_len": -1, "reduce": "QB"}, "train")[1]["LR"], ds[1]["LR"])
    for plain in (LRHRDataset(raw), create_dataset({"dataroot": raw, "data_len": -1}, "val")):
        assert plain.has_gt is False and len(plain) == 2
        item = plain[1]
        assert torch.equal(item["LR"], torch.from_numpy(ms32[1])) and torch.equal(item["PAN"], torch.from_numpy(pan32[1]))
        assert torch.equal(item["MS"], torch.from_numpy(metrics.upsample_poly23(ms32[1], 4)).float()) and torch.equal(item["HR"], item["MS"])
    # a file with a ground truth or an lms of its own is not reduced
    lms = g.integers(0, 2047, (2, 4, 32, 48)).astype(np.float64)
    kept = LRHRDataset({**raw, "lms": lms}, reduce="QB")
    assert kept.has_gt is False and torch.equal(kept[0]["MS"], torch.from_numpy(lms[0].astype(np.float32) / 2047.0))
    assert torch.equal(kept[0]["LR"], torch.from_numpy(ms32[0]))
