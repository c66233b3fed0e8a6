"""CPU-only tests of the adjoint of MTF-matched filtering and decimation: the float64 host definitions
``metrics.fir_decimate_adjoint`` / ``metrics.mtf_degrade_adjoint`` (the exact transpose of ``metrics.fir_decimate``, the
replicated border included), ``metrics.mtf_opnorm2`` and ``tiling.consistency_refine`` on host tensors, and the argument checks.

The definition is held to the transpose identity <A x, g> == <x, A^T g> and, at two small shapes, to the dense matrix of
``metrics.fir_decimate`` built column by column from unit images.

The file also holds what the GPU test (tests/test_gpu_mtf_adjoint.py) is measured against: its cases and a float32 restatement
of the kernel's summation order (``adjoint_float32``: acc = 0, then the terms of a pixel in lexicographic order of (i, u, j, v),
one fused multiply-add each), whose error against the float64 definition sets that test's working bound.  Errors are
elementwise, in units of u S with u = 2^-24 and S = the adjoint of |g| under |taps| at the same pixel.  Measured here over
the GPU test's cases, randn taps and g, both tap periods:
    K = 1: 0.991   K = 3: 3.122   K = 7: 3.841   K = 41: 4.578   the real MTF kernels (float64 taps rounded to float32): 72.480
(randn terms cancel; the all-positive MTF taps on an all-positive g do not, and a corner pixel of a 48 x 48 image at x4 folds
60^2 = 3600 of them into one chain).  The GPU test allows 4 x the figure, rounded up (the margin is for the restatement's emulated fused multiply-add), and never more than
the a-priori bound (n + 1) u / (1 - (n + 1) u) S, n the largest number of terms of a pixel at that shape, which holds for any
order and covers the rounding of the taps to float32."""
import numpy as np
import pytest
import torch

from test_mtf_host import MTF_KS, MTF_OFFSETS, U

# (H, W) of the small cases: two ragged shapes, one below the radius of every K > 7 (everything folds), and 3 x 2, which at x4 with
# offset 3 has no sample; every K, ratio and offset runs on them.  The GPU test adds 40 x 24 (more than one tile along one
# axis at x1 and x2, a ragged edge along the other) and 70 x 70 at x4 with K = 41: an interior 64 x 64 tile, all four borders and corners
ADJ_SHAPES = [(9, 13), (24, 24), (5, 7), (3, 2)]
ADJ_GPU_EXTRA = [(40, 24)]
ADJ_BIG = (70, 70, 41, 4, (2, 2))
ADJ_PERIODS = (3, 1)                      # 2 x 3 planes: a table per band, one table for all
ALL_OFFSETS = {r: [(a, b) for a in range(r) for b in range(r)] for r in (1, 2, 4)}
# worst error of adjoint_float32 against the definition in u S, as test_float32_restatement_error measures it (and holds it to)
ADJ_RESTATEMENT_U = {1: 0.991, 3: 3.122, 7: 3.841, 41: 4.578, "mtf": 72.480}
ADJ_REAL_CASES = [("QB", "QB", 4, (2, 4, 48, 48)), ("WV3 x2", "WV3", 2, (1, 8, 40, 24))]


def adj_cases(shapes):
    """(h, w, k, ratio, offset) over ``shapes``: every K, and per ratio the diagonal of offsets plus one pair off it."""
    return [(h, w, k, r, off) for h, w in shapes for k in MTF_KS for r, offs in MTF_OFFSETS.items() for off in offs]


def adj_taps(t, k, integer=False):
    g = torch.Generator().manual_seed(43 * k + t)
    return torch.randint(-3, 4, (t, k, k), generator=g).float() if integer else torch.randn(t, k, k, generator=g)


def adj_g(h, w, ratio, offset, integer=False, planes=(2, 3)):
    from tmdiff_amd.metrics import fir_decimate_shape
    (ho, wo), (oy, ox) = fir_decimate_shape(h, w, ratio, offset)
    g = torch.Generator().manual_seed(7000 + 1000 * ratio + 100 * oy + 10 * ox + 31 * h + w)
    return torch.randint(-8, 9, (*planes, ho, wo), generator=g).float() if integer else torch.randn(*planes, ho, wo, generator=g)


def term_count(h, w, k, ratio, offset):
    """The largest number of terms of a pixel: the adjoint of ones under ones."""
    from tmdiff_amd import metrics
    (ho, wo), _ = metrics.fir_decimate_shape(h, w, ratio, offset)
    return int(metrics.fir_decimate_adjoint(np.ones((ho, wo)), np.ones((k, k)), (h, w), ratio, offset).max())


def apriori_adj_u(n):
    """The elementwise a-priori bound in u S for n terms: (n + 1) u / (1 - (n + 1) u), over u."""
    return (n + 1) / (1.0 - (n + 1) * U)


def adj_tol_u(k, n):
    """The GPU test's tolerance in u S: 4 x the restatement's figure, rounded up, never above the a-priori bound for n terms."""
    return min(float(np.ceil(4.0 * ADJ_RESTATEMENT_U[k])), apriori_adj_u(n))


def adjoint_float32(g, taps, shape, ratio=1, offset=None):
    """The kernel's arithmetic in float32 on the host: per pixel acc = 0, then acc = fma(taps[u][v], g[i][j], acc) over the
    pixel's terms in lexicographic order of (i, u, j, v) (a fused multiply-add is the float64 product, which is exact, plus acc,
    rounded to float64 and once more to float32).  All terms are listed in that order, sorted by pixel (stably), and step s
    applies the s-th term of every pixel that has one."""
    from tmdiff_amd.metrics import fir_decimate_shape
    g = np.asarray(g, dtype=np.float32)
    taps = np.asarray(taps, dtype=np.float32)
    taps = taps[None] if taps.ndim == 2 else taps
    h, w = shape
    (ho, wo), (oy, ox) = fir_decimate_shape(h, w, ratio, offset)
    planes, (t, k) = int(np.prod(g.shape[:-2])), taps.shape[:2]
    acc = np.zeros((planes, h * w), dtype=np.float32)
    if ho * wo:
        gp = g.reshape(planes, ho * wo).astype(np.float64)
        band = np.tile(taps, (planes // t, 1, 1)).reshape(planes, k * k).astype(np.float64)
        i, u, j, v = (a.ravel() for a in np.meshgrid(np.arange(ho), np.arange(k), np.arange(wo), np.arange(k), indexing="ij"))
        pix = np.clip(ratio * i + oy - k // 2 + u, 0, h - 1) * w + np.clip(ratio * j + ox - k // 2 + v, 0, w - 1)
        order = np.argsort(pix, kind="stable")
        pix, gi, ti = pix[order], (i * wo + j)[order], (u * k + v)[order]
        first = np.searchsorted(pix, pix, side="left")
        rank = np.arange(pix.size) - first
        by_rank = np.argsort(rank, kind="stable")
        bounds = np.searchsorted(rank[by_rank], np.arange(rank.max() + 2))
        for s in range(rank.max() + 1):
            sel = by_rank[bounds[s]:bounds[s + 1]]
            p = pix[sel]
            acc[:, p] = (band[:, ti[sel]] * gp[:, gi[sel]] + acc[:, p].astype(np.float64)).astype(np.float32)
    return acc.reshape(g.shape[:-2] + (h, w))


def adj_error_in_us(got, g, taps, shape, ratio=1, offset=None):
    """(max |got - definition| / (u S) over the pixels with S > 0, the definition); where S == 0 the pixel must be 0."""
    from tmdiff_amd import metrics
    g, taps = np.asarray(g, dtype=np.float64), np.asarray(taps, dtype=np.float64)
    want = metrics.fir_decimate_adjoint(g, taps, shape, ratio, offset)
    scale = metrics.fir_decimate_adjoint(np.abs(g), np.abs(taps), shape, ratio, offset)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape
    assert not got[scale == 0.0].any()
    live = scale > 0.0
    return (float((np.abs(got - want)[live] / (U * scale[live])).max()) if live.any() else 0.0), want


@pytest.mark.parametrize("h,w", ADJ_SHAPES)
def test_transpose_identity(h, w):
    from tmdiff_amd import metrics
    rng = np.random.default_rng(100 * h + w)
    for k in MTF_KS:
        for ratio, offsets in ALL_OFFSETS.items():
            for off in offsets:
                for t in ADJ_PERIODS:
                    x, taps = rng.standard_normal((2, 3, h, w)), rng.standard_normal((t, k, k))
                    y = metrics.fir_decimate(x, taps, ratio, off)
                    g = rng.standard_normal(y.shape)
                    dx = metrics.fir_decimate_adjoint(g, taps, (h, w), ratio, off)
                    assert dx.shape == x.shape and dx.dtype == np.float64
                    lhs, rhs = float((y * g).sum()), float((x * dx).sum())
                    size = float(np.abs(y * g).sum() + np.abs(x * dx).sum())
                    assert abs(lhs - rhs) <= 1e-12 * max(size, 1e-300), (k, ratio, off, t, lhs, rhs)
                    if y.size == 0:
                        assert not dx.any()


def test_empty_output_has_a_zero_gradient():
    from tmdiff_amd import metrics
    taps = np.random.default_rng(1).standard_normal((3, 3))
    assert metrics.fir_decimate_shape(3, 2, 4, 3)[0] == (0, 0)
    dx = metrics.fir_decimate_adjoint(np.zeros((2, 0, 0)), taps, (3, 2), 4, 3)
    assert dx.shape == (2, 3, 2) and not dx.any()
    assert metrics.fir_decimate_shape(3, 9, 4, 3)[0] == (0, 2)          # one axis without a sample is enough
    assert not metrics.fir_decimate_adjoint(np.ones((0, 2)), taps, (3, 9), 4, 3).any()


@pytest.mark.parametrize("h,w", [(9, 13), (12, 8)])
def test_dense_matrix(h, w):
    """A column by column from unit images through ``metrics.fir_decimate``; A.T @ g is the adjoint."""
    from tmdiff_amd import metrics
    rng = np.random.default_rng(h)
    for k, ratio, off in ((7, 4, (1, 3)), (41, 2, None), (3, 1, None), (41, 4, None), (7, 2, (0, 1))):
        taps = rng.standard_normal((k, k))
        a = np.stack([metrics.fir_decimate(e.reshape(h, w), taps, ratio, off).ravel() for e in np.eye(h * w)], axis=1)
        ho, wo = metrics.fir_decimate_shape(h, w, ratio, off)[0]
        g = rng.standard_normal((ho, wo))
        want = (a.T @ g.ravel()).reshape(h, w)
        got = metrics.fir_decimate_adjoint(g, taps, (h, w), ratio, off)
        assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max()), (k, ratio, off)


def test_mtf_degrade_adjoint_is_the_transpose():
    from tmdiff_amd import metrics
    rng = np.random.default_rng(5)
    for sensor, ratio, pan, bands in (("QB", 4, False, 4), ("WV3", 2, False, 8), ("QB", 4, True, 1)):
        x = rng.standard_normal((2, bands, 24, 20))
        y = metrics.mtf_degrade(x, sensor, ratio, pan)
        g = rng.standard_normal(y.shape)
        dx = metrics.mtf_degrade_adjoint(g, sensor, (24, 20), ratio, pan)
        assert dx.shape == x.shape
        assert abs(float((y * g).sum()) - float((x * dx).sum())) <= 1e-12 * float(np.abs(y * g).sum() + np.abs(x * dx).sum())


@pytest.mark.parametrize("ratio,lo,hi", [(4, 0.0769, 0.0813), (2, 0.344, 0.377)])
def test_mtf_opnorm2(ratio, lo, hi):
    from tmdiff_amd import metrics
    n = 24
    for gain in (0.15, 0.22, 0.365):
        taps = metrics.mtf_kernel(gain, ratio)
        a = np.stack([metrics.fir_decimate(e.reshape(n, n), taps, ratio).ravel() for e in np.eye(n * n)], axis=1)
        top = float(np.linalg.svd(a, compute_uv=False)[0]) ** 2
        got = metrics.mtf_opnorm2(gain, ratio)
        print(f"mtf_opnorm2({gain}, {ratio}) = {got:.6f}, dense 24 x 24: {top:.6f}")
        assert abs(got - top) <= 0.01 * top
        assert lo - 5e-5 <= got <= hi + 5e-5            # the probed range, quoted to four (x4) and three (x2) digits
        assert metrics.mtf_opnorm2(gain, ratio) is metrics._MTF_OPNORM2[(gain, ratio)]          # cached


def _refine_scene():
    from tmdiff_amd import metrics
    hr = np.random.default_rng(48).random((1, 4, 48, 48))
    lr = metrics.mtf_degrade(hr, "QB", 4)
    return lr, metrics.upsample_poly23(lr, 4)


def _residual_rms(f, lr, sensor="QB", ratio=4):
    from tmdiff_amd import metrics
    return float(np.sqrt(np.mean((metrics.mtf_degrade(f, sensor, ratio) - lr) ** 2)))


@pytest.mark.parametrize("relax", (0.5, 1.0, 1.9))
def test_consistency_refine_on_the_host(relax):
    from tmdiff_amd.tiling import consistency_refine
    lr, start = _refine_scene()
    rms = [_residual_rms(start, lr)]
    f = start
    for _ in range(8):
        f = consistency_refine(f, lr, "QB", 4, iters=1, relax=relax)
        rms.append(_residual_rms(f, lr))
    print(f"consistency_refine relax {relax}: residual RMS " + " ".join(f"{r:.6f}" for r in rms) + f" (end / start {rms[-1] / rms[0]:.4f})")
    assert all(b <= a for a, b in zip(rms, rms[1:]))
    # eight steps in one call are the eight calls
    assert np.array_equal(consistency_refine(start, lr, "QB", 4, iters=8, relax=relax), f)
    if relax == 1.0:
        assert rms[-1] < 0.90 * rms[0]


def test_consistency_refine_arguments():
    from tmdiff_amd.tiling import consistency_refine, fuse_scene
    lr, start = _refine_scene()
    same = consistency_refine(start, lr, "QB", 4, iters=0)
    assert np.array_equal(same, start)
    t = consistency_refine(torch.from_numpy(start), torch.from_numpy(lr), "QB", 4, iters=1)
    assert torch.is_tensor(t) and t.dtype == torch.float64 and np.array_equal(t.numpy(), consistency_refine(start, lr, "QB", 4, iters=1))
    for relax in (0.0, 2.0, -1.0, 2.5):
        with pytest.raises(ValueError):
            consistency_refine(start, lr, "QB", 4, relax=relax)
    with pytest.raises(ValueError):
        consistency_refine(start, lr, "QB", 4, iters=-1)
    with pytest.raises(ValueError):
        consistency_refine(start, lr[..., :-1], "QB", 4)              # not the degradation's extent
    with pytest.raises(ValueError):
        consistency_refine(start[:, :3], lr[:, :3], "QB", 4)           # 4 gains, 3 bands
    with pytest.raises(ValueError, match="sensor"):
        fuse_scene(None, torch.zeros(1, 4, 12, 12), torch.zeros(1, 1, 48, 48), "QB", consistency={"iters": 2})
    with pytest.raises(ValueError):
        fuse_scene(None, torch.zeros(1, 4, 12, 12), torch.zeros(1, 1, 48, 48), "QB", sensor="QB", consistency={"steps": 2})


def test_adjoint_argument_errors():
    from tmdiff_amd import metrics
    taps = np.ones((3, 3, 3))
    with pytest.raises(ValueError):
        metrics.fir_decimate_adjoint(np.zeros((3, 3, 4)), taps, (9, 13), 4)            # [2, 3] is the extent
    with pytest.raises(ValueError):
        metrics.fir_decimate_adjoint(np.zeros((3, 2, 3)), taps, (9, 13), 4, (0, 1))            # [3, 3] at this offset
    with pytest.raises(ValueError):
        metrics.fir_decimate_adjoint(np.zeros((4, 2, 3)), taps, (9, 13), 4)            # 3 tables, 4 planes
    with pytest.raises(ValueError):
        metrics.fir_decimate_adjoint(np.zeros((3, 2, 3)), np.ones((3, 4, 4)), (9, 13), 4)
    with pytest.raises(ValueError):
        metrics.fir_decimate_adjoint(np.zeros((3, 2, 3)), taps, (9, 13), 4, 4)         # offset >= ratio
    with pytest.raises(ValueError):
        metrics.fir_decimate_adjoint(np.zeros((3, 2, 3)), taps, (0, 13), 4)
    with pytest.raises(ValueError):
        metrics.mtf_degrade_adjoint(np.zeros((1, 3, 6, 6)), "QB", (24, 24), 4)         # 4 gains, 3 bands
    assert metrics.fir_decimate_adjoint(np.zeros((3, 2, 3)), taps, (9, 13), 4).shape == (3, 9, 13)


def test_c_entry_point_checks_its_arguments():
    """The limits are the forward's, in the forward's order, and nothing is launched: the pointers are never touched."""
    from tmdiff_amd._lib import lib

    def call(**kw):
        a = dict(planes=6, period=3, h=8, w=8, k=3, ratio=4, oy=2, ox=2)
        a.update(kw)
        return lib.tmdiff_fir_decimate_adjoint(None, None, None, None, 1.0, 0.0, a["planes"], a["period"], a["h"], a["w"], a["k"],
                                               a["ratio"], a["oy"], a["ox"], None)

    for bad, word in ((dict(k=4), "K=4"), (dict(k=43), "K=43"), (dict(ratio=3), "ratio=3"), (dict(oy=4), "offset"), (dict(ox=-1), "offset"),
                      (dict(h=0), "bad extents"), (dict(planes=-1), "bad extents"), (dict(period=4), "taps_period=4"),
                      (dict(period=0), "taps_period=0"), (dict(planes=3 * 2 ** 20, h=32, w=32), "32-bit")):
        assert call(**bad) == -2, bad
        msg = lib.tmdiff_last_error_string().decode()
        assert msg.startswith("fir_decimate_adjoint: ") and word in msg and "planes * H * W <= 2^31 - 1" in msg, msg
    assert call(planes=0) == 0
    assert call() == -1                       # null tensors
    assert "null tensor" in lib.tmdiff_last_error_string().decode()


def test_float32_restatement_error():
    """Measures the working bound of the GPU test: the kernel's summation order in float32 against the definition."""
    from tmdiff_amd import metrics
    worst = {k: 0.0 for k in MTF_KS}
    cases = adj_cases(ADJ_SHAPES + ADJ_GPU_EXTRA) + [ADJ_BIG]
    for h, w, k, ratio, off in cases:
        n = term_count(h, w, k, ratio, off)
        for t in ADJ_PERIODS:
            g, taps = adj_g(h, w, ratio, off), adj_taps(t, k)
            err, _ = adj_error_in_us(adjoint_float32(g, taps, (h, w), ratio, off), g, taps, (h, w), ratio, off)
            assert err <= apriori_adj_u(n), (h, w, k, ratio, off, err, n)
            worst[k] = max(worst[k], err)
    real = 0.0
    for name, sensor, ratio, shape in ADJ_REAL_CASES:
        taps = np.stack([metrics.mtf_kernel(gn, ratio) for gn in metrics.band_gains(sensor, shape[1])]).astype(np.float32)
        ho, wo = metrics.fir_decimate_shape(shape[2], shape[3], ratio)[0]
        g = torch.rand(*shape[:2], ho, wo, generator=torch.Generator().manual_seed(shape[1])).numpy()
        got = adjoint_float32(g, taps, shape[2:], ratio)
        want = metrics.mtf_degrade_adjoint(g, sensor, shape[2:], ratio)          # float64 taps: the rounding of the table counts
        scale = metrics.fir_decimate_adjoint(g, np.abs(taps), shape[2:], ratio)
        real = max(real, float((np.abs(got - want) / (U * scale)).max()))
    print("adjoint_float32, worst error in u S: " + "  ".join(f"K = {k}: {worst[k]:.3f}" for k in MTF_KS) + f"  MTF kernels: {real:.3f}")
    for k in MTF_KS:
        assert worst[k] <= ADJ_RESTATEMENT_U[k] + 5e-4, (k, worst[k])
    assert real <= ADJ_RESTATEMENT_U["mtf"] + 5e-4
