"""The adjoint of MTF-matched filtering and decimation on the GPU (csrc/mtf.hip: ``ops.fir_decimate_adjoint``,
``ops.mtf_degrade_adjoint``), the differentiable ``ops.fir_decimate`` / ``ops.mtf_degrade`` / ``data.wald_pair`` on top of it
(``autograd.FirDecimateFn``) and ``tiling.consistency_refine`` / ``fuse_scene(consistency=...)``.

Cases (tests/test_mtf_adjoint_host.py): 2 x 3 planes at 9 x 13, 24 x 24, 5 x 7 (below the radius: everything folds), 3 x 2 (no
sample at x4 with offset 3: a zero gradient) and 40 x 24 (several tiles along an axis at x1 and x2, a ragged one along the other)
with K in {1, 3, 7, 41}, ratio 1, 2, 4, the diagonal of offsets and one pair off it, a tap table per band and one for all; and
70 x 70 at x4 with K = 41: an interior 64 x 64 tile, all four borders and corners.

Exact arithmetic catches indexing errors: integer taps in [-3, 3] and integer g in [-8, 8] keep every partial sum below 2^24
(a 70 x 70 corner folds 55^2 = 3025 terms of at most 24), so the device must equal the float64 definition bit for bit.

Tolerance against ``metrics.fir_decimate_adjoint`` with randn taps and g, elementwise in units of u S, u = 2^-24, S = the adjoint
of |g| under |taps|: the a-priori bound (n + 1) u / (1 - (n + 1) u) S, n the largest number of terms of a pixel at that shape
(the adjoint of ones under ones), holds for any order; the working bound is 4 x what a float32 restatement of the kernel's
order measured on the CPU (``adjoint_float32``: 0.991 / 3.122 / 3.841 / 4.578 u S at K = 1 / 3 / 7 / 41, 72.480 for the real MTF
kernels), rounded up -- 4, 13, 16, 19 and 290 u S -- and never above the a-priori bound.

``consistency_refine`` on the device against the host run: the error is propagated elementwise through the 8 steps,
E' = E + |s A^T| (|A| E + e_r) + e_a, with the two operators' u S bounds (183 u S for the degradation, tests/test_mtf_host.py;
290 u S for the adjoint), the subtraction's and the epilogue's roundings, all computed in float64 from the host iterates with the
bound so far added to every magnitude (the device's values are within it), so no term of higher order is left out.

Everything else is bit for bit."""
import numpy as np
import pytest
import torch

from test_mtf_adjoint_host import (ADJ_BIG, ADJ_GPU_EXTRA, ADJ_PERIODS, ADJ_SHAPES, adj_cases, adj_g, adj_taps, adj_tol_u,
                                   apriori_adj_u, term_count)
from test_mtf_host import MTF_KS, U, gpu_tol_u

pytestmark = pytest.mark.gpu

SHAPES = ADJ_SHAPES + ADJ_GPU_EXTRA


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _cases(h, w, k):
    return [c for c in adj_cases([(h, w)]) if c[2] == k]


def _check_exact(h, w, k, ratio, off):
    from tmdiff_amd import metrics, ops
    for t in ADJ_PERIODS:
        g, taps = adj_g(h, w, ratio, off, integer=True), adj_taps(t, k, integer=True)
        want = metrics.fir_decimate_adjoint(g, taps, (h, w), ratio, off)
        assert metrics.fir_decimate_adjoint(g.abs(), taps.abs(), (h, w), ratio, off).max() < 2 ** 24
        got = ops.fir_decimate_adjoint(g.cuda(), taps.cuda(), (h, w), ratio, off)
        assert got.dtype == torch.float32 and tuple(got.shape) == want.shape == (2, 3, h, w)
        bad = int((got.cpu().double().numpy() != want).sum())
        assert bad == 0, f"{h} x {w} K={k} period {t} ratio {ratio} offset {off}: {bad} of {want.size} pixels differ"


def _check_tolerance(h, w, k, ratio, off):
    """The worst error in u S over both tap periods, held to the working and the a-priori bound."""
    from tmdiff_amd import metrics, ops
    n = term_count(h, w, k, ratio, off)
    tol = adj_tol_u(k, n)
    assert tol <= apriori_adj_u(n)
    worst = 0.0
    for t in ADJ_PERIODS:
        g, taps = adj_g(h, w, ratio, off), adj_taps(t, k)
        got = ops.fir_decimate_adjoint(g.cuda(), taps.cuda(), (h, w), ratio, off).cpu().double().numpy()
        want = metrics.fir_decimate_adjoint(g, taps, (h, w), ratio, off)
        scale = metrics.fir_decimate_adjoint(g.abs(), taps.abs(), (h, w), ratio, off)
        assert got.shape == want.shape and not got[scale == 0.0].any()
        if not (scale > 0.0).any():                # no sample: a zero gradient
            continue
        err = float((np.abs(got - want)[scale > 0.0] / (U * scale[scale > 0.0])).max())
        worst = max(worst, err)
        assert err <= tol, f"{h} x {w} K={k} period {t} ratio {ratio} offset {off}: {err:.3f} u S, tolerance {tol:.3f} (n = {n})"
    return worst, tol


@pytest.mark.parametrize("k", MTF_KS)
@pytest.mark.parametrize("h,w", SHAPES)
def test_adjoint_exact_arithmetic(h, w, k):
    for _, _, _, ratio, off in _cases(h, w, k):
        _check_exact(h, w, k, ratio, off)


@pytest.mark.parametrize("k", MTF_KS)
@pytest.mark.parametrize("h,w", SHAPES)
def test_adjoint_against_the_definition(h, w, k):
    worst = 0.0
    for _, _, _, ratio, off in _cases(h, w, k):
        worst = max(worst, _check_tolerance(h, w, k, ratio, off)[0])
    print(f"fir_decimate_adjoint {h} x {w} K={k}: worst error {worst:.3f} u S (working bound {adj_tol_u(k, 10 ** 6):.0f} u S)")


def test_adjoint_interior_tile_borders_and_corners():
    h, w, k, ratio, off = ADJ_BIG
    _check_exact(h, w, k, ratio, off)
    err, tol = _check_tolerance(h, w, k, ratio, off)
    print(f"fir_decimate_adjoint {h} x {w} K={k} x{ratio}: worst error {err:.3f} u S (tolerance {tol:.3f}, n = {term_count(h, w, k, ratio, off)})")


@pytest.mark.parametrize("name,sensor,ratio,shape", [("QB", "QB", 4, (2, 4, 48, 48)), ("WV3 x2", "WV3", 2, (1, 8, 40, 24))])
def test_mtf_degrade_adjoint_against_the_definition(name, sensor, ratio, shape):
    from tmdiff_amd import metrics, ops
    ho, wo = ops.fir_decimate_shape(shape[2], shape[3], ratio)
    g = torch.rand(*shape[:2], ho, wo, generator=torch.Generator().manual_seed(shape[1]))
    got = ops.mtf_degrade_adjoint(g.cuda(), sensor, shape[2:], ratio)
    want = metrics.mtf_degrade_adjoint(g, sensor, shape[2:], ratio)
    taps = np.stack([metrics.mtf_kernel(gn, ratio) for gn in metrics.band_gains(sensor, shape[1])])
    scale = metrics.fir_decimate_adjoint(g, np.abs(taps), shape[2:], ratio)
    n = term_count(shape[2], shape[3], 41, ratio, None)
    tol = adj_tol_u("mtf", n)
    err = float((np.abs(got.cpu().double().numpy() - want) / (U * scale)).max())
    print(f"mtf_degrade_adjoint {name} x{ratio} {shape}: {err:.3f} u S (tolerance {tol:.1f}, a-priori {apriori_adj_u(n):.1f})")
    assert tuple(got.shape) == shape and err <= tol <= apriori_adj_u(n)
    # the table is mtf_degrade's
    gains = metrics.band_gains(sensor, shape[1])
    table = ops._MTF_TAPS[(gains, ratio, torch.device("cuda", torch.cuda.current_device()))]
    assert _same(ops.fir_decimate_adjoint(g.cuda(), table, shape[2:], ratio), got)


@pytest.mark.parametrize("h,w,k,ratio,off", [(40, 24, 41, 4, None), (40, 24, 7, 2, (0, 1)), (9, 13, 41, 1, None), (70, 70, 41, 4, (2, 2)),
                                             (24, 24, 3, 4, (3, 3))])
def test_transpose_on_the_device(h, w, k, ratio, off):
    from tmdiff_amd import ops
    x = torch.randn(2, 3, h, w, generator=torch.Generator().manual_seed(h + w))
    g, taps = adj_g(h, w, ratio, off), adj_taps(3, k)
    y = ops.fir_decimate(x.cuda(), taps.cuda(), ratio, off).cpu().double()
    dx = ops.fir_decimate_adjoint(g.cuda(), taps.cuda(), (h, w), ratio, off).cpu().double()
    lhs, rhs = float((y * g.double()).sum()), float((x.double() * dx).sum())
    size = float((y * g.double()).abs().sum() + (x.double() * dx).abs().sum())
    print(f"<A x, g> - <x, A^T g> at {h} x {w} K={k} x{ratio}: {abs(lhs - rhs) / size / U:.3f} u of sum |.|")
    assert abs(lhs - rhs) <= 4 * (k * k + 1) * U * size


def test_epilogue():
    from tmdiff_amd import metrics, ops
    h, w, k, ratio = 40, 24, 7, 4
    n = term_count(h, w, k, ratio, None)
    for shape_hw, r in (((h, w), ratio), ((9, 13), 2), ((9, 13), 1)):          # 16-byte rows, 8-byte rows cut short, single dwords
        g, taps = adj_g(*shape_hw, r, None), adj_taps(3, k)
        base = torch.randn(2, 3, *shape_hw, generator=torch.Generator().manual_seed(9))
        adj = metrics.fir_decimate_adjoint(g, taps, shape_hw, r)
        scale = metrics.fir_decimate_adjoint(g.abs(), taps.abs(), shape_hw, r)
        gd, td, bd = g.cuda(), taps.cuda(), base.cuda()
        plain = ops.fir_decimate_adjoint(gd, td, shape_hw, r)
        for alpha, beta in ((1.0, 1.0), (-0.75, 0.5), (2.5, -1.25), (0.0, 3.0)):
            got = ops.fir_decimate_adjoint(gd, td, shape_hw, r, base=bd, alpha=alpha, beta=beta)
            want = beta * base.double().numpy() + alpha * adj
            # the chain's bound scaled by |alpha|, one rounding of alpha * acc and one of the fma
            bound = U * (abs(alpha) * (adj_tol_u(k, n) + 1) * scale + np.abs(want))
            assert (np.abs(got.cpu().double().numpy() - want) <= bound).all(), (shape_hw, r, alpha, beta)
            # base aliasing out: a lane reads base where it writes
            alias = bd.clone()
            assert ops.fir_decimate_adjoint(gd, td, shape_hw, r, out=alias, base=alias, alpha=alpha, beta=beta) is alias and _same(alias, got)
        # alpha = 1, beta = 0 is the plain call; beta = 0 never reads base
        nan = torch.full_like(bd, float("nan"))
        assert _same(ops.fir_decimate_adjoint(gd, td, shape_hw, r, base=nan, alpha=1.0, beta=0.0), plain)
        assert _same(ops.fir_decimate_adjoint(gd, td, shape_hw, r, out=nan, base=nan, alpha=1.0, beta=0.0), plain)
        out = torch.full_like(bd, float("nan"))
        assert ops.fir_decimate_adjoint(gd, td, shape_hw, r, out=out) is out and _same(out, plain)
        # one element off 16-byte alignment: the single-dword stores, the same values
        buf = torch.full((plain.numel() + 1,), float("nan"), device="cuda")
        off = buf[1:].view(plain.shape)
        assert ops.fir_decimate_adjoint(gd, td, shape_hw, r, out=off) is off and _same(off, plain)
    with pytest.raises(ValueError):
        ops.fir_decimate_adjoint(gd, td, shape_hw, r, beta=1.0)                       # beta without base
    with pytest.raises(ValueError):
        ops.fir_decimate_adjoint(gd, td, (10, 13), r)                                 # g is not the extent of 10 x 13
    with pytest.raises(ValueError):
        ops.fir_decimate_adjoint(gd, adj_taps(4, k).cuda(), shape_hw, r)              # 4 tables, 6 planes
    with pytest.raises(ValueError):
        ops.mtf_degrade_adjoint(torch.zeros(1, 3, 6, 6, device="cuda"), "QB", (24, 24))       # 4 gains, 3 bands
    # out may be base, never g (at ratio 1 it has the shape) or the taps: other tiles still read them
    with pytest.raises(ValueError, match="overlaps g"):
        ops.fir_decimate_adjoint(gd, td, shape_hw, 1, out=gd)
    with pytest.raises(ValueError, match="overlaps taps"):
        t1 = torch.zeros(6, 1, 1, device="cuda")
        ops.fir_decimate_adjoint(torch.zeros(1, 6, 1, 1, device="cuda"), t1, (1, 1), 1, out=t1.view(1, 6, 1, 1))


def test_planes_beyond_the_grid_and_batches():
    from tmdiff_amd import ops
    gen = torch.Generator().manual_seed(65537)
    planes = 65537                                                  # gridDim.y stops at 65535: the plane loop runs twice for two
    g, taps = torch.randn(1, planes, 2, 2, generator=gen).cuda(), torch.randn(3, 3, generator=gen).cuda()
    got = ops.fir_decimate_adjoint(g, taps, (4, 4), 2)
    half = 32768
    parts = [ops.fir_decimate_adjoint(g[:, lo:hi].contiguous(), taps, (4, 4), 2) for lo, hi in ((0, half), (half, planes))]
    assert _same(got, torch.cat(parts, 1))
    # a batch is its samples one at a time (plane p takes taps[p % 3])
    gb, tb = adj_g(40, 24, 4, None).cuda(), adj_taps(3, 41).cuda()
    full = ops.fir_decimate_adjoint(gb, tb, (40, 24), 4)
    for b in range(2):
        assert _same(ops.fir_decimate_adjoint(gb[b:b + 1].contiguous(), tb, (40, 24), 4), full[b:b + 1])


def test_determinism_and_graph_replay():
    from tmdiff_amd import ops
    h, w, k, ratio, off = ADJ_BIG
    g, taps = adj_g(h, w, ratio, off).cuda(), adj_taps(3, k).cuda()
    want = ops.fir_decimate_adjoint(g, taps, (h, w), ratio, off)
    assert _same(ops.fir_decimate_adjoint(g, taps, (h, w), ratio, off), want)
    src, out = torch.zeros_like(g), torch.zeros_like(want)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.fir_decimate_adjoint(src, taps, (h, w), ratio, off, out=out)               # warm-up on the capture stream
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):                                       # one stream: no parallel branches
        ops.fir_decimate_adjoint(src, taps, (h, w), ratio, off, out=out)
    src.copy_(g)
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert _same(out, want)


def test_autograd():
    from tmdiff_amd import ops
    from tmdiff_amd.data import wald_pair
    gen = torch.Generator().manual_seed(11)
    x = torch.rand(2, 4, 40, 24, generator=gen).cuda()
    g = torch.randn(2, 4, 10, 6, generator=gen).cuda()
    plain = ops.mtf_degrade(x, "QB")
    assert plain.grad_fn is None and not plain.requires_grad
    xr = x.clone().requires_grad_()
    y = ops.mtf_degrade(xr, "QB")
    assert y.grad_fn is not None and _same(y.detach(), plain)
    y.backward(g)
    assert _same(xr.grad, ops.mtf_degrade_adjoint(g, "QB", (40, 24)))
    with torch.no_grad():
        quiet = ops.mtf_degrade(xr, "QB")
        assert quiet.grad_fn is None and not quiet.requires_grad and _same(quiet, plain)
        out = torch.empty_like(plain)
        assert ops.mtf_degrade(xr, "QB", out=out) is out and _same(out, plain)          # out= is fine without grad mode
    with pytest.raises(ValueError, match="out="):
        ops.mtf_degrade(xr, "QB", out=torch.empty_like(plain))
    # fir_decimate with another ratio and offset; the taps get no gradient
    taps = adj_taps(1, 7).cuda().requires_grad_()
    xs = torch.randn(2, 3, 9, 13, generator=gen).cuda().requires_grad_()
    ys = ops.fir_decimate(xs, taps, 2, (0, 1))
    gs = torch.randn(ys.shape, generator=gen).cuda()
    ys.backward(gs)
    assert taps.grad is None and _same(xs.grad, ops.fir_decimate_adjoint(gs, taps.detach(), (9, 13), 2, (0, 1)))
    # the taps are saved for the backward: a table changed in place in between is reported, not used
    ys = ops.fir_decimate(xs, taps.detach(), 2, (0, 1))
    held = taps.detach().clone()
    yh = ops.fir_decimate(xs, held, 2, (0, 1))
    held.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        yh.backward(gs)
    # the backward is not differentiable again
    gx, = torch.autograd.grad(ys, xs, gs.clone().requires_grad_(), create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()
    # wald_pair on a grad-requiring ms
    ms = torch.rand(1, 4, 24, 24, generator=gen).cuda().requires_grad_()
    pan = torch.rand(1, 1, 96, 96, generator=gen).cuda()
    pair = wald_pair(ms, pan, "QB")
    pair["LR"].sum().backward()
    assert _same(ms.grad, ops.mtf_degrade_adjoint(torch.ones(1, 4, 6, 6, device="cuda"), "QB", (24, 24)))


def _rms(f, lr, sensor, ratio):
    from tmdiff_amd import ops
    return float(np.sqrt(((ops.mtf_degrade(f, sensor, ratio) - lr).cpu().double().numpy() ** 2).mean()))


@pytest.mark.parametrize("sensor,ratio,shape", [("QB", 4, (1, 4, 48, 48)), ("WV3", 2, (1, 8, 40, 24))])
def test_consistency_refine_on_the_device(sensor, ratio, shape):
    from tmdiff_amd import metrics, ops
    from tmdiff_amd.tiling import consistency_refine
    hr = np.random.default_rng(48).random(shape)
    lr = metrics.mtf_degrade(hr, sensor, ratio).astype(np.float32).astype(np.float64)
    start = metrics.upsample_poly23(lr, ratio).astype(np.float32).astype(np.float64)
    lrd, fd = torch.from_numpy(lr).float().cuda(), torch.from_numpy(start).float().cuda()
    gains = metrics.band_gains(sensor, shape[1])
    taps = np.stack([metrics.mtf_kernel(gn, ratio) for gn in gains])
    step = np.array([1.0 / metrics.mtf_opnorm2(gn, ratio) for gn in gains])[:, None, None]
    tol_f, tol_a = gpu_tol_u("mtf"), adj_tol_u("mtf", term_count(shape[2], shape[3], 41, ratio, None))
    fwd = lambda v: metrics.fir_decimate(v, np.abs(taps), ratio)
    adj = lambda v: step * metrics.fir_decimate_adjoint(v, np.abs(taps), shape[2:], ratio)
    f, bound = start, np.zeros(shape)
    rms = [_rms(fd, lrd, sensor, ratio)]
    for _ in range(8):
        low = metrics.mtf_degrade(f, gains, ratio)
        r = low - lr
        nxt = f - step * metrics.mtf_degrade_adjoint(r, gains, shape[2:], ratio)
        # every magnitude is the host's plus the bound on the device's deviation from it, so nothing of higher order is dropped
        e_low = fwd(bound) + U * tol_f * fwd(np.abs(f) + bound)                 # the error carried in, then the degradation's own
        e_r = e_low + U * (np.abs(low) + e_low + np.abs(lr))                    # then the subtraction's rounding
        bound = bound + adj(e_r) + U * tol_a * adj(np.abs(r) + e_r)             # through the adjoint, then the adjoint's own
        bound = bound + U * (np.abs(nxt) + bound)                               # the epilogue's fused multiply-add
        f = nxt
        fd = consistency_refine(fd, lrd, sensor, ratio, iters=1)
        rms.append(_rms(fd, lrd, sensor, ratio))
    assert np.array_equal(f, consistency_refine(start, lr, sensor, ratio, iters=8))
    got = consistency_refine(torch.from_numpy(start).float().cuda(), lrd, sensor, ratio, iters=8)
    assert _same(got, fd)                                                      # eight steps in one call are the eight calls
    err = np.abs(got.cpu().double().numpy() - f)
    print(f"consistency_refine {sensor} x{ratio}: max error {err.max():.3e}, bound there {bound.flat[err.argmax()]:.3e}, "
          f"largest error / bound {float((err / bound).max()):.4f}; residual RMS " + " ".join(f"{v:.6f}" for v in rms))
    assert (err <= bound).all()
    assert all(b <= a for a, b in zip(rms, rms[1:]))
    # out=: the scene itself, or another tensor; the input is left alone otherwise
    src = torch.from_numpy(start).float().cuda()
    keep = src.clone()
    other = torch.empty_like(src)
    assert consistency_refine(src, lrd, sensor, ratio, iters=8, out=other) is other and _same(other, got) and _same(src, keep)
    assert consistency_refine(src, lrd, sensor, ratio, iters=8, out=src) is src and _same(src, got)
    assert _same(consistency_refine(keep, lrd, sensor, ratio, iters=0), keep)
    with pytest.raises(ValueError):
        consistency_refine(keep, lrd, sensor, ratio, relax=2.0)


def test_metrics_ignore_requires_grad():
    """The metrics pass their own out= to the operators: an image that requires grad is scored as before, same bits."""
    from tmdiff_amd import ops
    gen = torch.Generator().manual_seed(31)
    ps, ms_exp = torch.rand(1, 4, 64, 64, generator=gen).cuda(), torch.rand(1, 4, 64, 64, generator=gen).cuda()
    pan = torch.rand(1, 1, 64, 64, generator=gen).cuda()
    want = ops.metrics_hqnr(ps, ms_exp, pan, "QB")
    got = ops.metrics_hqnr(ps.clone().requires_grad_(), ms_exp, pan.clone().requires_grad_(), "QB")
    assert torch.equal(got, want) and not got.requires_grad
    low = torch.empty(1, 1, 16, 16, device="cuda")
    lp = ops.pan_lowpass(pan.clone().requires_grad_(), "QB", low=low)
    assert _same(lp, ops.pan_lowpass(pan, "QB")) and not lp.requires_grad


def test_scaled_tap_tables_do_not_pile_up():
    from tmdiff_amd import ops
    from tmdiff_amd.tiling import consistency_refine
    f, lr = torch.rand(1, 4, 24, 24, device="cuda"), torch.rand(1, 4, 6, 6, device="cuda")
    plain = dict(ops._MTF_TAPS)
    for i in range(ops._MTF_STEP_TAPS_MAX + 3):
        consistency_refine(f, lr, "QB", 4, iters=1, relax=0.5 + 0.01 * i)
    assert len(ops._MTF_STEP_TAPS) <= ops._MTF_STEP_TAPS_MAX
    assert all(ops._MTF_TAPS[key] is plain[key] for key in plain) and len(ops._MTF_TAPS) <= len(plain) + 1
    again = consistency_refine(f, lr, "QB", 4, iters=1, relax=0.5)             # dropped and made again: the same bits
    assert _same(again, consistency_refine(f, lr, "QB", 4, iters=1, relax=0.5))


class _Stub:
    """A `diffusion` whose sample returns MS + fixed noise."""
    denoise_fn = None

    def sample(self, x_in, prompt, method="dpmsolver", **kw):
        gen = torch.Generator().manual_seed(5)
        return x_in["MS"] + 0.05 * torch.randn(x_in["MS"].shape, generator=gen).to(x_in["MS"].device)


def test_fuse_scene_with_consistency():
    from tmdiff_amd import metrics
    from tmdiff_amd.tiling import consistency_refine, fuse_scene
    gen = torch.Generator().manual_seed(21)
    hr = torch.rand(1, 4, 128, 128, generator=gen)
    lr = torch.from_numpy(metrics.mtf_degrade(hr, "QB", 4)).float().cuda()
    pan = hr.mean(1, keepdim=True).cuda()
    kw = dict(ratio=4, interp="poly23", tile=64)
    plain, q0 = fuse_scene(_Stub(), lr, pan, "QB", score="hqnr", sensor="QB", **kw)
    none, qn = fuse_scene(_Stub(), lr, pan, "QB", score="hqnr", sensor="QB", consistency=None, **kw)
    assert _same(plain, none) and all(torch.equal(q0[key], qn[key]) for key in q0)
    refined, q1 = fuse_scene(_Stub(), lr, pan, "QB", score="hqnr", sensor="QB", consistency={"iters": 4, "relax": 1.0}, **kw)
    assert _same(refined, consistency_refine(plain, lr, "QB", 4, iters=4, relax=1.0))
    assert _same(refined, fuse_scene(_Stub(), lr, pan, "QB", sensor="QB", consistency={"iters": 4, "relax": 1.0}, **kw))
    print(f"Khan's D_lambda: {float(q0['d_lambda_k']):.6f} unrefined, {float(q1['d_lambda_k']):.6f} after 4 steps")
    assert float(q1["d_lambda_k"]) <= float(q0["d_lambda_k"])
    with pytest.raises(ValueError, match="sensor"):
        fuse_scene(_Stub(), lr, pan, "QB", consistency={"iters": 4}, **kw)
