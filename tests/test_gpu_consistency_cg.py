"""Wald's consistency as a CGLS solve on the GPU (csrc/cg.hip, ``ops.plane_dots``, ``ops.consistency_solve``,
``tiling.consistency_solve``) and inside the DPM-Solver steps (``GeneralDiffusion.sample_by_dpmsolver(consistency=...)``,
``fuse_scene(consistency={"method": "cg", "in_loop": True})``).

The cases, the float64 definition's results and the tolerances come from tests/test_consistency_cg_host.py: the device is held to
4 times the distance of the float32 restatement from the definition, rounded up (``cg_tol_u``), on the correction d.
Measured on the MI355X, |d - d64| / max |d64| in u: see DESIGN.md section 5."""
import functools

import numpy as np
import pytest
import torch

from test_consistency_cg_host import CG_CASES, CG_DAMP, CG_ITERS, cg_scene, cg_tol_u, correction_error_u

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


def cu(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.array(a))).float().cuda().contiguous()


@functools.lru_cache(maxsize=None)
def definition(key):
    """(f0, lr, the float64 definition's f) of a case, computed once and shared (read-only)."""
    from tmdiff_amd import metrics
    name, damp = ("QB x4 48", CG_DAMP) if key == "damp" else (key, 0.0)
    sensor, ratio, _ = CG_CASES[name]
    f0, lr = cg_scene(name)
    want = metrics.consistency_solve(f0, lr, sensor, ratio, CG_ITERS, damp)
    for a in (f0, lr, want):
        a.setflags(write=False)
    return f0, lr, want, sensor, ratio, damp


# ---- ops.plane_dots ---------------------------------------------------------------------------------------------------
DOT_SHAPES = [(1, 1, 5, 7),          # a plane smaller than one chunk
              (2, 3, 67, 131),       # three chunks with a ragged tail, an odd width: no plane but the first is 16-byte aligned
              (2, 3, 64, 96),        # the 16-byte path, two chunks
              (2, 2500, 3, 3)]       # 5000 planes: more than the launch has workgroups


def _dot_check(got, a, b, exact):
    a64, b64 = a.double().cpu().numpy(), b.double().cpu().numpy()
    want = (a64 * b64).sum(axis=(2, 3))
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float64
    if exact:
        assert np.array_equal(got, want)
    else:
        n = a.shape[2] * a.shape[3]
        bound = n * 2.0 ** -53 * np.abs(a64 * b64).sum(axis=(2, 3))
        worst = float((np.abs(got - want) / bound).max())
        print(f"plane_dots {tuple(a.shape)}: |got - numpy| at most {worst:.3f} of n 2^-53 sum|a b|")
        assert (np.abs(got - want) <= bound).all()


@pytest.mark.parametrize("shape", DOT_SHAPES)
def test_plane_dots(shape):
    from tmdiff_amd import ops
    g = torch.Generator().manual_seed(shape[2] * 100 + shape[3])
    ia, ib = (torch.randint(-8, 9, shape, generator=g).float().cuda() for _ in range(2))
    _dot_check(ops.plane_dots(ia, ib), ia, ib, True)
    _dot_check(ops.plane_dots(ia), ia, ia, True)
    ra, rb = (torch.randn(shape, generator=g).cuda() for _ in range(2))
    got = ops.plane_dots(ra, rb)
    _dot_check(got, ra, rb, False)
    _dot_check(ops.plane_dots(ra), ra, ra, False)
    # buffers given: the same bits, nothing new
    out = torch.empty(shape[:2], device="cuda", dtype=torch.float64)
    ws = torch.empty(shape[0] * shape[1] * ops.plane_dots_partials(shape[2] * shape[3]), device="cuda", dtype=torch.float64)
    assert ops.plane_dots(ra, rb, out=out, workspace=ws) is out and torch.equal(out, got)
    # a batch equals its samples
    assert torch.equal(ops.plane_dots(ra[1:], rb[1:]), got[1:])


def test_plane_dots_two_extents_in_one_call():
    from tmdiff_amd import ops
    g = torch.Generator().manual_seed(3)
    full, low = torch.randn(2, 3, 200, 136, generator=g).cuda(), torch.randn(2, 3, 50, 34, generator=g).cuda()
    other = torch.randn(2, 3, 50, 34, generator=g).cuda()
    got = ops.plane_dots((full, low), (full, other))
    assert tuple(got.shape) == (2, 2, 3)
    assert torch.equal(got[0], ops.plane_dots(full)) and torch.equal(got[1], ops.plane_dots(low, other))
    _dot_check(got[0], full, full, False)
    _dot_check(got[1], low, other, False)
    with pytest.raises(ValueError):
        ops.plane_dots((full, low[:, :2]))
    with pytest.raises(ValueError):
        ops.plane_dots(full, low)
    with pytest.raises(ValueError):
        ops.plane_dots(full.cpu())


# ---- the update kernels -----------------------------------------------------------------------------------------------
def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("full,low", [((67, 131), (17, 33)), ((64, 72), (16, 18))])
def test_update_kernels(full, low):
    """Integer-valued partial sums make every total exact in any order, so alpha and beta are the host's float64 quotients rounded
    to float32, bit for bit; an element is then one fused multiply-add: within 1 ulp of the float64 evaluation rounded to float32."""
    from tmdiff_amd import ops
    from tmdiff_amd._lib import check, lib
    planes, nf, nl = 6, full[0] * full[1], low[0] * low[1]
    cf, cl = ops.plane_dots_partials(nf), ops.plane_dots_partials(nl)
    g = torch.Generator().manual_seed(nf)
    ints = lambda n, lo: torch.randint(lo, 50, (planes, n), generator=g).double()
    gam, qq, pp, old = ints(cf, 0), ints(cl, 1), ints(cf, 0), ints(cf, 1)
    qq[2] = 0.0                      # delta == 0 at damp == 0: alpha is exactly 0
    old[4] = 0.0                     # gamma == 0: beta is exactly 0
    p, d, s = (torch.randn(1, planes, *full, generator=g) for _ in range(3))
    q, r = (torch.randn(1, planes, *low, generator=g) for _ in range(2))
    col = lambda t: t.sum(1).numpy()[None, :, None, None]
    gam_d, qq_d, pp_d, old_d = gam.cuda(), qq.cuda(), pp.cuda(), old.cuda()
    for damp, first in ((0.0, False), (0.25, False), (0.0, True)):
        delta = col(qq) + damp * col(pp)
        alpha = np.divide(col(gam), delta, out=np.zeros_like(delta), where=delta != 0.0).astype(np.float32).astype(np.float64)
        want_d = alpha * p.double().numpy() + (0.0 if first else d.double().numpy())
        want_r = -alpha * q.double().numpy() + r.double().numpy()
        dd, rr_, pd, qd = d.cuda(), r.cuda(), p.cuda(), q.cuda()
        rr = torch.full((planes, cl), float("nan"), device="cuda", dtype=torch.float64)
        check(lib.tmdiff_cg_step(pd.data_ptr(), qd.data_ptr(), dd.data_ptr(), rr_.data_ptr(), gam_d.data_ptr(), qq_d.data_ptr(),
                                 pp_d.data_ptr() if damp else None, damp, rr.data_ptr(), planes, nf, nl, int(first),
                                 torch.cuda.current_stream().cuda_stream))
        got_d, got_r = dd.cpu().double().numpy(), rr_.cpu().double().numpy()
        assert (np.abs(got_d - want_d) <= _ulp32(want_d)).all() and (np.abs(got_r - want_r) <= _ulp32(want_r)).all()
        if damp == 0.0:              # the guard: the plane keeps d (0 on the first step) and r, bit for bit
            assert np.array_equal(got_d[0, 2], np.zeros(full) if first else d[0, 2].double().numpy())
            assert np.array_equal(got_r[0, 2], r[0, 2].double().numpy())
        # the partial sums of the new <r, r> are those of plane_dots
        tot = torch.empty(planes, device="cuda", dtype=torch.float64)
        check(lib.tmdiff_plane_totals(rr.data_ptr(), tot.data_ptr(), planes, cl, 1, 0, torch.cuda.current_stream().cuda_stream))
        assert torch.equal(tot.view(1, planes), ops.plane_dots(rr_))
    beta = np.divide(col(gam), col(old), out=np.zeros_like(col(gam)), where=col(old) != 0.0).astype(np.float32).astype(np.float64)
    want_p = beta * p.double().numpy() + s.double().numpy()
    pd, sd = p.cuda(), s.cuda()
    ppo = torch.full((planes, cf), float("nan"), device="cuda", dtype=torch.float64)
    check(lib.tmdiff_cg_direction(sd.data_ptr(), pd.data_ptr(), gam_d.data_ptr(), old_d.data_ptr(), ppo.data_ptr(), planes, nf,
                                  torch.cuda.current_stream().cuda_stream))
    got_p = pd.cpu().double().numpy()
    assert (np.abs(got_p - want_p) <= _ulp32(want_p)).all()
    assert np.array_equal(got_p[0, 4], s[0, 4].double().numpy())
    tot = torch.empty(planes, device="cuda", dtype=torch.float64)
    check(lib.tmdiff_plane_totals(ppo.data_ptr(), tot.data_ptr(), planes, cf, 1, 0, torch.cuda.current_stream().cuda_stream))
    assert torch.equal(tot.view(1, planes), ops.plane_dots(pd))


# ---- the solve --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(CG_CASES) + ["damp"])
def test_solve_against_the_definition(key):
    from tmdiff_amd import metrics, ops
    from tmdiff_amd.tiling import consistency_solve
    f0, lr, want, sensor, ratio, damp = definition(key)
    f0d, lrd = cu(f0), cu(lr)
    got = consistency_solve(f0d, lrd, sensor, ratio, iters=CG_ITERS, damp=damp)
    assert got.data_ptr() != f0d.data_ptr() and torch.equal(f0d, cu(f0))           # the input is left as it is
    err = correction_error_u(got.cpu().numpy(), f0, want, f0.astype(np.float64))
    print(f"consistency_solve {key}: |d - d64| / max |d64| = {err:.3f} u (tolerance {cg_tol_u(key):.0f} u)")
    assert err <= cg_tol_u(key)
    # the trace of the recurrence does not grow, and agrees with the definition's
    taps = ops._mtf_taps(metrics.band_gains(sensor, f0.shape[1]), ratio, f0d.device)
    info = torch.empty(*f0.shape[:2], CG_ITERS + 1, device="cuda", dtype=torch.float64)
    d = torch.empty_like(f0d)
    again = ops.consistency_solve(f0d, lrd, taps, ratio, CG_ITERS, damp, correction_out=d, info_out=info)
    assert torch.equal(again, got) and torch.equal(ops.add(f0d, d), got)
    tr = info.cpu().numpy()
    assert np.isfinite(tr).all() and (tr[..., 1:] <= tr[..., :-1]).all()
    _, want_info = metrics.consistency_solve(f0, lr, sensor, ratio, CG_ITERS, damp, return_info=True)
    assert np.abs(tr - want_info).max() <= 1e-3 * want_info.max()
    # independently of the recurrence: the residual, recomputed
    res = lambda f: float((lrd - ops.mtf_degrade(f, sensor, ratio)).double().pow(2).sum().sqrt())
    ratio_reached = res(got) / res(f0d)
    print(f"consistency_solve {key}: ||lr - A f|| / ||lr - A f0|| = {ratio_reached:.4f} after {CG_ITERS} iterations")
    if key == "QB x4 48":
        assert ratio_reached < 0.1


def test_solve_is_deterministic_and_takes_aliases():
    from tmdiff_amd import metrics, ops
    f0, lr, _, sensor, ratio, _ = definition("3 bands x4 200x136")
    f0d, lrd = cu(f0), cu(lr)
    taps = ops._mtf_taps(metrics.band_gains(sensor, f0.shape[1]), ratio, f0d.device)
    first = ops.consistency_solve(f0d, lrd, taps, ratio, CG_ITERS)
    assert torch.equal(ops.consistency_solve(f0d, lrd, taps, ratio, CG_ITERS), first)               # a second call
    for i in range(f0d.shape[0]):                                                                  # a batch equals its samples
        assert torch.equal(ops.consistency_solve(f0d[i:i + 1].contiguous(), lrd[i:i + 1].contiguous(), taps, ratio, CG_ITERS), first[i:i + 1])
    alias = f0d.clone()
    assert ops.consistency_solve(alias, lrd, taps, ratio, CG_ITERS, out=alias) is alias and torch.equal(alias, first)
    # iters = 0 and the workspace of a longer run
    ws = ops.consistency_solve_workspace(*f0d.shape, ratio, CG_ITERS, "cuda")
    assert torch.equal(ops.consistency_solve(f0d, lrd, taps, ratio, 0, workspace=ws), f0d)
    assert torch.equal(ops.consistency_solve(f0d, lrd, taps, ratio, 3, workspace=ws), ops.consistency_solve(f0d, lrd, taps, ratio, 3))
    # a consistent plane comes back unchanged and the others do not see it
    lr2 = lrd.clone()
    lr2[1, 2] = ops.mtf_degrade(f0d, sensor, ratio)[1, 2]
    info = torch.empty(2, 3, CG_ITERS + 1, device="cuda", dtype=torch.float64)
    got = ops.consistency_solve(f0d, lr2, taps, ratio, CG_ITERS, info_out=info)
    assert torch.isfinite(got).all() and torch.isfinite(info).all() and not info[1, 2].any()
    assert torch.equal(got[1, 2], f0d[1, 2])
    keep = torch.ones(2, 3, dtype=torch.bool)
    keep[1, 2] = False
    assert torch.equal(got[keep], first[keep])
    with pytest.raises(ValueError):
        ops.consistency_solve(f0d, lrd[..., :-1].contiguous(), taps, ratio, 2)
    with pytest.raises(ValueError):
        ops.consistency_solve(f0d, lrd, taps, ratio, -1)
    with pytest.raises(ValueError):
        ops.consistency_solve(f0d, lrd, taps, ratio, 2, damp=-1.0)
    with pytest.raises(ValueError):
        ops.consistency_solve(f0d, lrd, taps, ratio, CG_ITERS + 1, workspace=ws)                     # too small for 9 traces


def test_graph_replay_equals_the_eager_call():
    from tmdiff_amd import metrics, ops
    f0, lr, _, sensor, ratio, _ = definition("QB x4 48")
    f0d, lrd = cu(f0), cu(lr)
    taps = ops._mtf_taps(metrics.band_gains(sensor, f0.shape[1]), ratio, f0d.device)
    eager_info = torch.empty(1, 4, CG_ITERS + 1, device="cuda", dtype=torch.float64)
    eager = ops.consistency_solve(f0d, lrd, taps, ratio, CG_ITERS, CG_DAMP, info_out=eager_info)
    ws = ops.consistency_solve_workspace(*f0d.shape, ratio, CG_ITERS, "cuda")
    out, d, info = torch.zeros_like(f0d), torch.zeros_like(f0d), torch.zeros_like(eager_info)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()

    def allocations_of(body):
        """(the graph, the allocator's requests while it was captured)."""
        graph = torch.cuda.CUDAGraph()
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        with torch.cuda.graph(graph, stream=stream):
            body()
        return graph, torch.cuda.memory_stats()["allocation.all.allocated"] - before

    # torch allocates its generator's capture state while the first live graph is captured: keep one alive beside ours
    warm, _ = allocations_of(lambda: ops.add(f0d, d, out=out))
    graph, made = allocations_of(lambda: ops.consistency_solve(f0d, lrd, taps, ratio, CG_ITERS, CG_DAMP, out=out, correction_out=d,
                                                               info_out=info, workspace=ws))
    assert made == 0                                                                # the call allocated nothing while captured
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and torch.equal(info, eager_info) and torch.equal(ops.add(f0d, d), eager)


def test_fuse_functions_take_the_solve():
    from tmdiff_amd.tiling import classical_fuse, consistency_solve
    g = torch.Generator().manual_seed(9)
    lr, pan = torch.rand(1, 4, 16, 16, generator=g).cuda(), torch.rand(1, 1, 64, 64, generator=g).cuda()
    base = classical_fuse(lr, pan, "QB")
    assert torch.equal(classical_fuse(lr, pan, "QB", consistency={"method": "cg", "iters": 3, "damp": 1e-4}),
                       consistency_solve(base, lr, "QB", 4, iters=3, damp=1e-4))
    assert torch.equal(classical_fuse(lr, pan, "QB", consistency={"method": "landweber", "iters": 2}),
                       classical_fuse(lr, pan, "QB", consistency={"iters": 2}))


# ---- inside the sampler -----------------------------------------------------------------------------------------------
class _Stub(torch.nn.Module):
    """A denoiser that predicts one fixed residual in [-0.5, 0.5]: dynamic thresholding is the identity on it."""

    def __init__(self, value):
        super().__init__()
        self.value = value

    def forward(self, x_t, t_input, PAN=None, MS=None, prompt=None):
        return self.value


def _diffusion(net):
    from tmdiff_amd.diffusion_general import GeneralDiffusion
    diff = GeneralDiffusion(net, "l1", noise_fn=lambda like: torch.randn(like.shape, dtype=torch.float32)).cuda()
    diff.set_new_noise_schedule({"schedule": "cosine", "n_timestep": 1000}, "cuda")
    return diff


def test_sampler_projects_every_data_prediction():
    from tmdiff_amd import metrics
    from tmdiff_amd.tiling import consistency_solve
    g = torch.Generator().manual_seed(17)
    truth = torch.rand(1, 4, 48, 48, generator=g)
    lr = cu(metrics.mtf_degrade(truth, "QB", 4))
    ms = cu(metrics.upsample_poly23(lr.cpu().numpy(), 4))
    stub = (torch.rand(1, 4, 48, 48, generator=g) - 0.5).cuda()
    x_in = {"MS": ms, "PAN": torch.rand(1, 1, 48, 48, generator=g).cuda(), "Res": torch.zeros_like(ms)}
    diff = _diffusion(_Stub(stub))
    opts = {"lr_ms": lr, "sensor": "QB", "ratio": 4, "iters": 4, "damp": 0.0}
    torch.manual_seed(1)
    got = diff.sample_by_dpmsolver(x_in, "QB", steps=3, consistency=opts)
    assert diff.last_solver.nfe == 4
    want = consistency_solve(stub + ms, lr, "QB", 4, iters=4)
    gap = float(((got - want).abs() / want.abs().clamp(min=1.0)).max())
    print(f"sampler with a stub denoiser: max |sample - solve| / max(1, |v|) = {gap:.3e} (2^-21 = {2.0 ** -21:.3e})")
    assert gap <= 2.0 ** -21
    torch.manual_seed(1)
    through = diff.sample(x_in, "QB", method="dpmsolver", steps=3, consistency=opts)
    assert torch.equal(through, got)
    torch.manual_seed(1)
    plain = diff.sample_by_dpmsolver(x_in, "QB", steps=3)
    torch.manual_seed(1)
    assert torch.equal(diff.sample_by_dpmsolver(x_in, "QB", steps=3, consistency=None), plain)
    assert not torch.equal(plain, got)
    with pytest.raises(ValueError):
        diff.sample(x_in, "QB", method="ddpm", consistency=opts)


def test_fuse_scene_in_loop_through_the_tiny_unet():
    from oracle import unet_ref as U
    from oracle.make_golden import TINY
    from tmdiff_amd.Hyper_unet_general import WavBEST
    from tmdiff_amd.tiling import fuse_scene
    ref = U.fill_weights_(U.WavBESTRef(channels=TINY)).eval()
    net = WavBEST(channels=TINY)
    net.load_state_dict(ref.state_dict())
    diff = _diffusion(net.cuda().eval())
    g = torch.Generator().manual_seed(70)
    lr_ms, pan = torch.rand(1, 8, 24, 24, generator=g).cuda(), torch.rand(1, 1, 96, 96, generator=g).cuda()
    opts = {"method": "cg", "in_loop": True, "iters": 2}
    torch.manual_seed(11)
    scene = fuse_scene(diff, lr_ms, pan, "WV3", sensor="WV3", interp="poly23", method="dpmsolver", steps=3, overlap=8, consistency=opts)
    assert tuple(scene.shape) == (1, 8, 96, 96) and torch.isfinite(scene).all()
    torch.manual_seed(11)
    loop_only = fuse_scene(diff, lr_ms, pan, "WV3", sensor="WV3", interp="poly23", method="dpmsolver", steps=3, overlap=8,
                           consistency=dict(opts, iters_post=0))
    assert torch.isfinite(loop_only).all() and not torch.equal(loop_only, scene)
    with pytest.raises(ValueError, match="fused tile mode"):
        fuse_scene(diff, lr_ms, pan, "WV3", sensor="WV3", method="dpmsolver", steps=3, tile=32, consistency=opts)
