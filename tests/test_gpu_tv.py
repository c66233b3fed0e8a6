"""TV pansharpening on the GPU (csrc/tv.hip, ``ops.tv_pd_step`` / ``tv_norm`` / ``tv_pansharpen``, ``tiling.tv_fuse``, the "tv"
baseline of ``evaluate.val_dataset``).

The single step is held elementwise to ``metrics.tv_pd_step(storage=np.float32)`` on the same float32 inputs: one float32 ulp of
the expected value plus 2^-40 -- half an ulp for the single rounding, half for a tie that the fp64 operation order may flip, the
absolute term for cancellation in fp64.  ``tv_norm`` is held to n 2^-53 sum |terms| of the float64 value with
n = H W + 2 C + 2, the additions of the longest chain (the pixels, and the components under one root).  The solve's cases, the
float64 definition and the tolerances come from tests/test_tv_host.py (``tv_tol_u``: 4 times the distance of the float32
restatement from the float64 run, rounded up).  Measured on the MI355X: see DESIGN.md section 5.

No output of ``tv_pd_step`` may overlap an input (every input is read with a halo): the documented aliasing is none, the overlap
is refused, and the solve ping-pongs."""
import functools

import numpy as np
import pytest
import torch

from test_tv_host import TV_CASES, TV_ITERS, definition, tv_error_u, tv_scene, tv_tol_u

pytestmark = pytest.mark.gpu

T_H, T_W = 16, 32                                                                     # the tile of csrc/tv.hip
STEP_SHAPES = [(1, 1, 3, 5), (1, 8, T_H, T_W), (2, 4, T_H + 1, T_W + 1), (1, 16, T_H - 1, 2 * T_W + 3), (2, 3, 1, 70), (1, 2, 70, 1)]
TAU, SIGMA = 0.9, 0.07


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


def cu(a):
    return torch.from_numpy(np.array(a)).cuda()


@functools.lru_cache(maxsize=None)
def step_inputs(shape):
    """Float32 (u, x, ph, pv, pan), per-image weights with an offset, and the lam at which the projection is active on about half
    the pixels: the median over the pixels of |q|.  p is nonzero everywhere, the masked column and row included."""
    from tmdiff_amd import metrics
    b, c, h, w = shape
    rng = np.random.default_rng(h * 1000 + w)
    u, x = (rng.random(shape).astype(np.float32) for _ in range(2))
    pan = rng.random((b, 1, h, w)).astype(np.float32)
    ph, pv = ((0.05 * rng.standard_normal(shape)).astype(np.float32) for _ in range(2))
    assert ph.all() and pv.all()
    wt = np.concatenate([0.1 + 0.4 * rng.random((b, c)), 0.03 * (1 + np.arange(b))[:, None]], axis=1)
    _, qh, qv = metrics.tv_pd_step(u, x, ph, pv, pan, wt, TAU, SIGMA, 1e30, 1.0)
    lam = float(np.median(np.sqrt((qh * qh + qv * qv).sum(axis=1))))
    for a in (u, x, ph, pv, pan, wt):
        a.setflags(write=False)
    return u, x, ph, pv, pan, wt, lam


def _within_an_ulp(got, want, what):
    got, want = got.cpu().numpy().astype(np.float64), want.astype(np.float64)
    bound = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + 2.0 ** -40
    worst = float((np.abs(got - want) / bound).max())
    assert np.isfinite(got).all() and worst <= 1.0, (what, worst)
    return worst


@pytest.mark.parametrize("shape", STEP_SHAPES)
def test_pd_step_against_the_definition(shape):
    from tmdiff_amd import metrics, ops
    u, x, ph, pv, pan, wt, lam0 = step_inputs(shape)
    dev = [cu(a) for a in (u, x, ph, pv, pan)]
    wd = cu(wt)
    for lam, gamma in ((lam0, 1.0), (0.0, 1.0), (lam0, 0.0)):
        want = metrics.tv_pd_step(u, x, ph, pv, pan, wt, TAU, SIGMA, lam, gamma, storage=np.float32)
        if lam > 0.0:
            # the share of the EXPECTED output's pixels on which the projection is active: |p'| sits on the ball of radius lam
            norm = np.sqrt((want[1].astype(np.float64) ** 2 + want[2].astype(np.float64) ** 2).sum(axis=1))
            share = float((norm >= lam * (1.0 - 1e-6)).mean())
            assert 0.2 <= share <= 0.8, share
        else:
            assert not want[1].any() and not want[2].any()
        got = ops.tv_pd_step(*dev, wd, TAU, SIGMA, lam, gamma)
        worst = [_within_an_ulp(g, w_, (shape, lam, gamma, k)) for k, (g, w_) in enumerate(zip(got, want))]
        print(f"tv_pd_step {shape} lam={lam:.3g} gamma={gamma}: x', ph', pv' at most {worst[0]:.3f}, {worst[1]:.3f}, {worst[2]:.3f} of the bound")
        if lam == 0.0:
            assert not got[1].any() and not got[2].any()
    # host weights equal the device table; two calls agree; given outputs are used; a batch equals its samples
    first = ops.tv_pd_step(*dev, wd, TAU, SIGMA, lam0, 1.0)
    outs = [torch.full_like(dev[0], float("nan")) for _ in range(3)]
    again = ops.tv_pd_step(*dev, wt, TAU, SIGMA, lam0, 1.0, out_x=outs[0], out_p=(outs[1], outs[2]))
    assert all(a is o for a, o in zip(again, outs)) and all(torch.equal(a, f) for a, f in zip(again, first))
    for i in range(shape[0]):
        part = ops.tv_pd_step(*[t[i:i + 1].contiguous() for t in dev], wd[i:i + 1].contiguous(), TAU, SIGMA, lam0, 1.0)
        assert all(torch.equal(p, f[i:i + 1]) for p, f in zip(part, first))


def test_pd_step_refuses_what_it_cannot_take():
    from tmdiff_amd import ops
    u, x, ph, pv, pan, wt, lam = step_inputs(STEP_SHAPES[2])
    du, dx, dph, dpv, dpan = (cu(a) for a in (u, x, ph, pv, pan))
    spare = torch.empty_like(dx)
    for kw in (dict(out_x=du), dict(out_x=dx), dict(out_p=(dph, spare)), dict(out_p=(spare, dpv)), dict(out_p=(spare, spare)),
               dict(out_x=spare, out_p=(spare, torch.empty_like(dx))), dict(out_p=(spare,))):
        with pytest.raises(ValueError):
            ops.tv_pd_step(du, dx, dph, dpv, dpan, wt, TAU, SIGMA, lam, 1.0, **kw)
    for call in (lambda: ops.tv_pd_step(du, dx, dph, dpv, dpan, wt[:, :-1], TAU, SIGMA, lam, 1.0),
                 lambda: ops.tv_pd_step(du, dx, dph, dpv, dpan, cu(wt).float(), TAU, SIGMA, lam, 1.0),
                 lambda: ops.tv_pd_step(du, dx, dph, dpv[..., :-1].contiguous(), dpan, wt, TAU, SIGMA, lam, 1.0),
                 lambda: ops.tv_pd_step(du, dx, dph, dpv, dpan, wt, 0.0, SIGMA, lam, 1.0),
                 lambda: ops.tv_pd_step(du, dx, dph, dpv, dpan, wt, TAU, SIGMA, -1.0, 1.0),
                 lambda: ops.tv_pd_step(du.cpu(), dx.cpu(), dph.cpu(), dpv.cpu(), dpan.cpu(), wt, TAU, SIGMA, lam, 1.0),
                 lambda: ops.tv_pd_step(du.double(), dx.double(), dph.double(), dpv.double(), dpan.double(), wt, TAU, SIGMA, lam, 1.0),
                 lambda: ops.tv_norm(torch.zeros(1, 17, 4, 4, device="cuda")),
                 lambda: ops.tv_norm(dx, workspace=torch.empty(1, device="cuda", dtype=torch.float64)),
                 lambda: ops.tv_buffers(1, 4, 18, 16, "cuda", 4),
                 lambda: ops.tv_pansharpen(dx, dpan, (0.3,) * 4, 4)):
        with pytest.raises(ValueError):
            call()
    assert ops.tv_supported(1, 16, 1, 1) and not ops.tv_supported(1, 17, 4, 4)


@pytest.mark.parametrize("shape", STEP_SHAPES)
def test_tv_norm(shape):
    import math
    from tmdiff_amd import metrics, ops
    x = step_inputs(shape)[1]
    b, c, h, w = shape
    dh, dv = metrics.tv_grad(x)
    terms = np.sqrt((dh * dh + dv * dv).sum(axis=1)).reshape(b, -1)
    want = np.array([math.fsum(t) for t in terms])
    dx = cu(x)
    got = ops.tv_norm(dx)
    bound = (h * w + 2 * c + 2) * 2.0 ** -53 * terms.sum(axis=1)
    err = np.abs(got.cpu().numpy() - want)
    print(f"tv_norm {shape}: |got - float64| at most {float((err / np.maximum(bound, 1e-300)).max()):.3f} of n 2^-53 sum|terms|")
    assert got.dtype == torch.float64 and tuple(got.shape) == (b,) and (err <= bound).all()
    out, ws = torch.empty(b, device="cuda", dtype=torch.float64), ops.tv_norm_workspace(b, c, h, w, "cuda")
    assert ops.tv_norm(dx, out=out, workspace=ws) is out and torch.equal(out, got)    # equal across two runs
    assert torch.equal(ops.tv_norm(dx[b - 1:].contiguous()), got[b - 1:])             # a batch equals its samples
    assert torch.equal(ops.tv_norm(torch.full(shape, 0.37, device="cuda")), torch.zeros(b, device="cuda", dtype=torch.float64))


# ---- the solve --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def solved(name):
    """(lr, pan, x0, the float64 definition's result at TV_ITERS) of a case, computed once and shared (read-only)."""
    lr, pan, x0, _ = tv_scene(name)
    want = definition(name)
    for a in (lr, pan, x0, want):
        a.setflags(write=False)
    return lr, pan, x0, want


def _device_solve(name, iters=TV_ITERS, **kw):
    from tmdiff_amd import ops
    case = TV_CASES[name]
    lr, pan, x0, _ = solved(name)
    return ops.tv_pansharpen(cu(lr), cu(pan), case["gains"], case["ratio"], iters, case["lam"], case["gamma"], case["weights"],
                             x0=cu(x0), **kw)


@pytest.mark.parametrize("name", list(TV_CASES))
def test_solve_against_the_definition(name):
    from tmdiff_amd import metrics, ops
    case = TV_CASES[name]
    lr, pan, x0, want = solved(name)
    got = _device_solve(name)
    err = tv_error_u(got.cpu().numpy(), want, x0)
    print(f"tv_pansharpen {name}: |x - x64| / max |x64 - x0| = {err:.3f} u (tolerance {tv_tol_u(name):.0f} u)")
    assert torch.isfinite(got).all() and err <= tv_tol_u(name)
    assert torch.equal(_device_solve(name), got)                                      # a second call
    assert torch.equal(_device_solve(name, 0), cu(x0))                                # iters = 0 returns the start
    start = ops.tv_pansharpen(cu(lr), cu(pan), case["gains"], case["ratio"], 0)
    assert torch.equal(start, ops.upsample_poly23(cu(lr), case["ratio"]))
    wd = cu(metrics.tv_weights(case["weights"], *case["shape"][:2]))
    assert torch.equal(ops.tv_pansharpen(cu(lr), cu(pan), case["gains"], case["ratio"], 3, case["lam"], case["gamma"], wd, x0=cu(x0)),
                       _device_solve(name, 3))                                        # a device table of weights, an odd count
    if case["shape"][0] > 1:                                                          # a batch equals its samples
        one = ops.tv_pansharpen(cu(lr[1:]), cu(pan[1:]), case["gains"], case["ratio"], TV_ITERS, case["lam"], case["gamma"],
                                case["weights"][1], x0=cu(x0[1:]))
        assert torch.equal(one, got[1:])


def test_graph_replay_and_no_allocation():
    from tmdiff_amd import ops
    name = "QB x4 40x72"
    case = TV_CASES[name]
    lr, pan, x0, _ = solved(name)
    eager = _device_solve(name)
    b, c, h, w = case["shape"]
    buf, out = ops.tv_buffers(b, c, h, w, "cuda", case["ratio"]), torch.empty(b, c, h, w, device="cuda")
    dlr, dpan, dx0 = torch.zeros_like(cu(lr)), torch.zeros_like(cu(pan)), torch.zeros_like(cu(x0))
    args = (dlr, dpan, case["gains"], case["ratio"], TV_ITERS, case["lam"], case["gamma"], case["weights"])
    ops.tv_pansharpen(*args, x0=dx0, out=out, buffers=buf)                            # warm: the taps and the weights are cached
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    ops.tv_pansharpen(*args, x0=dx0, out=out, buffers=buf)
    assert torch.cuda.memory_allocated() == before
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.tv_pansharpen(*args, x0=dx0, out=out, buffers=buf)
    dlr.copy_(cu(lr))
    dpan.copy_(cu(pan))
    dx0.copy_(cu(x0))
    for _ in range(2):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


# ---- users ----------------------------------------------------------------------------------------------------------------------
def test_tiling_tv_fuse_on_the_device():
    from tmdiff_amd import metrics as M, ops
    from tmdiff_amd.tiling import consistency_refine, tv_fuse
    g = torch.Generator().manual_seed(12)
    lr, pan = (0.1 + 0.8 * torch.rand(1, 4, 16, 16, generator=g)).cuda(), (0.1 + 0.8 * torch.rand(1, 1, 64, 64, generator=g)).cuda()
    ms_exp = ops.upsample_poly23(lr, 4)
    base = ops.tv_pansharpen(lr, pan, "QB", 4, 6, x0=ms_exp)
    assert torch.equal(tv_fuse(lr, pan, "QB", iters=6), base) and torch.equal(ops.tv_pansharpen(lr, pan, "QB", 4, 6), base)
    scene, score = tv_fuse(lr, pan, "QB", iters=6, score=True)
    want = M.quality_fullres(lr, pan, scene)
    assert torch.equal(scene, base) and set(score) == set(want) and all(torch.equal(score[k], want[k]) for k in want)
    refined = tv_fuse(lr, pan, "QB", iters=6, consistency={"iters": 2})
    assert torch.equal(refined, consistency_refine(base, lr, "QB", 4, iters=2))
    # weights="regress": the least-squares fit of the reduced PAN by the bands and a constant, solved here
    low = M.mtf_degrade(pan.cpu().numpy().astype(np.float64), "QB", 4, pan=True)
    design = np.concatenate([lr[0].cpu().numpy().astype(np.float64).reshape(4, -1), np.ones((1, 256))]).T
    wt = np.linalg.lstsq(design, low.reshape(-1), rcond=None)[0]
    got = tv_fuse(lr, pan, "QB", iters=6, weights="regress")
    assert torch.equal(got, tv_fuse(lr, pan, "QB", iters=6, weights=wt)) and not torch.equal(got, base)
    assert torch.equal(got, ops.tv_pansharpen(lr, pan, "QB", 4, 6, weights=wt[None]))


def test_val_dataset_tv_baseline(tmp_path):
    from test_bdsd_host import bdsd_inputs
    from test_gpu_bdsd import _Trainer
    from tmdiff_amd import evaluate, metrics as M, ops
    loader = []
    for seed in (31, 32):
        ms, pan = bdsd_inputs(seed, 1, 4, 64, 64)
        hr = (0.5 * ms + 0.5 * pan).clamp(0, 1)
        loader.append({"MS": ms.cuda(), "PAN": pan.cuda(), "LR": ms[..., 2::4, 2::4].contiguous().cuda(), "HR": hr.cuda()})
    kw = dict(device_metrics=True, log=lambda *a: None)
    base = evaluate.val_dataset(_Trainer(), "QB", loader, str(tmp_path / "base"), baselines=("exp",), **kw)
    got = evaluate.val_dataset(_Trainer(), "QB", loader, str(tmp_path / "tv"), baselines=("exp", "tv"), **kw)
    fields = ("ssim", "sam", "psnr", "ergas", "scc", "cc", "q")
    assert set(got) == set(base) | {f"{k}_QB@tv" for k in fields}
    assert all(got[k] == base[k] for k in base if k != "sec_per_item")                # the @exp keys and the plain keys are unchanged
    rows = [ops.metrics_pair(d["HR"], ops.tv_pansharpen(d["LR"], d["PAN"], "QB", x0=d["MS"]), 1.0)[0].cpu().numpy() for d in loader]
    want = dict(zip(M.PAIR_FIELDS, np.mean(rows, 0)))
    for k in fields:
        assert np.isfinite(got[f"{k}_QB@tv"]) and abs(got[f"{k}_QB@tv"] - want[k]) <= 1e-9 * max(1.0, abs(want[k])), k
    assert evaluate.TV_BASELINES == ("tv",)
