"""The SSIM loss term on the device (csrc/ssim_loss.hip: dssim = 1 - SSIM, value and gradient from one kernel pair) against its
float64 definition, tmdiff_amd.losses.ssim_loss_host, on the same fp32 inputs with the gradient from torch autograd on the CPU.

The kernel's tile is 16 x 32 for every window size.  Shapes for win = 7: H from 7, 8, 15, 16, 17, 22, 23, 33 and W from 7, 8, 31, 32, 33, 38, 39, 65 -- one window, two windows, the tile minus 1, exactly, plus 1, plus
win - 1, plus win, two tiles plus 1 -- with B in {1, 3} and C in {1, 4, 8, 17}; win = 3 at 3 x 3 and 5 x 36, win = 11 at 11 x 11
and 19 x 44.  W = 8, 32, 36, 44 take the 16-byte path, the others the scalar one; nothing is larger than two tiles and one pixel
per axis.

Tolerances (derived, none measured).  ssim and dssim: 1e-11 absolute (|S| <= 1; the worst window's cancellation in
f(a a) - ux^2 is about 1e-15 against B2 >= c2 = 9e-4).  The fp32 total is the fp32 rounding of the fp64 value exactly.  Gradient,
standalone, per element: 4 * 2^-24 |g_ref| + 1e-12 max|g_ref| -- one fp32 rounding of a value that agrees in fp64, the floor
because an element is a signed sum of up to 3 n window terms.  Gradient accumulated onto a composite gradient gc, per element:
8 * 2^-24 (|gc_ref| + |s_ref|) plus the same floor: fl32(gc32 + s) carries the composite's 4 * 2^-24 |gc| and one more rounding."""
import math

import numpy as np
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 7, 7), (3, 4, 8, 8), (1, 4, 15, 31), (1, 8, 16, 32), (3, 4, 17, 33), (1, 17, 22, 38), (1, 8, 23, 39), (1, 4, 33, 65),
          (3, 1, 7, 65), (1, 4, 33, 7), (3, 8, 16, 36), (1, 4, 22, 31), (1, 1, 8, 39)]
WIN_SHAPES = [(3, (1, 4, 3, 3)), (3, (3, 4, 5, 36)), (11, (1, 4, 11, 11)), (11, (3, 4, 19, 44)), (5, (1, 4, 17, 33)), (9, (1, 4, 17, 36))]
CASES = [(7, s) for s in SHAPES] + WIN_SHAPES
EPS = 2.0 ** -24


def case_id(c):
    return f"win{c[0]}-" + "x".join(map(str, c[1]))


def inputs(kind, seed, shape):
    """float32 on the host.  `uniform`: x_true ~ U[0, 1), x_pred = x_true + 0.1 N(0, 1).  `normal`: both ~ N(0, 1), where the
    window means are near 0 and B1 is near c1."""
    g = torch.Generator().manual_seed(seed)
    if kind == "uniform":
        a = torch.rand(*shape, generator=g)
        return a, a + 0.1 * torch.randn(*shape, generator=g)
    return torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)


def yardstick(a, b, win=7, data_range=1.0):
    """([dssim, ssim] float64, d dssim / d x_pred float64) from the host definition and CPU autograd"""
    from tmdiff_amd.losses import ssim_loss_host
    x = b.double().requires_grad_(True)
    dssim, ssim = ssim_loss_host(a, x, win, data_range)
    g, = torch.autograd.grad(dssim, x)
    return torch.stack([dssim.detach(), ssim.detach()]), g


_YARD = {}


def shared(kind, seed, win, shape):
    key = (kind, seed, win, shape)
    if key not in _YARD:
        a, b = inputs(kind, seed, shape)
        _YARD[key] = (a, b) + yardstick(a, b, win)
    return _YARD[key]


def cu(t):
    return None if t is None else t.detach().cuda().contiguous()


def run(a, b, win=7, **kw):
    from tmdiff_amd import ops
    return ops.ssim_loss(cu(a), cu(b), win, **kw)


def assert_values(out, total32, want, weight, what):
    got = out.cpu()
    assert abs(float(got[0]) - float(want[0])) <= 1e-11 and abs(float(got[1]) - float(want[1])) <= 1e-11, (what, got, want)
    assert float(got[0]) == 1.0 - float(got[1]), what
    assert float(total32) == float(np.float32(weight * float(got[0]))), what


def assert_gradient(g, want, what, rel=4.0 * EPS, mag=None):
    """per element: rel * mag + 1e-12 max|want| (mag: |want| unless given)"""
    err = (g.cpu().double() - want).abs()
    bound = rel * (want.abs() if mag is None else mag) + 1e-12 * float(want.abs().max())
    worst = float((err / bound.clamp_min(1e-300)).max()) if float(bound.max()) > 0.0 else float(err.max() > 0)
    assert worst <= 1.0, f"{what}: an element is off by {worst:.3f} of its bound"
    return worst


@pytest.mark.parametrize("kind", ["uniform", "normal"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_value_and_gradient_against_the_float64_definition(case, kind):
    win, shape = case
    a, b, want, gwant = shared(kind, 11, win, shape)
    out, total32, g = run(a, b, win)
    what = f"win={win} {shape} {kind}"
    assert_values(out, total32, want, 1.0, what)
    worst = assert_gradient(g, gwant, what)
    print(f"{what}: dssim {float(out[0]):.15g} (definition {float(want[0]):.15g}), worst gradient element at {worst:.3f} of its bound")
    # a weight scales the gradient and the fp32 total, not the fp64 values
    out2, total2, g2 = run(a, b, win, weight=0.3)
    assert torch.equal(out2, out)
    assert float(total2) == float(np.float32(0.3 * float(out[0])))
    assert_gradient(g2, 0.3 * gwant, what + " weight 0.3")


@pytest.mark.parametrize("shape", [(1, 4, 17, 32), (3, 4, 19, 36), (1, 4, 9, 33)], ids=lambda s: "x".join(map(str, s)))
def test_unaligned_tensors_take_the_scalar_path_and_nothing_is_written_outside(shape):
    """Windows one float off a 16-byte boundary inside flat buffers (W % 4 == 0 in two cases: alignment alone decides); the
    gradient's buffer keeps its sentinel on both sides, and the values equal the aligned call's bit for bit."""
    from tmdiff_amd import ops
    a, b, want, gwant = shared("uniform", 12, 7, shape)
    n, pad = math.prod(shape), 64

    def window(data, fill):
        flat = torch.full((pad + 1 + n + pad,), fill, device="cuda", dtype=torch.float32)
        view = flat[pad + 1:pad + 1 + n].view(shape)
        if data is not None:
            view.copy_(data)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return flat, view

    (_, va), (_, vb) = window(a, float("nan")), window(b, float("nan"))
    gflat, gview = window(None, 777.0)
    out, total32, g = ops.ssim_loss(va, vb, grad=gview)
    assert g is gview
    assert_values(out, total32, want, 1.0, f"{shape} unaligned")
    assert_gradient(g, gwant, f"{shape} unaligned")
    assert bool((gflat[:pad + 1] == 777.0).all()) and bool((gflat[pad + 1 + n:] == 777.0).all())
    out2, _, g2 = run(a, b)
    assert torch.equal(out2, out) and torch.equal(g2, g)


@pytest.mark.parametrize("case", [(7, (3, 4, 17, 33)), (7, (1, 8, 16, 32)), (11, (1, 4, 19, 44))], ids=case_id)
def test_value_only_mode_writes_no_gradient(case):
    from tmdiff_amd import autograd as A
    win, shape = case
    a, b = (cu(t) for t in inputs("uniform", 22, shape))
    out, total, g = run(a, b, win)
    g.fill_(float("nan"))                               # the buffer the gradient mode wrote, poisoned: the next call does not get it
    keep = g.clone()
    out2, total2, none = run(a, b, win, grad=False)
    torch.cuda.synchronize()
    assert none is None and torch.equal(out2, out) and torch.equal(total2, total)
    assert torch.equal(g.view(torch.int32), keep.view(torch.int32))
    # the autograd function selects it when x_pred needs no gradient, and saves g when it does
    loss, t3 = A.ssim_loss(a, b, win)
    assert not loss.requires_grad and torch.equal(t3, out) and torch.equal(loss, total)
    leaf = b.clone().requires_grad_(True)
    loss, t4 = A.ssim_loss(a, leaf, win)
    assert loss.requires_grad and not t4.requires_grad
    (3.0 * loss).backward()
    _, _, gref = run(a, b, win)
    assert torch.equal(leaf.grad, gref * 3.0)


@pytest.mark.parametrize("case", [(7, (3, 4, 17, 33)), (7, (1, 8, 16, 36)), (3, (1, 4, 5, 36)), (11, (1, 4, 19, 44))], ids=case_id)
def test_identical_inputs_have_zero_dssim_exactly(case):
    win, shape = case
    for kind in ("uniform", "normal"):
        a, _ = inputs(kind, 31, shape)
        out, total32, g = run(a, a.clone(), win)
        assert float(out[0]) == 0.0 and float(out[1]) == 1.0 and float(total32) == 0.0, (kind, out)
        assert float(g.abs().max()) <= 1e-12, (kind, float(g.abs().max()))


@pytest.mark.parametrize("shape", [(3, 4, 17, 33), (1, 8, 16, 36)], ids=lambda s: "x".join(map(str, s)))
def test_constant_planes_stay_finite_and_within_the_bounds(shape):
    """Zero variance in every window: B2 is c2 up to the rounding of f(a a) - ux^2."""
    b_, c, h, w = shape
    lev = torch.linspace(0.05, 0.95, b_ * c).view(b_, c, 1, 1)
    a = lev.expand(shape).contiguous()
    b = (0.9 * lev + 0.07).expand(shape).contiguous()
    want, gwant = yardstick(a, b)
    out, total32, g = run(a, b)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(g).all()) and bool(torch.isfinite(total32))
    assert_values(out, total32, want, 1.0, f"{shape} constant")
    worst = assert_gradient(g, gwant, f"{shape} constant")
    print(f"{shape} constant planes: dssim {float(out[0]):.15g}, worst gradient element at {worst:.3f} of its bound")


def test_two_calls_and_two_replays_give_identical_bits():
    from tmdiff_amd import ops
    shape = (3, 8, 19, 36)
    a, b = (cu(t) for t in inputs("uniform", 21, shape))
    first = ops.ssim_loss(a, b, weight=0.7)
    again = ops.ssim_loss(a, b, weight=0.7)
    for u, v in zip(first, again):
        assert torch.equal(u, v)
    ws = torch.empty(ops.lib.tmdiff_ssim_loss_workspace_bytes(*shape, 7), device="cuda", dtype=torch.uint8)
    out, total, g = torch.empty(2, device="cuda", dtype=torch.float64), torch.empty((), device="cuda"), torch.empty_like(b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # one eager call on the capture stream first
        ops.ssim_loss(a, b, weight=0.7, grad=g, out=out, total=total, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.ssim_loss(a, b, weight=0.7, grad=g, out=out, total=total, workspace=ws)
    for _ in range(2):
        out.fill_(float("nan"))
        total.fill_(float("nan"))
        g.fill_(float("nan"))
        ws.view(torch.float64).fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, first[0]) and torch.equal(total, first[1]) and torch.equal(g, first[2])


def composite_yardstick(x0, xh, ms, base, w_sam, w_lap, w_dssim):
    """([total, base, sam, lap, dssim] float64, the composite gradient gc, the SSIM term's gradient s: float64, CPU autograd)"""
    from tmdiff_amd.losses import spectral_spatial_loss_host, ssim_loss_host
    x = xh.double().requires_grad_(True)
    comp = spectral_spatial_loss_host(x0, x, ms, base, w_sam, w_lap)
    gc, = torch.autograd.grad(comp[0], x)
    x = xh.double().requires_grad_(True)
    dssim = ssim_loss_host(x0.double() + ms.double(), x + ms.double())[0]
    s, = torch.autograd.grad(w_dssim * dssim, x)
    total = comp[0].detach() + w_dssim * dssim.detach()
    return torch.stack([total] + [o.detach() for o in comp[1:]] + [dssim.detach()]), gc, s


def composite_inputs(seed, shape):
    """x0, xhat ~ N(0, 1), MS ~ U[0, 1): float32 on the host (the inputs of tests/test_gpu_loss.py)"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g), torch.randn(*shape, generator=g), torch.rand(*shape, generator=g)


@pytest.mark.parametrize("shape", [(3, 4, 17, 33), (1, 8, 16, 36), (1, 4, 23, 39)], ids=lambda s: "x".join(map(str, s)))
def test_accumulate_and_terms_in_ride_on_the_composite_pair(shape):
    """The composite pair writes its four values and gc; the SSIM pair then adds 0.3 * d dssim to gc and composes the values:
    entries 1..3 are copied, entry 4 is the dssim, entry 0 is terms_in[0] + weight * dssim to 1 ulp."""
    from tmdiff_amd import ops
    x0, xh, ms = composite_inputs(41, shape)
    want, gc_ref, s_ref = composite_yardstick(x0, xh, ms, "l1", 0.1, 0.5, 0.3)
    terms4, total4, g = ops.spectral_spatial_loss(cu(x0), cu(xh), cu(ms), "l1", 0.1, 0.5)
    keep4 = terms4.clone()
    a, b = cu(x0) + cu(ms), cu(xh) + cu(ms)             # fp32 sums here: this case checks the mechanics on given images
    alone, _, s_dev = ops.ssim_loss(a, b, weight=0.3)
    gc_dev = g.clone()
    out, total32, g2 = ops.ssim_loss(a, b, weight=0.3, grad=g, accumulate=True, terms_in=terms4)
    assert g2 is g and out.numel() == 5 and torch.equal(terms4, keep4)
    got = out.cpu()
    assert torch.equal(got[1:4], keep4.cpu()[1:4]) and float(got[4]) == float(alone[0])
    exact = float(keep4[0]) + 0.3 * float(got[4])
    assert abs(float(got[0]) - exact) <= math.ulp(exact)
    assert float(total32) == float(np.float32(float(got[0])))
    # g = fl32(gc32 + s) with s in fp64, and the standalone call stored fl32(s): two roundings of 2^-24 apart, per element
    apart = (g.double() - (gc_dev.double() + s_dev.double())).abs()
    assert bool((apart <= 2.0 * EPS * (gc_dev.double().abs() + s_dev.double().abs()) + 1e-40).all())
    # ... and with ms added inside the kernel, in fp64, the whole is the composite definition's gradient
    terms4, _, g = ops.spectral_spatial_loss(cu(x0), cu(xh), cu(ms), "l1", 0.1, 0.5)
    out, total32, g = ops.ssim_loss(cu(x0), cu(xh), weight=0.3, grad=g, accumulate=True, terms_in=terms4, ms=cu(ms))
    for k in range(5):
        assert abs(float(out[k]) - float(want[k])) <= 1e-9 * abs(float(want[k])), (k, out, want)
    worst = assert_gradient(g, gc_ref + s_ref, f"{shape} accumulate", rel=8.0 * EPS, mag=gc_ref.abs() + s_ref.abs())
    print(f"{shape}: accumulated gradient, worst element at {worst:.3f} of its bound")
    with pytest.raises(ValueError, match="accumulate"):
        ops.ssim_loss(a, b, accumulate=True)
    with pytest.raises(ValueError, match="terms_in"):
        ops.ssim_loss(a, b, terms_in=torch.zeros(5, device="cuda", dtype=torch.float64))


@pytest.mark.parametrize("shape", [(3, 4, 17, 33), (2, 8, 16, 32)], ids=lambda s: "x".join(map(str, s)))
def test_module_with_the_ssim_term_against_the_definitions(shape):
    """SpectralSpatialLoss("l1", 0.1, 0.5, w_dssim=0.2) against spectral_spatial_loss_host(...) + 0.2 * ssim_loss_host(x0 + ms,
    xh + ms)[0] (the sums in float64): values to 1e-9 relative, the gradient to the accumulate bound.  w_dssim = 0 is the module
    as it was: the composite pair's bits, a [4] last_terms."""
    from tmdiff_amd import ops
    from tmdiff_amd.losses import SSIMLoss, SpectralSpatialLoss
    x0, xh, ms = composite_inputs(42, shape)
    d = xh.double() - x0.double()
    assert float(d.abs().min()) > 1e-12                  # away from the kink of l1 (the Laplacian's: tests/test_gpu_loss.py)
    want, gc_ref, s_ref = composite_yardstick(x0, xh, ms, "l1", 0.1, 0.5, 0.2)
    mod = SpectralSpatialLoss("l1", 0.1, 0.5, w_dssim=0.2).cuda()
    leaf = cu(xh).requires_grad_(True)
    loss = mod(cu(x0), leaf, cu(ms))
    loss.backward()
    terms = mod.last_terms.cpu()
    assert loss.dtype == torch.float32 and loss.dim() == 0 and terms.dtype == torch.float64 and terms.numel() == 5
    for k in range(5):
        assert abs(float(terms[k]) - float(want[k])) <= 1e-9 * abs(float(want[k])), (k, terms, want)
    assert float(loss) == float(np.float32(float(terms[0])))
    worst = assert_gradient(leaf.grad, gc_ref + s_ref, f"{shape} module", rel=8.0 * EPS, mag=gc_ref.abs() + s_ref.abs())
    print(f"{shape}: terms {[f'{float(v):.12g}' for v in terms]}, worst gradient element at {worst:.3f} of its bound")
    # value-only when x_recon needs no gradient
    loss2 = mod(cu(x0), cu(xh), cu(ms))
    assert not loss2.requires_grad and torch.equal(loss2, loss.detach()) and torch.equal(mod.last_terms.cpu(), terms)
    # w_dssim = 0: the module as it is without the term
    plain = SpectralSpatialLoss("l1", 0.1, 0.5, w_dssim=0.0).cuda()
    leaf0 = cu(xh).requires_grad_(True)
    loss0 = plain(cu(x0), leaf0, cu(ms))
    loss0.backward()
    t_ref, total_ref, g_ref = ops.spectral_spatial_loss(cu(x0), cu(xh), cu(ms), "l1", 0.1, 0.5)
    assert plain.last_terms.numel() == 4 and torch.equal(plain.last_terms, t_ref) and torch.equal(loss0.detach(), total_ref)
    assert torch.equal(leaf0.grad, g_ref)
    # the SSIM term alone, as a module
    alone = SSIMLoss().cuda()
    leaf1 = (cu(xh) + cu(ms)).requires_grad_(True)
    l1 = alone(cu(x0) + cu(ms), leaf1)
    l1.backward()
    o_ref, t32_ref, g1_ref = ops.ssim_loss(cu(x0) + cu(ms), cu(xh) + cu(ms))
    assert l1.dtype == torch.float32 and torch.equal(l1.detach(), t32_ref) and torch.equal(alone.last_terms, o_ref)
    assert torch.equal(leaf1.grad, g1_ref) and alone.last_terms.numel() == 2


def test_captured_step_with_the_ssim_term_replays_like_the_eager_step():
    """model.DDPM with loss_terms = {sam, lap, dssim} and train.hip_graph on the smallest trainer (the configuration of
    tests/test_gpu_loss.py): the two eager warm-up steps, then one capture and two replays.  The same two steps run eagerly from
    the same parameters, optimizer state, learning rates, dropout word, seeds, timesteps and noise leave parameters within 2e-6
    (max difference over max magnitude per tensor) and the same loss; l_dssim is a device scalar in the log beside l_base, l_sam
    and l_lap, refilled by every replay."""
    from oracle.make_golden import TINY, case_inputs
    from tmdiff_amd import ops
    from tmdiff_amd.model import DDPM
    names = ("l_pix", "l_base", "l_sam", "l_lap", "l_dssim")
    opt = {"phase": "train", "gpu_ids": [0], "distributed": False, "path": {"resume": None},
           "model": {"unet": {"channel_multiplier": TINY}, "init_type": "orthogonal",
                     "diffusion": {"loss_type": "l1", "loss_terms": {"sam": 0.1, "lap": 0.5, "dssim": 0.2}}},
           "train": {"optimizer": {"lr": 1e-3}, "max_iter": 100, "hip_graph": True}}
    torch.manual_seed(1)
    m = DDPM(opt)
    assert m.netG.loss_func.w_dssim == 0.2
    m.set_new_noise_schedule({"schedule": "cosine", "n_timestep": 10}, "train")
    m.scheduler.step()                                   # (the warm-up schedule starts at lr = 0, where no weight moves)
    d = {k: v.cuda() for k, v in case_inputs(41, 2, 4, 16).items()}
    d["LR"] = d["MS"]
    gen = torch.Generator().manual_seed(9)
    noises = [torch.randn(2, 4, 16, 16, generator=gen) for _ in range(4)]
    order = []
    m.netG.noise_fn = lambda like: order.pop(0)
    keep_word = ops.DROP_WORD
    try:
        order[:] = noises[:2]
        np.random.seed(1)
        for _ in range(DDPM.GRAPH_WARMUP):
            m.feed_data(dict(d))
            m.optimize_parameters("QB")
            log = m.get_current_log()
            for k in names[1:]:
                assert torch.is_tensor(log[k]) and log[k].is_cuda and log[k].dim() == 0, k
        params = list(m.netG.parameters())
        lr = m.optG.param_groups[0]["lr"]
        snap_p = [p.detach().clone() for p in params]
        snap_s = [{k: v.clone() for k, v in m.optG.state[p].items() if torch.is_tensor(v)} if p in m.optG.state else {} for p in params]
        word = ops.DROP_WORD.clone()
        lrs, logs = [], []
        order[:] = noises[2:]
        np.random.seed(2)
        for _ in range(2):                               # capture + replay, replay
            lrs.append(lr.clone())
            torch.manual_seed(7)                         # (the dropout seeds are drawn when the step is recorded)
            m.feed_data(dict(d))
            m.optimize_parameters("QB")
            log = m.get_current_log()
            for k in names:
                assert torch.is_tensor(log[k]) and log[k].is_cuda and log[k].dim() == 0, k
            logs.append([float(log[k]) for k in names])
        step = next(iter(m._captured.values()))
        assert len(m._captured) == 1 and step.replays == 2 and step.terms is not None and step.terms.numel() == 5
        assert logs[0] != logs[1] and all(math.isfinite(v) and v > 0.0 for v in logs[0] + logs[1])
        for pix, base, sam, lap, dssim in logs:
            assert abs(pix - (base + 0.1 * sam + 0.5 * lap + 0.2 * dssim)) <= 1e-6 * pix
        torch.cuda.synchronize()
        got = [p.detach().clone() for p in params]
        with torch.no_grad():
            for p, sp, ss in zip(params, snap_p, snap_s):
                p.copy_(sp)
                for k, v in ss.items():
                    m.optG.state[p][k].copy_(v)
            ops.DROP_WORD.copy_(word)
        order[:] = noises[2:]
        np.random.seed(2)
        eager = []
        for i in range(2):
            lr.copy_(lrs[i])
            step.load(d)
            m.netG.zero_grad(set_to_none=True)
            torch.manual_seed(7)
            with ops.config.override(train_two_streams=False):
                loss = step._step()
                m.optG.step()
            eager.append([float(loss.detach())] + [float(v) for v in m.netG.loss_func.last_terms[1:]])
        torch.cuda.synchronize()
        print(f"replays {logs}, eager {eager}")
        for u_, v_ in zip(logs, eager):
            assert len(u_) == len(v_) == 5
            for u, v in zip(u_, v_):
                assert abs(u - v) <= 2e-6 * abs(v), (logs, eager)
        worst = 0.0
        for (k, _), a, p in zip(m.netG.named_parameters(), got, params):
            mx, _ = rel_err(a, p.detach())
            worst = max(worst, mx)
            assert mx <= 2e-6, (k, mx)
        moved = sum(int(not torch.equal(a, b)) for a, b in zip(got, snap_p))
        print(f"{moved} tensors moved; worst replay-vs-eager difference {worst:.3e}")
        assert moved > 100
    finally:
        ops.DROP_WORD = keep_word
