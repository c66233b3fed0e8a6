"""The composite finetune loss on the device (csrc/loss.hip: base + w_sam * SAM + w_lap * LAP, value and gradient from one
kernel pair) against its float64 definition, tmdiff_amd.losses.spectral_spatial_loss_host, on the same fp32 inputs with the
gradient from torch autograd on the CPU.

The kernel's tile is 16 x 32 (a halo of 2 for the Laplacian of the Laplacian's sign).  Shapes: H from 3, 5, 15, 16, 17, 19 and W
from 3, 5, 31, 32, 33, 35 -- one interior pixel, then each tile extent minus 1, exactly, plus 1, plus 3 -- and the multiples of 4
among them plus 8, 36 and 64 for the 16-byte path; nothing beyond two tiles per axis.

Tolerances.  Values: 1e-9 relative on each of the four outputs (fixed-order fp64 sums of fewer than 1e5 terms and libm's few
ulps stay at 1e-13).  Gradient: per element 4 * 2^-24 * |g_ref| + 1e-30, one fp32 rounding of a value that agrees in fp64; the
inputs are continuous random numbers and every case asserts that no d or Lap d (nor |d| - 1 for smooth l1) lies within 1e-12 of
a kink, so the sign the two sides take is the same."""
import math

import numpy as np
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 3, 3), (3, 4, 5, 5), (1, 4, 15, 31), (1, 8, 16, 32), (3, 4, 17, 33), (1, 16, 19, 35), (3, 8, 3, 35), (1, 4, 19, 3),
          (1, 16, 5, 8), (3, 1, 16, 36), (1, 4, 32, 64), (1, 8, 17, 5)]
KINDS = ("l1", "l2", "smooth_l1")
TERMS = [(0.0, 0.0), (0.3, 0.0), (0.0, 0.7), (0.1, 0.5)]
GTOL = 4.0 * 2.0 ** -24


def inputs(seed, shape):
    """x0, xhat ~ N(0, 1) (|d| on both sides of 1), MS ~ U[0, 1): float32 on the host"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g), torch.randn(*shape, generator=g), torch.rand(*shape, generator=g)


def yardstick(x0, xh, ms, base, w_sam, w_lap):
    """([total, base, sam, lap] float64, dL/dxhat float64) from the host definition and CPU autograd"""
    from tmdiff_amd.losses import spectral_spatial_loss_host
    x = xh.double().requires_grad_(True)
    out = spectral_spatial_loss_host(x0, x, ms, base, w_sam, w_lap)
    g, = torch.autograd.grad(out[0], x)
    return torch.stack([o.detach() for o in out]), g


_YARD = {}


def shared_yardstick(seed, shape, base, w_sam, w_lap):
    key = (seed, shape, base, w_sam, w_lap)
    if key not in _YARD:
        x0, xh, ms = inputs(seed, shape)
        _YARD[key] = (x0, xh, ms) + yardstick(x0, xh, ms, base, w_sam, w_lap)
    return _YARD[key]


def laplacian(d):
    h, w = d.shape[-2:]
    return sum(d[..., 1 + i:h - 1 + i, 1 + j:w - 1 + j] for i in (-1, 0, 1) for j in (-1, 0, 1)) - 9.0 * d[..., 1:-1, 1:-1]


def assert_away_from_kinks(x0, xh, base, w_lap):
    d = xh.double() - x0.double()
    assert float(d.abs().min()) > 1e-12
    if base == "smooth_l1":
        assert float((d.abs() - 1.0).abs().min()) > 1e-12
    if w_lap != 0.0:
        assert float(laplacian(d).abs().min()) > 1e-12


def cu(t):
    return None if t is None else t.detach().cuda().contiguous()


def run(x0, xh, ms, base, w_sam, w_lap, **kw):
    from tmdiff_amd import ops
    return ops.spectral_spatial_loss(cu(x0), cu(xh), cu(ms), base, w_sam, w_lap, **kw)


def assert_values(terms, total32, want, what):
    got = terms.cpu()
    for k, name in enumerate(("total", "base", "sam", "lap")):
        err = abs(float(got[k]) - float(want[k]))
        assert err <= 1e-9 * abs(float(want[k])), (what, name, float(got[k]), float(want[k]))
    assert float(total32) == float(np.float32(float(got[0]))), what


def assert_gradient(g, want, what):
    err = (g.cpu().double() - want).abs()
    bound = GTOL * want.abs() + 1e-30
    worst = float((err / bound).max())
    assert worst <= 1.0, f"{what}: an element is off by {worst:.3f} of its bound (4 * 2^-24 |g_ref| + 1e-30)"
    return worst


@pytest.mark.parametrize("w_sam,w_lap", TERMS, ids=["base", "sam", "lap", "all"])
@pytest.mark.parametrize("base", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_value_and_gradient_against_the_float64_definition(shape, base, w_sam, w_lap):
    x0, xh, ms, want, gwant = shared_yardstick(11, shape, base, w_sam, w_lap)
    assert_away_from_kinks(x0, xh, base, w_lap)
    terms, total32, g = run(x0, xh, ms, base, w_sam, w_lap)
    what = f"{shape} {base} w_sam={w_sam} w_lap={w_lap}"
    assert_values(terms, total32, want, what)
    worst = assert_gradient(g, gwant, what)
    print(f"{what}: values {[f'{float(v):.12g}' for v in terms.cpu()]}, worst gradient element at {worst:.3f} of its bound")
    if w_sam == 0.0:
        assert float(terms[2]) == 0.0
    if w_lap == 0.0:
        assert float(terms[3]) == 0.0


@pytest.mark.parametrize("shape", [(1, 4, 17, 32), (3, 8, 19, 36), (1, 4, 5, 33)], ids=lambda s: "x".join(map(str, s)))
def test_unaligned_tensors_take_the_scalar_path_and_nothing_is_written_outside(shape):
    """Windows one float off a 16-byte boundary inside flat buffers (W % 4 == 0 in two cases: alignment alone decides); the
    gradient's buffer keeps its sentinel on both sides, and the values equal the aligned call's bit for bit."""
    from tmdiff_amd import ops
    x0, xh, ms, want, gwant = shared_yardstick(12, shape, "smooth_l1", 0.1, 0.5)
    n, pad = math.prod(shape), 64

    def window(data, fill):
        flat = torch.full((pad + 1 + n + pad,), fill, device="cuda", dtype=torch.float32)
        view = flat[pad + 1:pad + 1 + n].view(shape)
        if data is not None:
            view.copy_(data)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return flat, view

    (_, a), (_, b), (_, m) = window(x0, float("nan")), window(xh, float("nan")), window(ms, float("nan"))
    gflat, gview = window(None, 777.0)
    terms, total32, g = ops.spectral_spatial_loss(a, b, m, "smooth_l1", 0.1, 0.5, grad=gview)
    assert g is gview
    assert_values(terms, total32, want, f"{shape} unaligned")
    assert_gradient(g, gwant, f"{shape} unaligned")
    assert bool((gflat[:pad + 1] == 777.0).all()) and bool((gflat[pad + 1 + n:] == 777.0).all())
    t2, _, g2 = run(x0, xh, ms, "smooth_l1", 0.1, 0.5)
    assert torch.equal(t2, terms) and torch.equal(g2, g)


# ---- exact cases: integer-valued data, where the fp64 sums are exact -----------------------------------------------------------
def int_tensor(seed, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


@pytest.mark.parametrize("base", KINDS)
def test_equal_pixels_get_no_base_and_no_laplacian_gradient(base):
    """d is integer-valued and non-zero in one block only.  Where d and its 5 x 5 neighbourhood are 0, Lap d is 0 on the 3 x 3
    neighbourhood: sign 0, no gradient from either term; the values are exact sums."""
    shape = (2, 4, 20, 40)
    x0 = int_tensor(1, shape, -3, 3)
    d = torch.zeros(shape)
    d[:, :, 2:9, 3:15] = int_tensor(2, (2, 4, 7, 12), -2, 2)
    xh = x0 + d
    terms, total32, g = run(x0, xh, None, base, 0.0, 0.5)
    want, gwant = yardstick(x0, xh, None, base, 0.0, 0.5)
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(terms).all())
    g = g.cpu()
    far = torch.ones(shape, dtype=torch.bool)
    far[:, :, 0:11, 1:17] = False
    assert float(g[far].abs().max()) == 0.0 and float(g[~far].abs().max()) > 0.0
    for k in range(4):
        assert abs(float(terms[k]) - float(want[k])) <= 1e-15 * abs(float(want[k])), k
    assert torch.equal(g, gwant.float())


def test_a_patch_with_zero_laplacian_contributes_sign_zero():
    """d is a linear ramp (Lap d = 0 exactly, in integers) except in one corner block: the Laplacian term's value comes from
    the block's surroundings alone, and away from it the gradient is the base term's."""
    shape = (1, 4, 16, 32)
    yy, xx = torch.meshgrid(torch.arange(16.0), torch.arange(32.0), indexing="ij")
    d = (2.0 * yy - 3.0 * xx + 5.0).expand(shape).clone()
    d[:, :, 0:3, 0:4] += int_tensor(3, (1, 4, 3, 4), 1, 2)
    x0 = int_tensor(4, shape, -4, 4)
    terms, _, g = run(x0, x0 + d, None, "l2", 0.0, 1.0)
    want, gwant = yardstick(x0, x0 + d, None, "l2", 0.0, 1.0)
    assert float(terms[3]) == float(want[3]) and float(want[3]) > 0.0
    base_only = (2.0 * d.double() / d.numel()).float()        # n = 2048: exact
    g = g.cpu()
    assert torch.equal(g[:, :, 5:, :], base_only[:, :, 5:, :]) and torch.equal(g[:, :, :, 6:], base_only[:, :, :, 6:])
    assert not torch.equal(g[:, :, :5, :6], base_only[:, :, :5, :6])
    assert torch.equal(g, gwant.float())


def test_degenerate_spectra_get_an_exactly_zero_sam_gradient():
    """Integer band vectors: u parallel to v (v = 3 u), antiparallel (v = -2 u), equal, u = 0, v = 0, both 0, and one honest
    pixel.  The l2 base gradient 2 d / n is exact in fp32 here (n = 64), so the stored gradient equals it bit for bit wherever
    the sam gradient is exactly 0; everything is finite."""
    u = torch.tensor([[1.0, 2.0, 3.0, 1.0]] * 8)
    v = torch.tensor([[3.0, 6.0, 9.0, 3.0], [-2.0, -4.0, -6.0, -2.0], [1.0, 2.0, 3.0, 1.0], [1.0, 2.0, 3.0, 1.0], [0.0] * 4, [0.0] * 4,
                      [0.0, 1.0, 0.0, 0.0], [5.0, 10.0, 15.0, 5.0]])
    u[3] = 0.0
    u[5] = 0.0
    shape = (2, 4, 1, 8)
    ms = int_tensor(5, shape, -3, 3)
    x0 = u.t().reshape(1, 4, 1, 8).expand(shape) - ms
    xh = v.t().reshape(1, 4, 1, 8).expand(shape) - ms
    terms, total32, g = run(x0, xh, ms, "l2", 2.0, 0.0)
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(terms).all()) and bool(torch.isfinite(total32))
    base_only = (2.0 * (xh - x0).double() / 64.0).float()
    g = g.cpu()
    flat = [0, 1, 2, 3, 4, 5, 7]
    assert torch.equal(g[..., flat], base_only[..., flat])
    assert not torch.equal(g[..., 6], base_only[..., 6])
    # angles: 0, pi, 0, 0, 0, 0, the honest one, 0
    honest = math.atan2(math.sqrt(15.0 * 1.0 - 4.0), 2.0)
    assert abs(float(terms[2]) - (math.pi + honest) / 8.0) <= 1e-15
    want, gwant = yardstick(x0, xh, ms, "l2", 2.0, 0.0)
    assert_gradient(g, gwant, "degenerate spectra")


def test_tiny_spectra_saturate_instead_of_overflowing():
    """|v| of 1e-42 (a subnormal fp32): the gradient's magnitude 1 / |v| is beyond fp32; what is stored is finite."""
    shape = (1, 2, 3, 4)
    x0 = torch.tensor([1e-42, 2e-42]).view(1, 2, 1, 1).expand(shape).contiguous()
    xh = torch.tensor([2e-42, -1e-42]).view(1, 2, 1, 1).expand(shape).contiguous()
    terms, total32, g = run(x0, xh, torch.zeros(shape), "l1", 1.0, 0.0)
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(terms).all())
    assert float(g.abs().max()) > 1e30 and abs(float(terms[2]) - math.pi / 2) <= 1e-6


# ---- reproducibility, capture, value-only mode ----------------------------------------------------------------------------------
def test_two_calls_and_two_replays_give_identical_bits():
    from tmdiff_amd import ops
    x0, xh, ms = (cu(t) for t in inputs(21, (3, 8, 19, 36)))
    first = ops.spectral_spatial_loss(x0, xh, ms, "smooth_l1", 0.1, 0.5)
    again = ops.spectral_spatial_loss(x0, xh, ms, "smooth_l1", 0.1, 0.5)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    ws = torch.empty(ops.lib.tmdiff_loss_workspace_bytes(3, 8, 19, 36, 1), device="cuda", dtype=torch.uint8)
    terms, total, g = torch.empty(4, device="cuda", dtype=torch.float64), torch.empty((), device="cuda"), torch.empty_like(xh)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # one eager call on the capture stream first
        ops.spectral_spatial_loss(x0, xh, ms, "smooth_l1", 0.1, 0.5, grad=g, terms=terms, total=total, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.spectral_spatial_loss(x0, xh, ms, "smooth_l1", 0.1, 0.5, grad=g, terms=terms, total=total, workspace=ws)
    for _ in range(2):
        terms.fill_(float("nan"))
        total.fill_(float("nan"))
        g.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(terms, first[0]) and torch.equal(total, first[1]) and torch.equal(g, first[2])


@pytest.mark.parametrize("shape", [(3, 4, 17, 33), (1, 8, 16, 32)], ids=lambda s: "x".join(map(str, s)))
def test_value_only_mode_writes_no_gradient(shape):
    from tmdiff_amd import autograd as A
    x0, xh, ms = (cu(t) for t in inputs(22, shape))
    terms, total, g = run(x0, xh, ms, "l1", 0.1, 0.5)
    g.fill_(float("nan"))                               # the buffer the gradient mode wrote, poisoned
    keep = g.clone()
    terms2, total2, none = run(x0, xh, ms, "l1", 0.1, 0.5, grad=False)
    torch.cuda.synchronize()
    assert none is None and torch.equal(terms2, terms) and torch.equal(total2, total)
    assert torch.equal(g.view(torch.int32), keep.view(torch.int32))
    # the autograd function selects it when xhat needs no gradient, and saves g when it does
    loss, t3 = A.spectral_spatial_loss(x0, xh, ms, "l1", 0.1, 0.5)
    assert not loss.requires_grad and torch.equal(t3, terms) and torch.equal(loss, total)
    leaf = xh.clone().requires_grad_(True)
    loss, t4 = A.spectral_spatial_loss(x0, leaf, ms, "l1", 0.1, 0.5)
    assert loss.requires_grad and not t4.requires_grad
    (3.0 * loss).backward()
    _, _, gref = run(x0, xh, ms, "l1", 0.1, 0.5)
    assert torch.equal(leaf.grad, gref * 3.0)


@pytest.mark.parametrize("base,ref", [("l1", torch.nn.L1Loss), ("l2", torch.nn.MSELoss), ("smooth_l1", torch.nn.SmoothL1Loss)])
def test_zero_weights_match_torchs_loss_on_the_device(base, ref):
    """All weights zero: the module still goes through the kernel and equals torch's fp32 loss module -- 1e-6 relative on the
    value, 2e-7 relative per gradient element.  n = 2048 is a power of two, so torch's 1 / n and 2 / n are exact: its gradient
    carries the rounding of d and one product (2 * 2^-24), ours one rounding (2^-24)."""
    from tmdiff_amd.losses import SpectralSpatialLoss
    x0, xh, ms = (cu(t) for t in inputs(23, (2, 4, 16, 16)))
    mod = SpectralSpatialLoss(base, 0.0, 0.0).cuda()
    a = xh.clone().requires_grad_(True)
    b = xh.clone().requires_grad_(True)
    got = mod(x0, a, ms)
    want = ref()(x0, b)
    got.backward()
    want.backward()
    assert got.dtype == torch.float32 and got.dim() == 0
    assert abs(float(got) - float(want)) <= 1e-6 * abs(float(want))
    err = (a.grad.double() - b.grad.double()).abs()
    assert bool((err <= 2e-7 * b.grad.double().abs()).all()), float((err / b.grad.double().abs().clamp_min(1e-300)).max())
    assert float(mod.last_terms[1]) == float(mod.last_terms[0]) and float(mod.last_terms[2]) == 0.0 == float(mod.last_terms[3])


# ---- through the network ----------------------------------------------------------------------------------------------------------
def _tiny_diffusion(loss_terms):
    from oracle import unet_ref as U
    from oracle.make_golden import TINY
    from tmdiff_amd.Hyper_unet_general import WavBEST
    from tmdiff_amd.diffusion_general import GeneralDiffusion
    net = U.fill_weights_(WavBEST(channels=TINY)).cuda().eval()          # eval: dropout off
    diff = GeneralDiffusion(net, "l1", loss_terms=loss_terms).cuda()
    diff.set_loss("cuda")
    diff.set_new_noise_schedule({"schedule": "cosine", "n_timestep": 1000}, "cuda")
    return net, diff


def test_parameter_gradients_through_the_network_follow_the_yardstick_gradient():
    """p_losses_with(...).sum().backward() with loss_terms = {sam: 0.1, lap: 0.5} against a second run of the same forward whose
    output receives the yardstick's gradient (float64 on the CPU, cast to fp32): the same backward kernels on two gradients one
    rounding apart, so every parameter gradient agrees to 1e-5 relative L2; a tensor without a gradient has none in either."""
    from oracle.make_golden import case_inputs, randn
    from tmdiff_amd import ops
    from tmdiff_amd.losses import SpectralSpatialLoss
    net, diff = _tiny_diffusion({"sam": 0.1, "lap": 0.5})
    assert isinstance(diff.loss_func, SpectralSpatialLoss)
    d = {k: cu(v) for k, v in case_inputs(31, 2, 4, 16).items()}
    times = np.array([300, 700])
    t_dev = torch.from_numpy(times).view(2, 1).cuda()
    a_dev = torch.tensor(diff.sqrt_alphas_cumprod_prev[times], dtype=torch.float32).cuda()
    noise = cu(randn(32, 2, 4, 16, 16))
    net.zero_grad(set_to_none=True)
    loss = diff.p_losses_with(d, "QB", t_dev, a_dev, noise).sum()
    loss.backward()
    got = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in net.named_parameters()}
    terms = diff.loss_func.last_terms.cpu()
    # the second run
    net.zero_grad(set_to_none=True)
    x_noisy = ops.q_sample(d["Res"], noise, a_dev)
    x_recon = net.forward_train(x_noisy, t_dev, d["PAN"], d["MS"], "QB")
    want, gwant = yardstick(d["Res"].cpu(), x_recon.detach().cpu(), d["MS"].cpu(), "l1", 0.1, 0.5)
    x_recon.backward(gwant.float().cuda())
    assert abs(float(loss) - float(want[0])) <= 1e-6 * abs(float(want[0]))
    for k in range(4):
        assert abs(float(terms[k]) - float(want[k])) <= 1e-9 * abs(float(want[k])), k
    with_grad, worst = 0, 0.0
    for k, p in net.named_parameters():
        if p.grad is None:
            assert got[k] is None, k
            continue
        assert got[k] is not None, k
        with_grad += 1
        _, l2 = rel_err(got[k], p.grad)
        worst = max(worst, l2)
        assert l2 <= 1e-5, (k, l2)
    print(f"{with_grad} parameter gradients, worst relative L2 difference {worst:.3e}")
    assert with_grad > 100


def test_captured_step_with_the_terms_on_replays_like_the_eager_step():
    """model.DDPM with loss_terms and train.hip_graph on the smallest trainer: the two eager warm-up steps, then one capture and
    two replays (forward, loss kernel, backward, FusedAdamW).  The same two steps run eagerly from the same parameters, optimizer
    state, learning rates, dropout word, seeds, timesteps and noise leave parameters within 2e-6 (max difference over max
    magnitude per tensor: the bound of tests/test_gpu_configs.py for replay against eager) and the same loss; l_base, l_sam and
    l_lap are device scalars in the log and refilled by every replay."""
    from oracle.make_golden import TINY, case_inputs
    from tmdiff_amd import ops
    from tmdiff_amd.model import DDPM
    opt = {"phase": "train", "gpu_ids": [0], "distributed": False, "path": {"resume": None},
           "model": {"unet": {"channel_multiplier": TINY}, "init_type": "orthogonal",
                     "diffusion": {"loss_type": "l1", "loss_terms": {"sam": 0.1, "lap": 0.5}}},
           "train": {"optimizer": {"lr": 1e-3}, "max_iter": 100, "hip_graph": True}}
    torch.manual_seed(1)
    m = DDPM(opt)
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
            for k in ("l_base", "l_sam", "l_lap"):
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
            for k in ("l_pix", "l_base", "l_sam", "l_lap"):
                assert torch.is_tensor(log[k]) and log[k].is_cuda and log[k].dim() == 0, k
            logs.append([float(log[k]) for k in ("l_pix", "l_base", "l_sam", "l_lap")])
        step = next(iter(m._captured.values()))
        assert len(m._captured) == 1 and step.replays == 2 and step.terms is not None
        assert logs[0] != logs[1] and all(math.isfinite(v) and v > 0.0 for v in logs[0] + logs[1])
        for pix, base, sam, lap in logs:
            assert abs(pix - (base + 0.1 * sam + 0.5 * lap)) <= 1e-6 * pix
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
        for a, b in zip(logs, eager):
            for u, v in zip(a, b):
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
