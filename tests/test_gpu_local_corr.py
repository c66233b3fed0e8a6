"""The local PAN-correlation loss on the device (csrc/local_corr.hip: value and gradient from one kernel pair) against its
float64 definition, tmdiff_amd.metrics.local_corr_loss, on the same fp32 inputs.

The kernel's tile is th x tw = ops.LOCAL_CORR_TILE (16 x 32) for every window size.  Shapes: [1, 1, win, win], a single window;
[2, 3, th + 1, tw + 1], one past the tile in both axes (four workgroups per image, three of them ragged, the scalar path);
[1, 4, 37, 70], ragged, more than two tiles per axis; [3, 16, 9, 9], C = 16 and B > 1; [1, 4, 19, 36] and [2, 2, 16, 32] (exactly
one tile) take the 16-byte path.  Windows 2, 4 and 8, plus 3 and 7.

Tolerances (derived, none measured).
 * Exact leg: inputs on the grid of multiples of 2^-10 in [0, 1], win in {2, 4, 8}.  Every window sum (means, centred sums) is
   exact in fp64 on both sides in any order (local_corr_refs.grid_pair), so both sides hold the same S_xx, S_pp, S_xp.  Then per
   window: the product S_xx S_pp is correctly rounded on both sides (equal); the square roots are each within 1 ulp of the
   truth (2 u apart at most, u = 2^-53), the divisions add u / 2 each: |rho_dev - rho_host| <= 3 u |rho|.  The hinge
   rho_max - rho adds u / 2 of itself on each side.  Each side then adds `count` terms of one sign pattern in its own order
   (at most (count - 1) u of the sum of magnitudes each) and divides once (u / 2 each).  Together
       |loss_dev - loss_host|         <= u (3 mean|rho| + (2 count + 1) loss)
       |mean_rho_dev - mean_rho_host| <= u (3 + 2 count) mean|rho|
   which is within 8 u count times the value itself whenever 3 mean|rho| <= (6 count - 1) loss and (3 + 2 count) mean|rho| <=
   8 count |mean_rho|: the test picks the first seed whose INPUTS satisfy both (rho around 0.5 by construction) and then
   asserts 8 * 2^-53 * count relative.
 * General leg (random float32): values to 1e-11 absolute -- |rho| <= 1, and the inputs have a per-window spread of at least 2^-8
   of their magnitude (asserted), so a two-pass sum loses at most 8 of its 53 bits to cancellation and the n <= 64 terms add
   64 u: 2^8 * 64 * 2^-53 * a few operations is below 1e-11.  Gradient per element: 4 * 2^-24 |g_ref| + 1e-12 max|g_ref| -- one
   fp32 rounding of a value that agrees in fp64, the floor because an element is a signed sum of up to 3 n window terms (the
   bound of tests/test_gpu_ssim_loss.py, for the same reason).  Accumulated onto a gradient gc: 8 * 2^-24 (|gc| + |s_ref|) plus
   the same floor.  Every window is asserted to lie 1e-6 away from rho_max."""
import math

import numpy as np
import pytest
import torch

from local_corr_refs import U, grid_pair, random_pair, smooth_scene, window_spread

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
TH, TW = 16, 32


def shapes(win):
    return [(1, 1, win, win), (2, 3, TH + 1, TW + 1), (1, 4, 37, 70), (3, 16, 9, 9)]


CASES = [(win, s) for win in (2, 4, 8, 3, 7) for s in shapes(win)] + [(4, (1, 4, 19, 36)), (8, (2, 2, 16, 32))]
EXACT_CASES = [(win, s) for win in (2, 4, 8) for s in shapes(win)] + [(4, (1, 4, 19, 36))]


def case_id(c):
    return f"win{c[0]}-" + "x".join(map(str, c[1]))


def cu(t):
    return None if t is None else t.detach().cuda().contiguous()


def run(x, pan, win, rho_max=None, **kw):
    from tmdiff_amd import ops
    return ops.local_corr_loss(cu(x), cu(pan), win, rho_max, **kw)


_YARD = {}


def yardstick(x, pan, win, rho_max=None, key=None):
    """(loss, mean_rho, grad float64 tensor, rho [B, C, H', W']) from the host definition, made once per key"""
    from tmdiff_amd import metrics
    if key is None or key not in _YARD:
        loss, mean_rho, grad = metrics.local_corr_loss(x, pan, win, rho_max)
        val = (loss, mean_rho, torch.from_numpy(grad), metrics.local_corr(x, pan, win))
        if key is None:
            return val
        _YARD[key] = val
    return _YARD[key]


def general(seed, win, shape, rho_max=None):
    """Random float32 inputs whose windows keep a spread of 2^-8 and stay 1e-6 away from rho_max (the first such seed from `seed`)"""
    for s in range(seed, seed + 20):
        x, pan = random_pair(s, shape)
        want = yardstick(x, pan, win, rho_max, key=("general", s, win, shape, rho_max))
        rmax = 1.0 if rho_max is None else rho_max
        if float(np.abs(want[3] - rmax).min()) > 1e-6:
            assert window_spread(x, win) >= 2.0 ** -8 and window_spread(pan, win) >= 2.0 ** -8
            return x, pan, want
    raise AssertionError("no seed keeps every window 1e-6 away from rho_max")


def assert_gradient(g, want, what, rel=4.0 * EPS, mag=None):
    """per element: rel * mag + 1e-12 max|want| (mag: |want| unless given)"""
    err = (g.cpu().double() - want).abs()
    bound = rel * (want.abs() if mag is None else mag) + 1e-12 * float(want.abs().max())
    worst = float((err / bound.clamp_min(1e-300)).max()) if float(bound.max()) > 0.0 else float(err.max() > 0)
    assert worst <= 1.0, f"{what}: an element is off by {worst:.3f} of its bound"
    return worst


def test_the_tile_is_the_documented_one():
    from tmdiff_amd import ops
    assert ops.LOCAL_CORR_TILE == (TH, TW)


@pytest.mark.parametrize("case", EXACT_CASES, ids=case_id)
def test_exact_leg_on_the_dyadic_grid(case):
    win, shape = case
    from tmdiff_amd import metrics
    count = shape[0] * shape[1] * (shape[2] - win + 1) * (shape[3] - win + 1)
    for seed in range(1, 60):
        x, pan = grid_pair(seed, shape)
        loss, mean_rho, gref, rho = yardstick(x, pan, win)
        mabs = float(np.abs(rho).mean())
        if 3.0 * mabs <= (6 * count - 1) * loss and (3 + 2 * count) * mabs <= 8 * count * abs(mean_rho) and float((1.0 - rho).min()) > 1e-6:
            break
    else:
        raise AssertionError("no seed satisfies the preconditions of the bound")
    assert rho.size == count
    out, total32, g = run(x, pan, win)
    got = out.cpu()
    rel = 8.0 * U * count
    print(f"win={win} {shape} seed {seed}: loss {float(got[0]):.17g} (definition {loss:.17g}), mean rho {float(got[1]):.17g} "
          f"(definition {mean_rho:.17g}), bound {rel:.3e} relative")
    assert abs(float(got[0]) - loss) <= rel * abs(loss)
    assert abs(float(got[1]) - mean_rho) <= rel * abs(mean_rho)
    assert float(total32) == float(np.float32(float(got[0])))
    assert_gradient(g, gref, f"exact win={win} {shape}")
    # the value-only mode gives the gradient mode's values bit for bit
    out2, total2, none = run(x, pan, win, grad=False)
    assert none is None and torch.equal(out2, out) and torch.equal(total2, total32)


@pytest.mark.parametrize("win", [2, 3, 4, 7, 8])
def test_constant_windows_give_the_hosts_exact_zeros(win):
    from tmdiff_amd import metrics
    shape = (2, 3, 37, 70)
    x, pan = random_pair(2, shape)
    flat_band = x.clone()
    flat_band[:, 1] = 0.3
    per = torch.empty(2, device="cuda", dtype=torch.float64)
    out, _, g = run(flat_band[:, 1:2], pan, win, per_image=per)
    assert float(out[0]) == 1.0 and float(out[1]) == 0.0 and bool((per == 0.0).all()) and bool((g == 0.0).all())
    out, _, g = run(x, torch.full_like(pan, 0.7), win)
    assert float(out[0]) == 1.0 and float(out[1]) == 0.0 and bool((g == 0.0).all())
    out, _, g = run(flat_band, pan, win)
    loss, mean_rho, gref, _ = yardstick(flat_band, pan, win)
    assert abs(float(out[0]) - loss) <= 1e-11 and abs(float(out[1]) - mean_rho) <= 1e-11
    assert bool((g[:, 1] == 0.0).all()) and bool((gref[:, 1] == 0.0).all())
    assert_gradient(g, gref, f"constant band win={win}")
    # a patch across a tile corner that is constant only inside some windows: the pixels whose windows all lie inside it get
    # exactly no gradient, and the value is the host's
    patch = x.clone()
    patch[0, 2, 10:10 + 2 * win + 2, 26:26 + 2 * win] = 0.1
    out, _, g = run(patch, pan, win)
    loss, mean_rho, gref, rho = yardstick(patch, pan, win)
    assert int((rho[0, 2] == 0.0).sum()) == (win + 3) * (win + 1)
    assert abs(float(out[0]) - loss) <= 1e-11 and abs(float(out[1]) - mean_rho) <= 1e-11
    inner = (slice(10 + win - 1, 10 + win + 3), slice(26 + win - 1, 26 + win + 1))
    assert bool((g[0, 2][inner] == 0.0).all()) and bool((gref[0, 2][inner] == 0.0).all())
    assert_gradient(g, gref, f"constant patch win={win}")


@pytest.mark.parametrize("rho_max", [None, 0.5], ids=["rho_max-none", "rho_max-0.5"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_value_and_gradient_against_the_float64_definition(case, rho_max):
    win, shape = case
    x, pan, (loss, mean_rho, gref, _) = general(11, win, shape, rho_max)
    out, total32, g = run(x, pan, win, rho_max)
    got = out.cpu()
    what = f"win={win} {shape} rho_max={rho_max}"
    assert abs(float(got[0]) - loss) <= 1e-11 and abs(float(got[1]) - mean_rho) <= 1e-11, (what, got, loss, mean_rho)
    assert float(total32) == float(np.float32(float(got[0]))), what
    worst = assert_gradient(g, gref, what)
    print(f"{what}: loss {float(got[0]):.15g} (definition {loss:.15g}), worst gradient element at {worst:.3f} of its bound")
    # a weight scales the gradient and the fp32 total, not the fp64 values
    out2, total2, g2 = run(x, pan, win, rho_max, weight=0.3)
    assert torch.equal(out2, out)
    assert float(total2) == float(np.float32(0.3 * float(got[0])))
    assert_gradient(g2, 0.3 * gref, what + " weight 0.3")


def test_rho_max_per_band():
    shape, rmax = (2, 3, TH + 1, TW + 1), (0.2, 0.5, 1.0)
    x, pan = random_pair(13, shape)
    loss, mean_rho, gref, rho = yardstick(x, pan, 4, rmax)
    assert min(float(np.abs(rho[:, c] - r).min()) for c, r in enumerate(rmax)) > 1e-6
    out, _, g = run(x, pan, 4, rmax)
    assert abs(float(out[0]) - loss) <= 1e-11 and abs(float(out[1]) - mean_rho) <= 1e-11
    assert_gradient(g, gref, "rho_max per band")
    again = run(x, pan, 4, list(rmax))
    assert torch.equal(again[0], out) and torch.equal(again[2], g)
    with pytest.raises(ValueError, match="rho_max"):
        run(x, pan, 4, (0.2, 0.5))


@pytest.mark.parametrize("shape", [(1, 4, 17, 32), (2, 3, 19, 36), (1, 4, 9, 33)], ids=lambda s: "x".join(map(str, s)))
def test_unaligned_tensors_take_the_scalar_path_and_nothing_is_written_outside(shape):
    """Views one float off a 16-byte boundary inside flat buffers (W % 4 == 0 in two cases: alignment alone decides); the
    gradient's buffer keeps its sentinel on both sides, and the results equal the aligned call's bit for bit."""
    from tmdiff_amd import ops
    x, pan, (loss, mean_rho, gref, _) = general(12, 4, shape)
    pad = 64

    def window(data, fill, like):
        n = math.prod(like)
        flat = torch.full((pad + 1 + n + pad,), fill, device="cuda", dtype=torch.float32)
        view = flat[pad + 1:pad + 1 + n].view(like)
        if data is not None:
            view.copy_(data)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return flat, view

    (_, vx), (_, vp) = window(x, float("nan"), shape), window(pan, float("nan"), tuple(pan.shape))
    gflat, gview = window(None, 777.0, shape)
    out, total32, g = ops.local_corr_loss(vx, vp, 4, grad=gview)
    assert g is gview
    assert abs(float(out[0]) - loss) <= 1e-11 and abs(float(out[1]) - mean_rho) <= 1e-11
    assert_gradient(g, gref, f"{shape} unaligned")
    n = math.prod(shape)
    assert bool((gflat[:pad + 1] == 777.0).all()) and bool((gflat[pad + 1 + n:] == 777.0).all())
    out2, _, g2 = run(x, pan, 4)
    assert torch.equal(out2, out) and torch.equal(g2, g)


@pytest.mark.parametrize("case", [(4, (2, 3, TH + 1, TW + 1)), (4, (1, 4, 19, 36)), (7, (1, 4, 37, 70))], ids=case_id)
def test_accumulate_adds_to_an_existing_gradient(case):
    """g = fl32(gc + s) with s in fp64 against gc + s_ref: 8 * 2^-24 (|gc| + |s_ref|) plus the floor, per element."""
    win, shape = case
    x, pan, (_, _, sref, _) = general(14, win, shape, 0.5)
    gc = 0.01 * torch.randn(*shape, generator=torch.Generator().manual_seed(3))
    g = cu(gc).clone()
    out, _, g2 = run(x, pan, win, 0.5, weight=0.7, grad=g, accumulate=True)
    assert g2 is g
    ref = gc.double() + 0.7 * sref
    worst = assert_gradient(g, ref, f"accumulate {shape}", rel=8.0 * EPS, mag=gc.double().abs() + 0.7 * sref.abs())
    alone = run(x, pan, win, 0.5, weight=0.7)
    assert torch.equal(alone[0], out)
    apart = (g.double() - (cu(gc).double() + alone[2].double())).abs()
    assert bool((apart <= 2.0 * EPS * (cu(gc).double().abs() + alone[2].double().abs()) + 1e-40).all())
    print(f"{shape}: accumulated gradient, worst element at {worst:.3f} of its bound")
    with pytest.raises(ValueError, match="accumulate"):
        run(x, pan, win, accumulate=True)


@pytest.mark.parametrize("case", [(4, (3, 4, 37, 70)), (8, (3, 16, 9, 9)), (3, (2, 3, TH + 1, TW + 1))], ids=case_id)
def test_a_batch_equals_its_samples_bit_for_bit(case):
    """The per-image mean of a batch is the one-image call's, and with weight = B the batch's gradient is the one-image calls'
    (B / (B N1) and 1 / N1 round to the same double)."""
    win, shape = case
    b = shape[0]
    x, pan = random_pair(15, shape)
    per = torch.empty(b, device="cuda", dtype=torch.float64)
    out, _, g = run(x, pan, win, 0.5, weight=float(b), per_image=per)
    for i in range(b):
        one = torch.empty(1, device="cuda", dtype=torch.float64)
        o1, _, g1 = run(x[i:i + 1], pan[i:i + 1], win, 0.5, per_image=one)
        assert torch.equal(one[0], per[i]) and float(o1[1]) == float(one[0])
        assert torch.equal(g1[0], g[i])


def test_per_image_is_one_minus_d_rho():
    from tmdiff_amd import metrics
    shape = (3, 4, 37, 70)
    x, pan = random_pair(16, shape)
    assert window_spread(x, 4) >= 2.0 ** -8 and window_spread(pan, 4) >= 2.0 ** -8
    per = torch.empty(3, device="cuda", dtype=torch.float64)
    out, _, none = run(x, pan, 4, grad=False, per_image=per)
    want = 1.0 - metrics.d_rho(x, pan, 4)
    assert none is None and np.abs(per.cpu().numpy() - want).max() <= 1e-11
    assert abs(float(out[1]) - float(want.mean())) <= 1e-11 and abs(float(out[0]) - (1.0 - float(want.mean()))) <= 1e-11


def test_two_calls_and_two_replays_give_identical_bits():
    from tmdiff_amd import ops
    shape = (3, 8, 19, 36)
    x, pan = (cu(t) for t in random_pair(21, shape))
    first = ops.local_corr_loss(x, pan, 4, 0.5, weight=0.7)
    again = ops.local_corr_loss(x, pan, 4, 0.5, weight=0.7)
    for u, v in zip(first, again):
        assert torch.equal(u, v)
    ws = torch.empty(ops.lib.tmdiff_local_corr_loss_workspace_bytes(*shape, 4), device="cuda", dtype=torch.uint8)
    out, total, g = torch.empty(2, device="cuda", dtype=torch.float64), torch.empty((), device="cuda"), torch.empty_like(x)
    per = torch.empty(3, device="cuda", dtype=torch.float64)
    kw = dict(weight=0.7, grad=g, out=out, total=total, workspace=ws, per_image=per)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # one eager call on the capture stream first
        ops.local_corr_loss(x, pan, 4, 0.5, **kw)
    torch.cuda.current_stream().wait_stream(side)
    keep_per = per.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.local_corr_loss(x, pan, 4, 0.5, **kw)
    for _ in range(2):
        for t in (out, total, g, per):
            t.fill_(float("nan"))
        ws.view(torch.float64).fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, first[0]) and torch.equal(total, first[1]) and torch.equal(g, first[2]) and torch.equal(per, keep_per)


def test_autograd_function_and_module():
    from tmdiff_amd import autograd as A
    from tmdiff_amd.losses import LocalCorrLoss
    shape = (2, 3, TH + 1, TW + 1)
    x, pan = (cu(t) for t in random_pair(22, shape))
    out, total, g = run(x, pan, 4, 0.5)
    leaf = x.clone().requires_grad_(True)
    pan_leaf = pan.clone().requires_grad_(True)
    loss, terms = A.local_corr_loss(leaf, pan_leaf, 4, 0.5)
    assert loss.requires_grad and not terms.requires_grad and loss.dtype == torch.float32 and loss.dim() == 0
    loss.backward()
    assert torch.equal(leaf.grad, g) and pan_leaf.grad is None and torch.equal(terms, out) and torch.equal(loss.detach(), total)
    # value-only when x needs no gradient: the saved gradient's buffer is not made
    loss2, terms2 = A.local_corr_loss(x, pan, 4, 0.5)
    assert not loss2.requires_grad and torch.equal(terms2, out) and torch.equal(loss2, total)
    # only the PAN asks for a gradient: value-only forward, and backward hands out None instead of failing
    pan_only = pan.clone().requires_grad_(True)
    loss3, _ = A.local_corr_loss(x, pan_only, 4, 0.5)
    assert torch.equal(loss3.detach(), total)
    if loss3.requires_grad:
        loss3.backward()
    assert pan_only.grad is None
    mod = LocalCorrLoss(4, 0.5).cuda()
    leaf2 = x.clone().requires_grad_(True)
    l3 = mod(leaf2, pan)
    (3.0 * l3).backward()
    assert torch.equal(leaf2.grad, g * 3.0) and torch.equal(mod.last_terms, out)
    with pytest.raises(ValueError, match="win"):
        LocalCorrLoss(9)


def test_quality_fullres_gains_d_rho_and_keeps_the_other_keys():
    from tmdiff_amd import metrics
    g = torch.Generator().manual_seed(23)
    ps, pan = random_pair(23, (1, 4, 64, 64))
    l_ms = torch.rand(1, 4, 16, 16, generator=g)
    plain = metrics.quality_fullres(cu(l_ms), cu(pan), cu(ps))
    more = metrics.quality_fullres(cu(l_ms), cu(pan), cu(ps), d_rho=True)
    assert list(more) == list(plain) + ["d_rho"] and "d_rho" not in plain
    for k in plain:
        assert torch.equal(plain[k].view(torch.int64), more[k].view(torch.int64)), k
    want = metrics.d_rho(ps, pan, 4)
    assert more["d_rho"].dtype == torch.float64 and tuple(more["d_rho"].shape) == (1,)
    assert abs(float(more["d_rho"][0]) - float(want[0])) <= 1e-11
    hq = metrics.quality_hqnr(cu(ps), cu(pan), cu(ps), "GF2", d_rho=True)
    assert list(hq) == list(metrics.HQNR_FIELDS) + ["d_rho"] and abs(float(hq["d_rho"][0]) - float(want[0])) <= 1e-11


def test_structure_refine_on_the_device_follows_the_host_iterates():
    """[1, 4, 48, 48] (local_corr_refs.smooth_scene), step = 1e-3, 4 iterations, 4 x 4 windows.

    One step, rigorously: from the SAME iterate f (the device's, fp32) the device forms G = fl32(step N grad) and f' = fl32(f - G)
    where the host forms f - step N grad in fp64.  The gradient agrees to 4 * 2^-24 |G| + 1e-12 max|G| per element (the bound of
    the general leg) and the subtraction adds one fp32 rounding, 2^-24 |f'|:
        per_step = 4 * 2^-24 |G| + 1e-12 max|G| + 2^-24 |f'|        per element.
    Four steps against the host's own fp64 iterates: the per-step bound times iters, taken with max|G| and max|f| over the run
    (6.2e-8 per step here: max|G| = 0.052, max|f| = 0.83), i.e. the errors of the steps add and are not amplified.  That is the
    behaviour of a descent step whose iterates approach each other; the worst-case Lipschitz constant of the step map (step * n *
    (5 sqrt(n) + 2) / min S_xx, about 12 here) is not a usable bound and is not used.
    So the one-step assertions are the rigorous part; the summed bound is an assumption about this scene (no amplification),
    and a failure of it alone, with every one-step assertion holding, points at the scene's conditioning, not at the kernel."""
    from tmdiff_amd import metrics, tiling
    x, pan = smooth_scene()
    step, n_win = 1e-3, 4 * 45 * 45
    f_dev = cu(x)
    host = x.double().numpy()
    pan64 = pan.double().numpy()
    g_max = f_max = 0.0
    for it in range(4):
        before = f_dev.cpu().double().numpy()
        G = metrics.local_corr_loss(before, pan64, 4, None, step * n_win)[2]
        one = before - G
        nxt = tiling.structure_refine(f_dev, cu(pan), step, iters=1)
        assert nxt is not f_dev and nxt.dtype == torch.float32
        bound = 4.0 * EPS * np.abs(G) + 1e-12 * np.abs(G).max() + EPS * np.abs(one)
        worst = float((np.abs(nxt.cpu().double().numpy() - one) / bound).max())
        assert worst <= 1.0, f"step {it}: an element is off by {worst:.3f} of the one-step bound"
        Gh = metrics.local_corr_loss(host, pan64, 4, None, step * n_win)[2]
        host = host - Gh
        g_max, f_max = max(g_max, float(np.abs(Gh).max())), max(f_max, float(np.abs(host).max()))
        f_dev = nxt
    whole = tiling.structure_refine(cu(x), cu(pan), step, iters=4)
    assert torch.equal(whole, f_dev)                                     # four steps in one call are the four calls
    total = 4 * (4.0 * EPS * g_max + 1e-12 * g_max + EPS * f_max)
    apart = float(np.abs(whole.cpu().double().numpy() - host).max())
    print(f"after 4 steps the device is {apart:.3e} from the host iterates; bound {total:.3e}")
    assert apart <= total
    assert metrics.local_corr_loss(whole.cpu(), pan, 4)[0] < 0.25       # 0.576 at the start (tests/test_local_corr_host.py)
    # in place, and with the Landweber step in between
    buf = cu(x).clone()
    assert tiling.structure_refine(buf, cu(pan), step, iters=4, out=buf) is buf and torch.equal(buf, whole)
    lr = cu(torch.from_numpy(metrics.mtf_degrade(x.double().numpy(), metrics.band_gains("GF2", 4), 4)).float())
    both = tiling.structure_refine(cu(x), cu(pan), step, iters=1, lr_ms=lr, sensor="GF2")
    by_hand = tiling.consistency_refine(tiling.structure_refine(cu(x), cu(pan), step, iters=1), lr, "GF2", 4, 1)
    assert torch.equal(both, by_hand)


def test_structure_refine_can_be_captured_after_a_first_call():
    from tmdiff_amd import tiling
    x, pan = (cu(t) for t in smooth_scene())
    want = tiling.structure_refine(x, pan, 1e-3, iters=2, rho_max=0.9)
    buf = x.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        tiling.structure_refine(x, pan, 1e-3, iters=2, rho_max=0.9, out=buf)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tiling.structure_refine(x, pan, 1e-3, iters=2, rho_max=0.9, out=buf)
    buf.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(buf, want)


def test_unsupported_extents_raise_and_launch_nothing():
    import collections
    from tmdiff_amd import ops
    x, pan = (cu(t) for t in random_pair(31, (1, 4, 16, 16)))
    keep, ops.COUNTS = ops.COUNTS, collections.Counter()
    try:
        with pytest.raises(ValueError, match="win=9"):
            ops.local_corr_loss(x, pan, 9)
        wide = torch.rand(1, 17, 16, 16, device="cuda")
        with pytest.raises(ValueError, match="C=17"):
            ops.local_corr_loss(wide, pan, 4)
        with pytest.raises(ValueError, match="not supported"):
            ops.local_corr_loss(x[..., :3, :].contiguous(), pan[..., :3, :].contiguous(), 4)
        with pytest.raises(ValueError, match="pan"):
            ops.local_corr_loss(x, x, 4)
        with pytest.raises(ValueError, match="weight"):
            ops.local_corr_loss(x, pan, 4, weight=-1.0)
        assert sum(ops.COUNTS.values()) == 0
    finally:
        ops.COUNTS = keep
    assert not ops.local_corr_loss_supported(1, 4, 16, 16, 9) and not ops.local_corr_loss_supported(1, 17, 16, 16, 4)
    assert not ops.local_corr_loss_supported(1, 4, 3, 16, 4) and ops.local_corr_loss_supported(1, 16, 8, 8, 8)


def test_val_dataset_reports_d_rho_for_the_network_and_the_baselines(tmp_path):
    """A stub trainer whose result is 0.6 MS + 0.4 PAN: d_rho_<dataset> is the mean over the items of metrics.d_rho(SR, PAN)
    (4 x 4 windows) in both protocols, d_rho_<dataset>@exp that of the interpolated MS, and every other key keeps its bits."""
    from tmdiff_amd import evaluate, metrics

    class Trainer:
        keys = ("MS", "PAN", "LR")

        def feed_data(self, d):
            self.d = d

        def test(self, continous=False, prompt="QB"):
            fused = (0.6 * self.d["MS"] + 0.4 * self.d["PAN"]).clamp(0, 1)
            self.SR = torch.cat([torch.zeros_like(fused), fused])              # a stack; the last image is the result

        def get_current_visuals(self):
            return {"SR": self.SR, **{k: self.d[k] for k in self.keys}}

    loader, want, want_exp = [], [], []
    for seed in (41, 42):
        ms, pan = random_pair(seed, (1, 4, 64, 64))
        loader.append({"MS": cu(ms), "PAN": cu(pan), "LR": cu(ms[..., 2::4, 2::4])})
        sr = (0.6 * cu(ms) + 0.4 * cu(pan)).clamp(0, 1).cpu()
        want.append(float(metrics.d_rho(sr, pan, 4)[0]))
        want_exp.append(float(metrics.d_rho(ms, pan, 4)[0]))
    kw = dict(log=lambda *a: None, full_resolution=True)
    for protocol in ("qnr", "hqnr"):
        plain = evaluate.val_dataset(Trainer(), "QB", loader, str(tmp_path / f"{protocol}0"), protocol=protocol, baselines=("exp",), **kw)
        more = evaluate.val_dataset(Trainer(), "QB", loader, str(tmp_path / f"{protocol}1"), protocol=protocol, baselines=("exp",),
                                    d_rho=True, **kw)
        assert set(more) == set(plain) | {"d_rho_QB", "d_rho_QB@exp"} and "d_rho_QB" not in plain
        for k in plain:
            assert k == "sec_per_item" or more[k] == plain[k], k
        assert abs(more["d_rho_QB"] - sum(want) / 2) <= 1e-11 and abs(more["d_rho_QB@exp"] - sum(want_exp) / 2) <= 1e-11
    alone = evaluate.val_dataset(Trainer(), "QB", loader, str(tmp_path / "alone"), d_rho=True, **kw)
    assert set(alone) == {"d_lambda_QB", "d_s_QB", "qnr_QB", "d_rho_QB", "sec_per_item"} and alone["d_rho_QB"] == more["d_rho_QB"]
    with pytest.raises(ValueError, match="d_rho"):
        evaluate.val_dataset(Trainer(), "QB", loader, str(tmp_path / "bad"), log=lambda *a: None, d_rho=True)


def test_fuse_scene_runs_structure_refine_on_the_stitched_scene():
    """fuse_scene(structure=...) is fuse_scene followed by structure_refine against the PAN -- with lr_ms and the sensor when
    the sensor is given -- and the post-hoc consistency option comes after it."""
    from oracle import unet_ref as Un
    from oracle.make_golden import TINY
    from tmdiff_amd import tiling
    from tmdiff_amd.Hyper_unet_general import WavBEST
    from tmdiff_amd.diffusion_general import GeneralDiffusion
    ref = Un.fill_weights_(Un.WavBESTRef(channels=TINY)).eval()
    net = WavBEST(channels=TINY)
    net.load_state_dict(ref.state_dict())
    net = net.cuda().eval()
    diff = GeneralDiffusion(net, "l1", noise_fn=lambda like: torch.randn(like.shape, dtype=torch.float32)).cuda()
    diff.set_new_noise_schedule({"schedule": "cosine", "n_timestep": 1000}, "cuda")
    g = torch.Generator().manual_seed(70)
    lr_ms, pan = torch.rand(1, 8, 8, 12, generator=g).cuda(), torch.rand(1, 1, 32, 48, generator=g).cuda()
    kw = dict(tile=32, method="dpmsolver", steps=3, overlap=16)
    opts = {"step": 1e-3, "iters": 2, "win": 4, "rho_max": 0.9}

    def fuse(**more):
        torch.manual_seed(11)
        return tiling.fuse_scene(diff, lr_ms, pan, "WV3", **kw, **more)

    plain = fuse()
    by_hand = tiling.structure_refine(plain, pan, 1e-3, iters=2, win=4, rho_max=0.9)
    assert not torch.equal(by_hand, plain)
    assert torch.equal(fuse(structure=opts), by_hand) and torch.equal(fuse(structure=None), plain)
    with_ms = tiling.structure_refine(plain, pan, 1e-3, iters=2, win=4, rho_max=0.9, lr_ms=lr_ms, sensor="WV3")
    then = tiling.consistency_refine(with_ms, lr_ms, "WV3", 4, iters=1)
    assert not torch.equal(with_ms, by_hand)
    assert torch.equal(fuse(structure=opts, sensor="WV3", consistency={"iters": 1}), then)
