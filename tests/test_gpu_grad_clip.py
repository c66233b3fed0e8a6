"""Global-norm gradient clipping inside the one-launch AdamW step (tmdiff_amd.optim.FusedAdamW(max_grad_norm=...)): the
device-side norm (tmdiff_multi_sqnorm_partial / _finish) against fp64 on the host, the gradient-scaled AdamW kernel
(tmdiff_multi_adamw_scaled) against the plain one on pre-scaled gradients bit for bit and against clip_grad_norm_ +
torch.optim.AdamW in fp64, the skipped step, two parameter groups, a HIP-graph replay and the trainer option."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LR, WD = 1e-3, 1e-2


def _chunk():
    from tmdiff_amd._lib import lib
    return lib.tmdiff_multi_axpby_chunk()


def _lengths():
    c = _chunk()
    return [1, 3, c - 1, c, c + 1, 3 * c + 7] + [5 + (37 * k) % 63 for k in range(40)]       # 40 tensors of 5..67 elements


def _off_by_one_float(values):
    """`values` in a tensor whose base address is one float past a 16-byte boundary."""
    buf = torch.empty(values.numel() + 1, device="cuda")
    view = buf[1:]
    view.copy_(values)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def make_params(seed=0):
    """The tensor list of every test here: lengths around the chunk size, 40 small tensors, one tensor (longer than a chunk)
    whose base address is not 16-byte aligned, and -- last -- one parameter that never gets a gradient."""
    g = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(n, generator=g).cuda()) for n in _lengths()]
    params.append(torch.nn.Parameter(_off_by_one_float(torch.randn(_chunk() + 9, generator=g).cuda())))
    params.append(torch.nn.Parameter(torch.randn(9, generator=g).cuda()))
    return params


def set_grads(params, seed, scale=1.0):
    """randn gradients under `seed` (the unaligned parameter's gradient is unaligned too; the last parameter gets none).
    A second call refills the same gradient tensors in place."""
    g = torch.Generator().manual_seed(seed)
    for k, p in enumerate(params[:-1]):
        val = (torch.randn(p.shape, generator=g) * scale).cuda()
        if p.grad is not None:
            p.grad.copy_(val)
        else:
            p.grad = _off_by_one_float(val) if k == len(params) - 2 else val
    assert params[-1].grad is None and params[-2].grad.data_ptr() % 16 == 4
    return params


def host_norm(params):
    return math.sqrt(sum(float(p.grad.double().square().sum()) for p in params if p.grad is not None))


def fused(params, **kw):
    from tmdiff_amd.optim import FusedAdamW
    kw.setdefault("lr", torch.tensor(LR, device="cuda"))
    kw.setdefault("weight_decay", WD)
    return FusedAdamW(params, **kw)


def bits(t):
    return t.detach().clone().view(torch.int32)


def same_state(oa, pa, ob, pb, what=""):
    """parameters, both moments and the step counter, bit for bit"""
    for k, (x, y) in enumerate(zip(pa, pb)):
        assert torch.equal(bits(x), bits(y)), f"{what}: parameter {k} ({x.numel()} elements)"
        sx, sy = oa.state.get(x, {}), ob.state.get(y, {})
        assert ("exp_avg" in sx) == ("exp_avg" in sy), f"{what}: state of parameter {k}"
        if "exp_avg" in sx:
            assert torch.equal(bits(sx["exp_avg"]), bits(sy["exp_avg"])), f"{what}: exp_avg {k}"
            assert torch.equal(bits(sx["exp_avg_sq"]), bits(sy["exp_avg_sq"])), f"{what}: exp_avg_sq {k}"
            assert float(sx["step"]) == float(sy["step"]), f"{what}: step {k}"


def worst_rel(got, want):
    """the measure of tests/test_gpu_training.py::test_fused_adamw_is_torch_adamw: max |x - y| / max |x| per tensor"""
    return max(float((y.detach().double().cpu() - x).abs().max() / x.abs().max()) for x, y in zip(want, got))


# ---- the norm -----------------------------------------------------------------------------------------------------------------
def test_norm_matches_fp64_on_the_host():
    """(float)sqrt(sum of squares in double): the fp64 accumulation contributes at most n * 2^-53, the rest is the one
    rounding to fp32 -- relative error <= 2^-23."""
    for seed, scale in ((1, 1.0), (2, 1e-3), (3, 300.0)):
        params = set_grads(make_params(), seed, scale)
        opt = fused(params, max_grad_norm=1.0)
        opt.step()
        want = host_norm(params)
        got = float(opt.last_grad_norm)
        print(f"norm seed {seed}: device {got!r} host {want!r} relative error {abs(got - want) / want:.3e}")
        assert abs(got - want) <= 2.0 ** -23 * want
        assert float(opt.last_step_ok) == 1.0


def test_zero_gradients_give_norm_zero_and_coefficient_one():
    params = set_grads(make_params(), 1, 0.0)
    before = [p.detach().clone() for p in params]
    opt = fused(params, max_grad_norm=0.5, weight_decay=0.0)
    opt.step()
    assert float(opt.last_grad_norm) == 0.0 and float(opt.last_clip_coef) == 1.0 and float(opt.last_step_ok) == 1.0
    assert all(torch.equal(p, q) for p, q in zip(params, before))           # m = 0: nothing moves without weight decay


def test_norm_and_coefficient_are_reproducible():
    params = set_grads(make_params(), 5)
    opt = fused(params, max_grad_norm=0.25 * host_norm(params))
    seen = []
    for _ in range(2):
        opt.step()
        seen.append((bits(opt.last_grad_norm), bits(opt.last_clip_coef)))
    assert torch.equal(seen[0][0], seen[1][0]) and torch.equal(seen[0][1], seen[1][1])
    other = fused(set_grads(make_params(), 5), max_grad_norm=opt.max_grad_norm)
    other.step()
    assert torch.equal(bits(other.last_grad_norm), seen[0][0]) and torch.equal(bits(other.last_clip_coef), seen[0][1])


# ---- the scaled step against the plain one ----------------------------------------------------------------------------------
def test_inactive_clip_is_exact():
    pa, pb = make_params(), make_params()
    oa, ob = fused(pa), fused(pb, max_grad_norm=1e30)
    for it in range(3):
        set_grads(pa, 10 + it)
        set_grads(pb, 10 + it)
        oa.step()
        ob.step()
        assert float(ob.last_clip_coef) == 1.0
    same_state(oa, pa, ob, pb, "max_grad_norm = 1e30")


def test_active_clip_is_the_plain_step_on_scaled_gradients():
    """The clipped step on g equals the unclipped FusedAdamW on g * coef (formed in fp32 by torch), and g keeps its bits."""
    pa, pb = set_grads(make_params(), 21), set_grads(make_params(), 21)
    oa, ob = fused(pa, max_grad_norm=0.5 * host_norm(pa)), fused(pb)
    for it in range(2):                          # the second step starts from moments that are not zero
        if it:
            set_grads(pa, 22)
            set_grads(pb, 22)
        g0 = [bits(p.grad) for p in pa[:-1]]
        oa.step()
        coef = oa.last_clip_coef.clone()
        assert 0.0 < float(coef) < 1.0
        assert all(torch.equal(bits(p.grad), g) for p, g in zip(pa[:-1], g0)), "the clipped step wrote to a gradient"
        for p in pb[:-1]:
            p.grad.mul_(coef)
        ob.step()
        same_state(oa, pa, ob, pb, f"step {it}")
    assert pa[-1].grad is None and "exp_avg" not in oa.state.get(pa[-1], {})        # the gradient-free parameter is ignored


def test_clipped_step_with_one_misaligned_gradient_between_guards():
    """Three parameters of 5, chunk and chunk + 5 elements; the middle one's gradient alone starts one float past a 16-byte
    boundary (so that tensor takes the scalar walk in the norm and in the step while its parameter and moments are aligned).
    Every parameter, gradient and moment sits between sentinels.  The norm is within 2^-23 of fp64 (as in
    test_norm_matches_fp64_on_the_host), two clipped steps equal the plain steps on g * coef bit for bit, and no store lands
    outside a tensor or in a gradient."""
    sentinel, front, back = 12345.0, 4, 64
    sizes = (5, _chunk(), _chunk() + 5)
    gen = torch.Generator().manual_seed(91)
    p0 = [torch.randn(n, generator=gen) for n in sizes]
    g0 = [torch.randn(n, generator=gen) for n in sizes]
    want = math.sqrt(sum(float(g.double().square().sum()) for g in g0))

    def build(**kw):
        bufs = []

        def put(values, off=0):
            lo = front + off
            buf = torch.full((lo + values.numel() + back,), sentinel, device="cuda")
            view = buf[lo:lo + values.numel()]
            view.copy_(values)
            assert view.data_ptr() % 16 == 4 * off and view.is_contiguous()
            bufs.append((buf, lo, values.numel()))
            return view
        params = [torch.nn.Parameter(put(v)) for v in p0]
        opt = fused(params, **kw)
        for k, (q, g) in enumerate(zip(params, g0)):
            q.grad = put(g, 1 if k == 1 else 0)
            opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"] = put(torch.zeros_like(g)), put(torch.zeros_like(g))
        assert params[1].data_ptr() % 16 == 0 and params[1].grad.data_ptr() % 16 == 4
        return params, opt, bufs
    pa, oa, bufs_a = build(max_grad_norm=0.5 * want)
    pb, ob, bufs_b = build()
    for it in range(2):                          # the second step starts from moments that are not zero
        oa.step()
        got, coef = float(oa.last_grad_norm), oa.last_clip_coef.clone()
        print(f"step {it}: norm {got!r}, fp64 {want!r}, relative error {abs(got - want) / want:.3e}, coefficient {float(coef)!r}")
        assert abs(got - want) <= 2.0 ** -23 * want
        assert float(oa.last_step_ok) == 1.0 and 0.0 < float(coef) < 1.0
        for q, g in zip(pa, g0):
            assert torch.equal(bits(q.grad), bits(g.cuda())), "the clipped step wrote to a gradient"
        for q, g in zip(pb, g0):
            q.grad.copy_(g)
            q.grad.mul_(coef)
        ob.step()
        same_state(oa, pa, ob, pb, f"step {it}")
    torch.cuda.synchronize()
    for buf, lo, n in bufs_a + bufs_b:
        assert bool((buf[:lo] == sentinel).all()), "a store landed in front of a tensor"
        assert bool((buf[lo + n:] == sentinel).all()), "a store landed past the end of a tensor"


# ---- against torch ----------------------------------------------------------------------------------------------------------------
def _torch_reference(params, groups, max_norm, grad_sets):
    """clip_grad_norm_(max_norm) + torch.optim.AdamW in fp64 on the CPU; `groups`: (index list, lr, weight_decay)"""
    ref = [torch.nn.Parameter(p.detach().double().cpu()) for p in params]
    opt = torch.optim.AdamW([{"params": [ref[i] for i in idx], "lr": lr, "weight_decay": wd} for idx, lr, wd in groups])
    for seed, scale in grad_sets:
        set_grads(params, seed, scale)
        for p, r in zip(params, ref):
            r.grad = None if p.grad is None else p.grad.detach().double().cpu()
        torch.nn.utils.clip_grad_norm_([r for r in ref if r.grad is not None], max_norm)
        opt.step()
    return [r.detach() for r in ref]


def test_clipped_steps_follow_clip_grad_norm_and_torch_adamw():
    """Three steps, the middle one with small gradients: coef < 1, == 1, < 1.  Tolerance: 2e-6 on max |x - y| / max |x| per
    tensor, the bound of FusedAdamW against torch.optim.AdamW in tests/test_gpu_training.py:264 (there after eight steps)."""
    grad_sets = ((31, 1.0), (32, 0.1), (33, 1.0))
    params = set_grads(make_params(), 31)
    max_norm = 0.5 * host_norm(params)               # between the norms of the large and the small sets
    want = _torch_reference(make_params(), [(list(range(len(params))), LR, WD)], max_norm, grad_sets)
    opt = fused(params, max_grad_norm=max_norm)
    coefs = []
    for seed, scale in grad_sets:
        set_grads(params, seed, scale)
        opt.step()
        coefs.append(float(opt.last_clip_coef))
    assert coefs[0] < 1.0 and coefs[1] == 1.0 and coefs[2] < 1.0, coefs
    worst = worst_rel(params, want)
    print(f"clipped FusedAdamW vs clip_grad_norm_ + AdamW (fp64): {worst:.2e} after 3 steps, coefficients {coefs}")
    assert worst <= 2e-6, worst


def test_two_parameter_groups_share_one_norm():
    params = make_params()
    idx_a = [k for k in range(len(params)) if k % 2 == 0]
    idx_b = [k for k in range(len(params)) if k % 2 == 1]
    groups = [(idx_a, 1e-3, 1e-2), (idx_b, 3e-3, 0.0)]
    grad_sets = ((41, 1.0), (42, 0.1))
    max_norm = 0.5 * host_norm(set_grads(make_params(), 41))
    want = _torch_reference(make_params(), groups, max_norm, grad_sets)
    opt = fused([{"params": [params[i] for i in idx], "lr": torch.tensor(lr, device="cuda"), "weight_decay": wd}
                 for idx, lr, wd in groups], max_grad_norm=max_norm)
    coefs = []
    for seed, scale in grad_sets:
        set_grads(params, seed, scale)
        opt.step()
        total = host_norm(params)
        assert abs(float(opt.last_grad_norm) - total) <= 2.0 ** -23 * total          # over BOTH groups
        coefs.append(float(opt.last_clip_coef))
    assert coefs[0] < 1.0 and coefs[1] == 1.0, coefs
    worst = worst_rel(params, want)
    print(f"two groups vs torch: {worst:.2e}")
    assert worst <= 2e-6, worst                                                      # tests/test_gpu_training.py:264


# ---- the skipped step ---------------------------------------------------------------------------------------------------------
def test_nonfinite_gradients_skip_the_step():
    pa, pb = make_params(), make_params()
    oa, ob = fused(pa, max_grad_norm=1.0), fused(pb, max_grad_norm=1.0)          # ob never sees the bad batches
    for o, p in ((oa, pa), (ob, pb)):
        set_grads(p, 51)
        o.step()
    for bad, where in ((float("inf"), 3), (float("nan"), 5), (float("-inf"), len(pa) - 2)):
        set_grads(pa, 52)
        pa[where].grad.view(-1)[pa[where].numel() // 2] = bad
        oa.step()
        assert float(oa.last_step_ok) == 0.0 and float(oa.last_clip_coef) == 0.0
        assert not math.isfinite(float(oa.last_grad_norm))
        same_state(oa, pa, ob, pb, f"after a gradient with {bad}")             # p, m, v and the counter kept their bits
    assert float(oa.state[pa[0]]["step"]) == 1.0
    for o, p in ((oa, pa), (ob, pb)):
        set_grads(p, 53)
        o.step()
    assert float(oa.last_step_ok) == 1.0 and float(oa.state[pa[0]]["step"]) == 2.0
    same_state(oa, pa, ob, pb, "the step after the skipped ones")


def test_without_skip_nonfinite_gradients_propagate_as_in_torch():
    """error_if_nonfinite=False: an infinite norm makes the coefficient 0 (inf * 0 = NaN in the bad element), a NaN norm
    makes it NaN (every element).  Arithmetic only."""
    for bad in (float("inf"), float("nan")):
        params = set_grads(make_params(), 61)
        ref = [torch.nn.Parameter(p.detach().clone()) for p in params]
        params[3].grad[1] = bad
        for p, r in zip(params, ref):
            r.grad = None if p.grad is None else p.grad.detach().clone()
        opt = fused(params, max_grad_norm=1.0, skip_nonfinite=False)
        opt.step()
        torch.nn.utils.clip_grad_norm_([r for r in ref if r.grad is not None], 1.0, error_if_nonfinite=False)
        topt = torch.optim.AdamW(ref, lr=LR, weight_decay=WD)
        topt.step()
        assert float(opt.last_step_ok) == 1.0 and float(opt.state[params[0]]["step"]) == 1.0
        assert not torch.isfinite(params[3]).all()
        for k, (p, r) in enumerate(zip(params, ref)):
            assert torch.equal(torch.isfinite(p), torch.isfinite(r)), (bad, k)


# ---- HIP graph -----------------------------------------------------------------------------------------------------------------
def test_recorded_clipped_step_replays_like_the_eager_one():
    """step() with clipping recorded on a side stream after one eager warm-up step (as model.CapturedStep does); each replay
    follows an in-place refill of the same gradient tensors -- clipped, not clipped, non-finite -- and equals the eager
    optimizer on the same gradients bit for bit: parameters, moments, counter, norm, coefficient and flag."""
    pe, pg = set_grads(make_params(), 71), set_grads(make_params(), 71)
    max_norm = 0.5 * host_norm(pe)
    oe, og = fused(pe, max_grad_norm=max_norm), fused(pg, max_grad_norm=max_norm)
    oe.step()
    og.step()                                        # warm-up: state, tables and the norm buffers exist
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(graph, stream=side):
        og.step()
    same_state(oe, pe, og, pg, "recording runs nothing")
    seen = []
    for seed, scale, bad in ((72, 1.0, None), (73, 0.1, None), (74, 1.0, float("inf")), (75, 1.0, None)):
        for p in (pe, pg):
            set_grads(p, seed, scale)
            if bad is not None:
                p[2].grad[7] = bad
        oe.step()
        graph.replay()
        torch.cuda.synchronize()
        same_state(oe, pe, og, pg, f"replay on gradient set {seed}")
        for name in ("last_grad_norm", "last_clip_coef", "last_step_ok"):
            assert torch.equal(bits(getattr(oe, name)), bits(getattr(og, name))), (seed, name)
        seen.append((float(og.last_clip_coef), float(og.last_step_ok)))
    assert seen[0][0] < 1.0 and seen[1] == (1.0, 1.0) and seen[2] == (0.0, 0.0) and seen[3][1] == 1.0, seen
    assert float(og.state[pg[0]]["step"]) == 4.0                    # warm-up + three applied replays


# ---- the trainer --------------------------------------------------------------------------------------------------------------
def test_trainer_option_clips_inside_the_eager_and_the_captured_step():
    """train.max_grad_norm on the smallest DDPM of tests/test_gpu_training.py (test_trainer_wrapper_roundtrip): the eager
    warm-up steps and one HIP-graph step.  After each, the weights equal those a standalone clipped FusedAdamW makes of the weights,
    the moments and the learning rate from before the step and the gradients the trainer's own backward left behind."""
    from oracle.make_golden import TINY, case_inputs
    from tmdiff_amd.model import DDPM
    from tmdiff_amd.optim import FusedAdamW
    bound = 1e-3
    opt = {"phase": "train", "gpu_ids": [0], "distributed": False, "path": {"resume": None},
           "model": {"unet": {"channel_multiplier": TINY}, "diffusion": {"loss_type": "l1"}, "init_type": "orthogonal"},
           "train": {"optimizer": {"lr": 1e-3}, "max_iter": 100, "hip_graph": True, "max_grad_norm": bound}}
    torch.manual_seed(1)
    np.random.seed(1)
    m = DDPM(opt)
    assert isinstance(m.optG, FusedAdamW) and m.optG.max_grad_norm == bound
    m.set_new_noise_schedule({"schedule": "cosine", "n_timestep": 10}, "train")
    m.scheduler.step()                               # (the warm-up schedule starts at lr = 0, where no weight moves)
    d = case_inputs(3, 2, 8, 16)
    d["LR"] = d["MS"].clone()
    trained = [p for n, p in m.netG.named_parameters() if "clip_text" not in n]
    for it in range(DDPM.GRAPH_WARMUP + 1):          # the eager warm-up steps, then the step recorded and replayed
        lr = float(m.optG.param_groups[0]["lr"])
        assert lr > 0.0
        before = [(p.detach().clone(), {k: v.detach().clone() for k, v in m.optG.state.get(p, {}).items()}) for p in trained]
        m.feed_data({k: v.clone() for k, v in d.items()})
        m.optimize_parameters("WV3")
        log = m.get_current_log()
        assert math.isfinite(log["grad_norm"]) and log["grad_norm"] > bound and log["skipped"] == 0.0
        twin = [torch.nn.Parameter(w.clone()) for w, _ in before]
        topt = FusedAdamW(twin, lr=torch.tensor(lr, device="cuda"), weight_decay=1e-4, max_grad_norm=bound)
        for q, p, (_, st) in zip(twin, trained, before):
            q.grad = None if p.grad is None else p.grad.detach().clone()
            if st:
                topt.state[q] = st
        topt.step()
        assert float(topt.last_grad_norm) == log["grad_norm"]
        moved = 0
        for k, (q, p, (w, _)) in enumerate(zip(twin, trained, before)):
            assert torch.equal(q, p), (it, k)
            moved += int(not torch.equal(p, w))
        assert moved > 100, moved
        print(f"trainer step {it} ({'graph' if m._captured else 'eager'}): grad_norm {log['grad_norm']:.4f}, {moved} tensors moved")
    assert len(m._captured) == 1 and next(iter(m._captured.values())).replays == 1
