"""The transformer modules of tmdiff_amd.Attention on their differentiable path: the gradient of every input and every
parameter against torch autograd over the oracle modules in float64 on the CPU, and the differentiable forward against the
inference path (bit-equal).

Tolerance, as in test_gpu_norm_bwd.py: rel-L2 error against float64 at most 4 x that of the oracle module evaluated in float32
on the CPU, the yardstick floored at 2^-24 * sqrt(n).  n is the longest sum behind one element of the gradient: for a parameter
the rows it is summed over (batch x tokens, the weight-gradient GEMM's depth), for an input the widest contraction on its way
back (the largest layer width of the module).  Each comparison prints kernel error, yardstick and ratio.
"""
import functools

import pytest
import torch

from oracle import attention_ref as R
from oracle import unet_ref as U

pytestmark = pytest.mark.gpu


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# name -> (class name, args, kwargs, input shapes (x, context or None), context passed as a list of that many, n_param, n_input)
CASES = {
    "ff_glu": ("FeedForward", (64,), dict(glu=True), ((3, 10, 64), None), 0, 30, 256),
    "ff_gelu": ("FeedForward", (64,), dict(glu=False), ((3, 10, 64), None), 0, 30, 256),
    "block": ("BasicTransformerBlock", (128, 8, 16), dict(context_dim=768), ((2, 64, 128), (2, 77, 768)), 0, 154, 768),
    "block_no_self": ("BasicTransformerBlock", (128, 8, 16), dict(context_dim=768, disable_self_attn=True),
                      ((2, 64, 128), (2, 77, 768)), 0, 154, 768),
    "st_conv": ("SpatialTransformer", (128, 8, 16), dict(depth=1, context_dim=768), ((2, 128, 8, 8), (2, 77, 768)), 0, 154, 768),
    "st_linear": ("SpatialTransformer", (128, 8, 16), dict(depth=1, context_dim=768, use_linear=True),
                  ((2, 128, 8, 8), (2, 77, 768)), 0, 154, 768),
    "st_depth2": ("SpatialTransformer", (64, 4, 16), dict(depth=2, context_dim=[32, 32]), ((1, 64, 8, 8), (1, 10, 32)), 2, 64, 256),
    "ssa": ("SpatialSelfAttention", (64,), {}, ((2, 64, 8, 8), None), 0, 128, 64),
    "attnpp_rescale": ("AttnBlockpp", (64,), dict(skip_rescale=True), ((2, 16, 4, 8, 8), None), 0, 128, 64),
    "attnpp_plain": ("AttnBlockpp", (64,), dict(skip_rescale=False), ((2, 16, 4, 8, 8), None), 0, 128, 64),
}


def _call(module, x, ctx, as_list):
    if ctx is None:
        return module(x)
    return module(x, context=[ctx] * as_list if as_list else ctx)


def _cross_forward(self, x, context=None, mask=None):
    """oracle/attention_ref.py's CrossAttention.forward line by line, without its casts of q and k to float32 (with them the
    module cannot run in float64); _case checks that in float32 the two agree bit for bit."""
    h = self.heads
    ctx = x if context is None else context
    split = lambda t: t.reshape(t.shape[0], t.shape[1], h, -1).permute(0, 2, 1, 3)
    q, k, v = split(self.to_q(x)), split(self.to_k(ctx)), split(self.to_v(ctx))
    sim = torch.matmul(q, k.transpose(-1, -2)) * self.scale
    if mask is not None:
        sim = sim.masked_fill(~mask.reshape(mask.shape[0], 1, 1, -1), -torch.finfo(torch.float32).max)
    out = torch.matmul(sim.softmax(dim=-1), v)
    out = out.permute(0, 2, 1, 3).reshape(x.shape[0], x.shape[1], -1)
    return self.to_out(out)


def _oracle(ref, x, ctx, as_list, dout, dtype, restate=False):
    """Output and gradients (inputs, then parameters by name) of the oracle module in `dtype` on the CPU; restate: with the
    CrossAttention layers on _cross_forward."""
    import copy
    import types
    m = copy.deepcopy(ref).to(dtype)
    if restate:
        for sub in m.modules():
            if isinstance(sub, R.CrossAttention):
                sub.forward = types.MethodType(_cross_forward, sub)
    x = x.to(dtype).clone().requires_grad_()
    ctx = None if ctx is None else ctx.to(dtype).clone().requires_grad_()
    out = _call(m, x, ctx, as_list)
    out.backward(dout.to(dtype))
    grads = {"x": x.grad}
    if ctx is not None:
        grads["context"] = ctx.grad
    grads.update({name: p.grad for name, p in m.named_parameters()})
    return out.detach(), grads


@functools.lru_cache(maxsize=None)
def _case(name):
    """Modules, inputs, the float64 oracle and the float32 yardstick of one case: computed once, never modified."""
    from tmdiff_amd import Attention as A
    cls, args, kw, (xs, cs), as_list, n_param, n_input = CASES[name]
    ref = U.fill_weights_(getattr(R, cls)(*args, **kw), seed=3).eval()      # every parameter, the zero-initialised proj_out too
    hip = getattr(A, cls)(*args, **kw)
    hip.load_state_dict(ref.state_dict())
    hip = hip.cuda().eval()
    x, ctx = _randn(21, *xs), None if cs is None else _randn(22, *cs)
    with torch.no_grad():
        dout = _randn(23, *_call(ref, x, ctx, as_list).shape)
    f32, restated = _oracle(ref, x, ctx, as_list, dout, torch.float32), _oracle(ref, x, ctx, as_list, dout, torch.float32, True)
    assert torch.equal(f32[0], restated[0]) and all(torch.equal(restated[1][n], g) for n, g in f32[1].items()), \
        "the float64 reference does not restate the oracle"
    return dict(hip=hip, x=x, ctx=ctx, as_list=as_list, dout=dout, n_param=n_param, n_input=n_input,
                f64=_oracle(ref, x, ctx, as_list, dout, torch.float64, True), f32=f32)


def _rel_l2(a, ref):
    a, ref = a.detach().cpu().double(), ref.double()
    return float((a - ref).norm() / ref.norm().clamp_min(1e-30))


def _check(what, got, f32, f64, n):
    assert got is not None, f"{what}: no gradient"
    assert got.shape == f64.shape, (what, got.shape, f64.shape)
    assert torch.isfinite(got).all(), f"{what}: not finite"
    err, yard = _rel_l2(got, f64), max(_rel_l2(f32, f64), 2.0 ** -24 * n ** 0.5)
    print(f"{what}: kernel {err:.3e}  yardstick {yard:.3e}  ratio {err / yard:.2f}")
    assert err <= 4 * yard, f"{what}: rel-L2 error {err:.3e} > 4 x {yard:.3e}"


# The bias of a key projection shifts every score of a query by the same amount, which softmax ignores: its gradient is zero
# in exact arithmetic, and what any evaluation returns is rounding residue (float64: 1e-17, float32: 1e-8), for which a
# relative error means nothing.  It is bounded in absolute terms instead: 4 x the larger of the float32 evaluation's residue
# and 2^-24 sqrt(n) times the size of the query bias's gradient (a sum of the same n terms that does not cancel).
SHIFT_BIAS = {"k.bias": "q.bias", "NIN_1.b": "NIN_0.b"}


def _check_zero(what, got, f32, sibling64, n):
    assert got is not None and torch.isfinite(got).all(), what
    res, yard = float(got.abs().max()), max(float(f32.abs().max()), 2.0 ** -24 * n ** 0.5 * float(sibling64.abs().max()))
    print(f"{what}: kernel residue {res:.3e}  yardstick {yard:.3e}  ratio {res / yard:.2f}")
    assert res <= 4 * yard, f"{what}: residue {res:.3e} > 4 x {yard:.3e}"


@pytest.mark.parametrize("name", list(CASES))
def test_module_backward_vs_float64(name):
    c = _case(name)
    hip = c["hip"]
    hip.zero_grad(set_to_none=True)
    x = c["x"].cuda().requires_grad_()
    ctx = None if c["ctx"] is None else c["ctx"].cuda().requires_grad_()
    assert torch.is_grad_enabled()
    out = _call(hip, x, ctx, c["as_list"])
    with torch.no_grad():
        assert torch.equal(out.detach(), _call(hip, x, ctx, c["as_list"])), "differentiable forward differs from the inference path"
    out.backward(c["dout"].cuda())          # (on the inference-only modules: no grad_fn, and this raises)
    (_, f64), (_, f32) = c["f64"], c["f32"]
    _check(f"{name} x", x.grad, f32["x"], f64["x"], c["n_input"])
    if ctx is not None:
        _check(f"{name} context", ctx.grad, f32["context"], f64["context"], c["n_input"])
    params = dict(hip.named_parameters())
    assert set(params) == set(f64) - {"x", "context"}
    for pname, p in params.items():
        if pname in SHIFT_BIAS:
            _check_zero(f"{name} {pname}", p.grad, f32[pname], f64[SHIFT_BIAS[pname]], c["n_param"])
        else:
            _check(f"{name} {pname}", p.grad, f32[pname], f64[pname], c["n_param"])
    hip.zero_grad(set_to_none=True)


@pytest.mark.parametrize("name", list(CASES))
def test_frozen_module_takes_the_inference_path(name):
    c = _case(name)
    hip = c["hip"]
    for p in hip.parameters():
        p.requires_grad_(False)
    try:
        out = _call(hip, c["x"].cuda(), None if c["ctx"] is None else c["ctx"].cuda(), c["as_list"])
        assert out.grad_fn is None and not out.requires_grad
    finally:
        for p in hip.parameters():
            p.requires_grad_(True)
