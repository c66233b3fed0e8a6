"""The attention backward on the device (tmdiff_attn_fwd_lse / tmdiff_attn_bwd, autograd.AttentionFn, CrossAttention's
differentiable path) against torch autograd in float64 on the CPU.

Tolerance: the same formula evaluated by torch in float32 on the CPU has a rel-L2 error against float64; the kernel's error
on the same inputs may be at most 4 x that yardstick, separately for every gradient (the margin is for re-forming P from a
stored LSE and summing in 32-key blocks).  Each comparison prints both numbers.
"""
import functools

import pytest
import torch

from oracle import attention_ref as R
from oracle import unet_ref as U

pytestmark = pytest.mark.gpu

FILL = -torch.finfo(torch.float32).max

#          B  H  Nq   Nk   D
CASES = ((2, 2, 33, 40, 16),      # generic kernel, one D tile
         (2, 2, 33, 40, 40),      # D tail (padded to two D tiles)
         (1, 2, 130, 160, 64),    # pipelined forward routes
         (1, 2, 130, 160, 128),
         (2, 8, 130, 77, 64),     # small-context kernel, 80-row variant
         (2, 8, 130, 96, 64),     # ... 96-row variant
         (2, 8, 130, 97, 64),     # first Nk past the small-context kernel
         (1, 1, 1, 1, 64),        # degenerate extents
         (1, 1, 1, 77, 64),
         (1, 1, 130, 1, 64))
MASK_CASE = (2, 8, 130, 77, 64)


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _formula(q, k, v, scale, heads, mask):
    """softmax((q k^T) * scale masked_fill(-finfo(float32).max)) v with the heads split as ops.attention splits them."""
    b, nq, hd = q.shape
    split = lambda t: t.reshape(b, t.shape[1], heads, hd // heads).permute(0, 2, 1, 3)
    sim = torch.matmul(split(q), split(k).transpose(-1, -2)) * scale
    if mask is not None:
        sim = sim.masked_fill(~mask[:, None, None, :], FILL)
    out = torch.matmul(sim.softmax(dim=-1), split(v))
    return out.permute(0, 2, 1, 3).reshape(b, nq, hd), torch.logsumexp(sim, dim=-1)


def _autograd(q, k, v, dout, scale, heads, mask, dtype):
    q, k, v = (t.to(dtype).clone().requires_grad_() for t in (q, k, v))       # (leaves of their own: the inputs are shared)
    out, lse = _formula(q, k, v, scale, heads, mask)
    out.backward(dout.to(dtype))
    return {"out": out.detach(), "lse": lse.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad}


def _mask(b, nk):
    m = torch.ones(b, nk, dtype=torch.bool)
    m[0, 40:] = False      # keys 40.. of sample 0
    m[1, :] = False        # every key of sample 1
    return m


@functools.lru_cache(maxsize=None)
def _case(extents, masked=False):
    """Inputs, the float64 oracle and the float32 yardstick of one case: computed once, shared by the tests, never modified."""
    b, h, nq, nk, d = extents
    q, k, v, dout = _randn(1, b, nq, h * d), _randn(2, b, nk, h * d), _randn(3, b, nk, h * d), _randn(4, b, nq, h * d)
    mask = _mask(b, nk) if masked else None
    scale = d ** -0.5
    return dict(q=q, k=k, v=v, dout=dout, mask=mask, scale=scale, heads=h,
                f64=_autograd(q, k, v, dout, scale, h, mask, torch.float64),
                f32=_autograd(q, k, v, dout, scale, h, mask, torch.float32))


def _rel_l2(a, ref):
    a, ref = a.detach().cpu().double(), ref.double()
    return float((a - ref).norm() / ref.norm().clamp_min(1e-30))


def _check(what, got, f32, f64):
    """rel-L2 error of `got` against float64 <= 4 x that of the float32 evaluation; prints both."""
    err, yard = _rel_l2(got, f64), _rel_l2(f32, f64)
    print(f"{what}: kernel {err:.3e}  float32 eager {yard:.3e}  ratio {err / yard if yard > 0 else float(err > 0):.2f}")
    assert err <= 4 * yard, f"{what}: rel-L2 error {err:.3e} > 4 x {yard:.3e} (float32 eager against float64)"


def _device_backward(c, need=(True, True, True)):
    from tmdiff_amd import ops
    q, k, v, dout = (c[n].cuda() for n in ("q", "k", "v", "dout"))
    out, lse = ops.attention_lse(q, k, v, c["scale"], heads=c["heads"], key_mask=c["mask"])
    return out, lse, ops.attention_bwd(q, k, v, out, dout, lse, c["scale"], heads=c["heads"], key_mask=c["mask"], need=need)


@pytest.mark.parametrize("extents", CASES, ids=lambda e: "x".join(map(str, e)))
def test_backward_vs_float64(extents):
    c = _case(extents)
    _, _, grads = _device_backward(c)
    for name, g in zip(("dq", "dk", "dv"), grads):
        _check(f"{extents} {name}", g, c["f32"][name], c["f64"][name])


@pytest.mark.parametrize("extents", CASES, ids=lambda e: "x".join(map(str, e)))
def test_forward_identity_and_lse(extents):
    from tmdiff_amd import ops
    c = _case(extents)
    q, k, v = (c[n].cuda() for n in ("q", "k", "v"))
    out, lse = ops.attention_lse(q, k, v, c["scale"], heads=c["heads"])
    assert torch.equal(out, ops.attention(q, k, v, c["scale"], heads=c["heads"]))
    assert lse.shape == c["f64"]["lse"].shape
    err = float((lse.cpu().double() - c["f64"]["lse"]).abs().max())
    print(f"{extents} lse: max abs error {err:.3e}")
    assert err <= 1e-5


def test_masked_keys():
    from tmdiff_amd import ops
    c = _case(MASK_CASE, masked=True)
    b, h, nq, nk, d = MASK_CASE
    out, _, (dq, dk, dv) = _device_backward(c)
    q, k, v = (c[n].cuda() for n in ("q", "k", "v"))
    assert torch.equal(out, ops.attention(q, k, v, c["scale"], heads=h, key_mask=c["mask"]))
    _check("masked out", out, c["f32"]["out"], c["f64"]["out"])
    for name, g in zip(("dq", "dk", "dv"), (dq, dk, dv)):
        _check(f"masked {name}", g, c["f32"][name], c["f64"][name])
    # sample 0: masked keys weigh exp(-FLT_MAX - m) = 0 exactly
    assert not dk[0, 40:].any() and not dv[0, 40:].any()
    assert dk[0, :40].any() and dv[0, :40].any()
    # sample 1, every key masked: uniform P = 1 / Nk, and masked_fill passes no gradient to the scores
    assert not dq[1].any() and not dk[1].any()
    # ... so every dv row of the sample is (1 / Nk) * sum_q dO.  Elementwise bound of a float32 sum of Nq terms in any order,
    # (Nq - 1) u sum|dO|, plus the roundings of 1 / Nk and of the product with it (u = 2^-24)
    g = c["dout"][1].double()
    want = g.sum(0, keepdim=True).expand(nk, h * d) / nk
    bound = (nq + 2) * 2.0 ** -24 * g.abs().sum(0, keepdim=True) / nk
    excess = float(((dv[1].cpu().double() - want).abs() / bound).max())
    print(f"all-masked dv against (1/Nk) sum_q dO: worst error / bound {excess:.3f}")
    assert excess <= 1.0


def test_deterministic_and_need_flags():
    c = _case(MASK_CASE)
    _, _, full = _device_backward(c)
    _, _, again = _device_backward(c)
    for a, b2 in zip(full, again):
        assert torch.equal(a, b2)
    _, _, (dq, dk, dv) = _device_backward(c, need=(True, False, False))
    assert dk is None and dv is None and torch.equal(dq, full[0])
    _, _, (dq, dk, dv) = _device_backward(c, need=(False, True, True))
    assert dq is None and torch.equal(dk, full[1]) and torch.equal(dv, full[2])


def test_attention_fn():
    """autograd.attention: needs_input_grad is honoured, a non-contiguous dout is accepted."""
    from tmdiff_amd import autograd
    c = _case((2, 2, 33, 40, 16))
    q, k, v = c["q"].cuda().requires_grad_(), c["k"].cuda(), c["v"].cuda().requires_grad_()
    out = autograd.attention(q, k, v, c["scale"], heads=c["heads"])
    dout = c["dout"].cuda().transpose(0, 1).contiguous().transpose(0, 1)          # the same values, other strides
    assert not dout.is_contiguous()
    out.backward(dout)
    assert k.grad is None
    _check("AttentionFn dq", q.grad, c["f32"]["dq"], c["f64"]["dq"])
    _check("AttentionFn dv", v.grad, c["f32"]["dv"], c["f64"]["dv"])


# ---- CrossAttention against the oracle's restatement -------------------------------------------------------------------

PARAMS = ("to_q.weight", "to_k.weight", "to_v.weight", "to_out.0.weight", "to_out.0.bias")


class _CrossRef(torch.nn.Module):
    """The oracle's CrossAttention in the dtype of its parameters.  oracle/attention_ref.py casts q and k to float32, so it
    cannot serve as the float64 reference itself; this restates its forward line by line (on its own parameters) without
    the casts, and the test checks that in float32 the two agree bit for bit."""

    def __init__(self, ref):
        super().__init__()
        self.ref = ref

    def forward(self, x, context=None, mask=None):
        r = self.ref
        ctx = x if context is None else context
        out, _ = _formula(r.to_q(x), r.to_k(ctx), r.to_v(ctx), r.scale, r.heads, None if mask is None else mask.reshape(mask.shape[0], -1))
        return r.to_out(out)


def _module_grads(mod, x, context, mask, residual, dout, dtype, device):
    """Output and gradients of a CrossAttention (the oracle's or the device's) in `dtype`; the oracle adds the residual outside."""
    mod = mod.to(dtype=dtype, device=device)
    mod.zero_grad(set_to_none=True)
    to = lambda t: None if t is None else t.to(dtype=dtype, device=device).clone().requires_grad_()
    x, context, residual = to(x), to(context), to(residual)
    kw = {} if mask is None else {"mask": mask}
    if isinstance(mod, (R.CrossAttention, _CrossRef)):
        y = mod(x, context=context, **kw)
        y = y if residual is None else y + residual
    else:
        y = mod(x, context=context, residual=residual, **kw)
    y.backward(dout.to(dtype=dtype, device=device))
    got = {"out": y.detach(), "dx": x.grad}
    if context is not None:
        got["dcontext"] = context.grad
    if residual is not None:
        got["dresidual"] = residual.grad
    params = dict(mod.named_parameters())
    got.update({n: params.get(n, params.get("ref." + n)).grad for n in PARAMS})
    return got


@pytest.mark.parametrize("heads,dim_head", ((8, 16), (2, 64)))
@pytest.mark.parametrize("variant", ("plain", "mask", "self", "residual"))
def test_cross_attention_gradients(heads, dim_head, variant):
    import copy
    from tmdiff_amd import Attention as A
    self_attn = variant == "self"
    kw = dict(heads=heads, dim_head=dim_head) if self_attn else dict(context_dim=768, heads=heads, dim_head=dim_head)
    ref = U.fill_weights_(R.CrossAttention(128, **kw), seed=3)
    hip = A.CrossAttention(128, **kw)
    hip.load_state_dict(ref.state_dict())
    hip = hip.cuda()
    x, dout = _randn(11, 2, 64, 128), _randn(12, 2, 64, 128)
    context = None if self_attn else _randn(13, 2, 77, 768)
    residual = _randn(14, 2, 64, 128) if variant == "residual" else None
    mask = None
    if variant == "mask":
        mask = torch.ones(2, 77, dtype=torch.bool)
        mask[0, 40:] = False
        mask[1, 5:9] = False
    f64 = _module_grads(_CrossRef(copy.deepcopy(ref)), x, context, mask, residual, dout, torch.float64, "cpu")
    f32 = _module_grads(copy.deepcopy(ref), x, context, mask, residual, dout, torch.float32, "cpu")
    restated = _module_grads(_CrossRef(copy.deepcopy(ref)), x, context, mask, residual, dout, torch.float32, "cpu")
    assert all(torch.equal(restated[n], f32[n]) for n in f32), "the float64 reference does not restate the oracle"
    got = _module_grads(hip, x, context, mask, residual, dout, torch.float32, "cuda")
    assert set(got) == set(f64)
    for name in sorted(f64):
        _check(f"CrossAttention {heads}x{dim_head} {variant} {name}", got[name], f32[name], f64[name])
    # the inference path: no graph, the same bits
    cu = lambda t: None if t is None else t.cuda()
    with torch.no_grad():
        y = hip(cu(x), context=cu(context), mask=mask, residual=cu(residual))
    assert y.grad_fn is None and not y.requires_grad and torch.equal(y, got["out"])
    hip.requires_grad_(False)
    y = hip(cu(x), context=cu(context), mask=mask, residual=cu(residual))
    assert y.grad_fn is None and not y.requires_grad and torch.equal(y, got["out"])
    hip.requires_grad_(True)
    assert hip(cu(x), context=cu(context), mask=mask, residual=cu(residual)).grad_fn is not None


def test_cross_attention_dropout_is_refused():
    from tmdiff_amd import Attention as A
    m = A.CrossAttention(128, context_dim=768, heads=2, dim_head=64, dropout=0.1).cuda().train()
    x, ctx = _randn(11, 2, 64, 128).cuda(), _randn(13, 2, 77, 768).cuda()
    with pytest.raises(NotImplementedError):
        m(x, context=ctx)
    m.eval()
    assert m(x, context=ctx).grad_fn is not None
