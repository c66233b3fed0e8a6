"""The LayerNorm / GroupNorm / GEGLU backward on the device (tmdiff_layer_norm_bwd, tmdiff_group_norm_bwd, tmdiff_geglu_bwd and
the *_stats forwards) against torch autograd in float64 on the CPU.

Tolerance, as in test_gpu_attention_bwd.py: the same formula evaluated by torch in float32 on the CPU has a rel-L2 error
against float64; the kernel's error on the same inputs may be at most 4 x that yardstick, separately for every gradient.  The
yardstick is floored at 2^-24 * sqrt(n), n the number of terms in the longest sum that forms one element of the gradient (the
random-walk rounding of an n-term float32 sum): D for a LayerNorm dx, rows for its dgamma / dbeta, cpg * P for a GroupNorm dx,
B * P for its dgamma / dbeta, 1 for the elementwise GEGLU.  Each comparison prints kernel error, yardstick and ratio.
"""
import functools
import itertools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

#            rows  D
LN_CASES = ((1, 1),          # zero variance: dx exactly 0
            (7, 40),         # D below a wave
            (5, 64),         # exactly one wave width
            (5, 65),         # one column past a wave
            (130, 128),      # several rows per workgroup
            (1030, 320),     # several row blocks, the last one ragged: more than one partial in the second stage
            (3, 4096))       # the largest D
#            B  C   P   groups
GN_CASES = ((2, 32, 64, 32),     # one channel per group
            (2, 64, 64, 32),     # two channels per group
            (2, 64, 49, 32),     # odd P
            (3, 64, 1, 32),      # P = 1
            (1, 32, 1, 32),      # one element per group: zero variance, dx exactly 0
            (2, 16, 64, 4),      # AttnBlockpp's min(channels // 4, 32) groups
            (1, 128, 256, 32))   # larger channel count and plane
GEGLU_CASES = ((1, 1), (3, 5), (10, 256), (130, 1024))
GATES = (-12.0, -6.0, -1e-3, 0.0, 1e-3, 6.0, 12.0)
LN_EPS, GN_EPS = 1e-5, 1e-6
NEEDS = [n for n in itertools.product((True, False), repeat=3) if any(n) and not all(n)]
ids = lambda e: "x".join(map(str, e))


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _rel_l2(a, ref):
    a, ref = a.detach().cpu().double(), ref.double()
    return float((a - ref).norm() / ref.norm().clamp_min(1e-30))


def _check(what, got, f32, f64, n):
    """rel-L2 error of `got` against float64 <= 4 x max(that of the float32 evaluation, 2^-24 sqrt(n)); prints all of them."""
    assert torch.isfinite(got).all(), f"{what}: not finite"
    err, yard = _rel_l2(got, f64), max(_rel_l2(f32, f64), 2.0 ** -24 * n ** 0.5)
    print(f"{what}: kernel {err:.3e}  yardstick {yard:.3e}  ratio {err / yard:.2f}")
    assert err <= 4 * yard, f"{what}: rel-L2 error {err:.3e} > 4 x {yard:.3e}"


def _grads(fn, tensors, dout, dtype):
    leaves = [None if t is None else t.to(dtype).clone().requires_grad_() for t in tensors]
    out = fn(*leaves)
    out.backward(dout.to(dtype))
    return [out.detach()] + [None if t is None else t.grad for t in leaves]


@functools.lru_cache(maxsize=None)
def _ln_case(extents):
    rows, d = extents
    x, dy = 0.3 + 1.5 * _randn(1, rows, d), _randn(2, rows, d)
    gamma, beta = 1 + 0.1 * _randn(3, d), 0.1 * _randn(4, d)
    fn = lambda x_, g_, b_: F.layer_norm(x_, (d,), g_, b_, LN_EPS)
    xd = x.double()
    mean, var = xd.mean(-1), xd.var(-1, unbiased=False)
    return dict(x=x, dy=dy, gamma=gamma, beta=beta, mean=mean, rstd=(var + LN_EPS).rsqrt(),
                f64=_grads(fn, (x, gamma, beta), dy, torch.float64), f32=_grads(fn, (x, gamma, beta), dy, torch.float32))


@functools.lru_cache(maxsize=None)
def _gn_case(extents, affine=True):
    b, c, p, groups = extents
    x, dy = 0.3 + 1.5 * _randn(5, b, c, p), _randn(6, b, c, p)
    gamma, beta = (1 + 0.1 * _randn(7, c), 0.1 * _randn(8, c)) if affine else (None, None)
    fn = lambda x_, g_, b_: F.group_norm(x_, groups, g_, b_, GN_EPS)
    if b * c * p // c == 1:      # F.group_norm refuses one value per channel ([1, 32, 1]): the same formula written out
        def fn(x_, g_, b_):
            xg = x_.reshape(b, groups, -1)
            xhat = (xg - xg.mean(-1, keepdim=True)) * (xg.var(-1, unbiased=False, keepdim=True) + GN_EPS).rsqrt()
            return xhat.reshape(b, c, p) * g_[None, :, None] + b_[None, :, None]
    xg = x.double().reshape(b, groups, -1)
    mean, var = xg.mean(-1), xg.var(-1, unbiased=False)
    return dict(x=x, dy=dy, gamma=gamma, beta=beta, mean=mean, rstd=(var + GN_EPS).rsqrt(),
                f64=_grads(fn, (x, gamma, beta), dy, torch.float64), f32=_grads(fn, (x, gamma, beta), dy, torch.float32))


def _cu(t):
    return None if t is None else t.cuda()


def _ln_device(c, need=(True, True, True)):
    from tmdiff_amd import ops
    x, gamma, beta, dy = (_cu(c[k]) for k in ("x", "gamma", "beta", "dy"))
    y, mean, rstd = ops.layer_norm_stats(x, gamma, beta, LN_EPS)
    return y, mean, rstd, ops.layer_norm_bwd(x, gamma, dy, mean, rstd, need=need)


def _gn_device(c, groups, need=(True, True, True)):
    from tmdiff_amd import ops
    x, gamma, beta, dy = (_cu(c[k]) for k in ("x", "gamma", "beta", "dy"))
    y, mean, rstd = ops.group_norm_stats(x, gamma, beta, groups, GN_EPS)
    return y, mean, rstd, ops.group_norm_bwd(x, gamma, dy, mean, rstd, groups, need=need)


def _check_stats(what, mean, rstd, c):
    for name, got in (("mean", mean), ("rstd", rstd)):
        ref = c[name].reshape(got.shape)
        err, mag = float((got.cpu().double() - ref).abs().max()), float(ref.abs().max())
        print(f"{what} {name}: max abs error {err:.3e}, magnitude {mag:.3e}")
        assert err <= 1e-5 * mag, f"{what} {name}: {err:.3e} > 1e-5 x {mag:.3e}"


@pytest.mark.parametrize("extents", LN_CASES, ids=ids)
def test_layer_norm_backward(extents):
    from tmdiff_amd import ops
    rows, d = extents
    c = _ln_case(extents)
    y, mean, rstd, grads = _ln_device(c)
    assert torch.equal(y, ops.layer_norm(c["x"].cuda(), c["gamma"].cuda(), c["beta"].cuda(), LN_EPS))
    _check_stats(f"layer_norm {extents}", mean, rstd, c)
    if d == 1:      # zero variance: xhat = 0 and g - mean(g) = 0, so dx and dgamma are exactly 0
        assert torch.isfinite(grads[0]).all() and not grads[0].any() and not grads[1].any()
        _check(f"layer_norm {extents} dbeta", grads[2], c["f32"][3], c["f64"][3], rows)
    else:
        for k, (name, n) in enumerate((("dx", d), ("dgamma", rows), ("dbeta", rows))):
            _check(f"layer_norm {extents} {name}", grads[k], c["f32"][k + 1], c["f64"][k + 1], n)
    for need in NEEDS:      # every subset: what is wanted is unchanged, the rest is not computed
        part = _ln_device(c, need)[3]
        for k in range(3):
            assert (part[k] is None) if not need[k] else torch.equal(part[k], grads[k]), (need, k)


@pytest.mark.parametrize("extents", GN_CASES, ids=ids)
def test_group_norm_backward(extents):
    from tmdiff_amd import ops
    b, ch, p, groups = extents
    c = _gn_case(extents)
    y, mean, rstd, grads = _gn_device(c, groups)
    assert torch.equal(y, ops.group_norm(c["x"].cuda(), c["gamma"].cuda(), c["beta"].cuda(), groups, GN_EPS))
    _check_stats(f"group_norm {extents}", mean, rstd, c)
    n_group = ch // groups * p
    if n_group == 1:      # zero variance, as for LayerNorm with D = 1
        assert torch.isfinite(grads[0]).all() and not grads[0].any() and not grads[1].any()
        _check(f"group_norm {extents} dbeta", grads[2], c["f32"][3], c["f64"][3], b * p)
    else:
        for k, (name, n) in enumerate((("dx", n_group), ("dgamma", b * p), ("dbeta", b * p))):
            _check(f"group_norm {extents} {name}", grads[k], c["f32"][k + 1], c["f64"][k + 1], n)
    for need in NEEDS:
        part = _gn_device(c, groups, need)[3]
        for k in range(3):
            assert (part[k] is None) if not need[k] else torch.equal(part[k], grads[k]), (need, k)


def test_group_norm_backward_without_affine():
    from tmdiff_amd import ops
    extents = (2, 64, 49, 32)
    c = _gn_case(extents, affine=False)
    y, mean, rstd, (dx, dgamma, dbeta) = _gn_device(c, 32, need=(True, False, False))
    assert dgamma is None and dbeta is None
    assert torch.equal(y, ops.group_norm(c["x"].cuda(), None, None, 32, GN_EPS))
    _check_stats("group_norm without affine", mean, rstd, c)
    _check("group_norm without affine dx", dx, c["f32"][1], c["f64"][1], 2 * 49)


def _geglu_check(what, u, dy, gelu_only):
    from tmdiff_amd import ops
    fn = (lambda u_: F.gelu(u_)) if gelu_only else (lambda u_: u_.chunk(2, -1)[0] * F.gelu(u_.chunk(2, -1)[1]))
    f64, f32 = _grads(fn, (u,), dy, torch.float64), _grads(fn, (u,), dy, torch.float32)
    du = ops.geglu_bwd(u.cuda(), dy.cuda(), gelu_only=gelu_only)
    assert du.shape == u.shape
    _check(what, du, f32[1], f64[1], 1)
    return du


@pytest.mark.parametrize("gelu_only", (False, True), ids=("geglu", "gelu"))
@pytest.mark.parametrize("extents", GEGLU_CASES, ids=ids)
def test_geglu_backward(extents, gelu_only):
    rows, inner = extents
    u, dy = 1.5 * _randn(9, rows, inner if gelu_only else 2 * inner), _randn(10, rows, inner)
    _geglu_check(f"{'gelu' if gelu_only else 'geglu'} {extents}", u, dy, gelu_only)


@pytest.mark.parametrize("gelu_only", (False, True), ids=("geglu", "gelu"))
def test_geglu_backward_tails(gelu_only):
    """Gates far in both tails of Phi / phi, and around 0."""
    gate = torch.tensor(GATES).repeat(3, 1)
    u = gate if gelu_only else torch.cat([1.5 * _randn(11, 3, len(GATES)), gate], dim=1)
    du = _geglu_check(f"{'gelu' if gelu_only else 'geglu'} tails", u, _randn(12, 3, len(GATES)), gelu_only)
    assert torch.isfinite(du).all()


def test_reproducible():
    """No atomics: a second run gives the same bits, the two-stage parameter gradients included."""
    c = _ln_case((1030, 320))
    first, second = _ln_device(c), _ln_device(c)
    for a, b in zip(first[:3] + first[3], second[:3] + second[3]):
        assert torch.equal(a, b)
    c = _gn_case((1, 128, 256, 32))
    first, second = _gn_device(c, 32), _gn_device(c, 32)
    for a, b in zip(first[:3] + first[3], second[:3] + second[3]):
        assert torch.equal(a, b)
