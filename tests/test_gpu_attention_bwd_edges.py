"""The attention backward (csrc/attention_bwd.hip, the LSE variants of csrc/attention.hip, ops.attention_lse / attention_bwd,
autograd.gemm_nt) on the paths test_gpu_attention_bwd.py never reaches: every head-dim tile count, extents at and around the
tile edges, four distinct stride triples through the C ABI, masks on every forward route, stressed logits, the LSE store with
several query blocks per wave, the remaining `need` combinations and gemm_nt's gradients at its edges.

Reference: torch autograd in float64 on the CPU of test_gpu_attention_bwd._formula (masked_fill(-finfo(float32).max), softmax,
matmul).  Yardstick: the same formula in float32 on the CPU.  Unless a section says otherwise a gradient's rel-L2 error against
float64 may be at most 4 x the yardstick's (test_gpu_attention_bwd._check, which prints both), and where the float64 gradient is
exactly zero the device's must be exactly zero too (tmdiff_hip.h promises it for masked keys and fully masked samples).
"""
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import test_gpu_attention_bwd as W
from oracle.make_golden import randn
from test_gpu_attention_bwd import _autograd, _check, _rel_l2
from test_gpu_attention_edges import (BND, HEAD_MAJOR, SENTINEL, ctx_qpw, fused, merge, padded_rows, shifted, split,
                                      stressed_inputs)

pytestmark = pytest.mark.gpu

FILL = -torch.finfo(torch.float32).max
EPS32 = float(torch.finfo(torch.float32).eps)
U24 = 2.0 ** -24
GRADS = ("dq", "dk", "dv")
ids = lambda e: "x".join(map(str, e))


def _check_grad(what, got, f32, f64):
    """_check, and exact zeros of the float64 gradient are exact zeros on the device."""
    _check(what, got, f32, f64)
    zero = f64 == 0
    if bool(zero.any()):
        bad = int((got.detach().cpu()[zero] != 0).sum())
        assert bad == 0, f"{what}: {bad} of {int(zero.sum())} elements whose float64 gradient is exactly 0 are not 0"


def _reference(q, k, v, dout, scale, heads, mask):
    """The float64 oracle and the float32 yardstick of inputs in the [B, N, H*D] layout."""
    return dict(q=q, k=k, v=v, dout=dout, mask=mask, scale=scale, heads=heads,
                f64=_autograd(q, k, v, dout, scale, heads, mask, torch.float64),
                f32=_autograd(q, k, v, dout, scale, heads, mask, torch.float32))


def _lse_error(what, lse, want):
    assert lse.shape == want.shape
    err = float((lse.cpu().double() - want).abs().max())
    print(f"{what} lse: max abs error {err:.3e}")
    assert err <= 1e-5, f"{what}: LSE differs from float64 by {err:.3e}"


# ---- B1 / B2: head-dim tiles, tile-exact and multi-workgroup extents ------------------------------------------------------------
#             B  H  Nq   Nk   D
HEAD_DIMS = ((2, 2, 33, 40, 2),       # DT = 1, one MFMA step
             (2, 2, 33, 40, 32),      # DT = 1, full tile
             (2, 2, 33, 40, 66),      # DT = 3, a 2-column tail in the third tile
             (2, 2, 33, 40, 80),      # DT = 3, the common dim_head 80
             (2, 2, 33, 40, 96),      # DT = 3, full
             (2, 2, 33, 40, 98),      # DT = 4, a 2-column tail in the fourth tile
             (2, 2, 33, 40, 126),     # DT = 4, the largest D with a tail
             (1, 2, 130, 160, 96))    # DT = 3 over two key workgroups and two query workgroups
EXTENTS = ((1, 2, 128, 128, 64),      # exactly one workgroup each way, four full waves
           (1, 2, 129, 127, 64),      # one query past / one key short of it
           (1, 2, 127, 129, 128),
           (1, 2, 256, 32, 32),       # exactly two query workgroups, exactly one key tile
           (1, 2, 32, 256, 32),
           (1, 1, 257, 257, 16),      # a third workgroup of one row
           (1, 2, 31, 33, 40),        # around one tile
           (1, 1, 300, 300, 16))      # three workgroups on both axes


@pytest.mark.parametrize("extents", HEAD_DIMS + EXTENTS, ids=ids)
def test_tiles_and_extents(extents):
    from tmdiff_amd import ops
    c = W._case(extents)
    out, lse, grads = W._device_backward(c)
    q, k, v = (c[n].cuda() for n in ("q", "k", "v"))
    assert torch.equal(out, ops.attention(q, k, v, c["scale"], heads=c["heads"])), "attention_lse's out is not attention's"
    _lse_error(extents, lse, c["f64"]["lse"])
    for name, g in zip(GRADS, grads):
        _check_grad(f"{extents} {name}", g, c["f32"][name], c["f64"][name])


# ---- B3: four distinct stride triples through the C ABI -------------------------------------------------------------------------
STRIDED = [
    # (H, Nq, Nk, D, q layout, k layout, v layout, out layout, small-context forward)
    (4, 150, 150, 32, fused(0), padded_rows(1), padded_rows(3), HEAD_MAJOR, False),
    (4, 150, 150, 64, HEAD_MAJOR, fused(1), padded_rows(2), shifted(1), False),
    (2, 130, 77, 128, padded_rows(1), HEAD_MAJOR, fused(2), BND, False),
    (4, 300, 77, 64, BND, shifted(3), fused(1), padded_rows(4), True),     # q / out rows 16-byte aligned: stays small-context
    (3, 150, 100, 80, padded_rows(1), fused(1), padded_rows(5), padded_rows(3), False),   # DT = 3, pad columns next to live data
    (2, 70, 45, 2, shifted(1), BND, padded_rows(1), HEAD_MAJOR, False),
]


def _placed(layout, fill, dims, x=None):
    """(flat buffer of `fill`, its [B, H, N, D] view in `layout` holding x)"""
    flat, view = layout.view(lambda n: torch.full((n,), fill, device="cuda"), *dims)
    if x is not None:
        view.copy_(x.cuda())
    return flat, view


def _gap_map(layout, dims):
    """True where the flat buffer of `layout` lies outside the [N, D] rows of every head; proved to miss exactly B*H*N*D elements."""
    gap_flat, gap = layout.view(lambda n: torch.ones(n, dtype=torch.bool, device="cuda"), *dims)
    gap.fill_(False)
    assert int((~gap_flat).sum()) == math.prod(dims), "the view overlaps itself"
    return gap_flat


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("h,nq,nk,d,ql,kl,vl,ol,ctx", STRIDED,
                         ids=[f"d{c[3]}-nk{c[2]}-{c[4].name}-{c[5].name}-{c[6].name}-{c[7].name}" for c in STRIDED])
def test_distinct_strides_through_the_c_abi(h, nq, nk, d, ql, kl, vl, ol, ctx, masked):
    """tmdiff_attn_fwd_lse then tmdiff_attn_bwd with four stride triples that all differ: q / k / v / dout lie among NaNs (a read
    outside the [N, D] rows of a head poisons a result), out / dq / dk / dv among sentinels that must all survive.  dq / dk / dv
    take the layouts of q / k / v, dout that of out; lse and the workspace are dense."""
    from tmdiff_amd import _lib, ops
    b, scale = 2, d ** -0.5
    assert len({l.name for l in (ql, kl, vl, ol)}) == 4, "the four layouts must differ from one another"
    assert (ctx_qpw(b, h, nq, nk, d) > 0) == ctx
    dims = {"q": (b, h, nq, d), "k": (b, h, nk, d), "v": (b, h, nk, d), "dout": (b, h, nq, d)}
    lay = {"q": ql, "k": kl, "v": vl, "dout": ol}
    host = {n: randn(seed, *dims[n]) for n, seed in (("q", 41), ("k", 42), ("v", 43), ("dout", 44))}
    ins = {n: _placed(lay[n], float("nan"), dims[n], host[n]) for n in host}
    outs = {n: _placed(lay[src], SENTINEL, dims[src]) for n, src in (("out", "dout"), ("dq", "q"), ("dk", "k"), ("dv", "v"))}
    gaps = {n: _gap_map(lay[src], dims[src]) for n, src in (("out", "dout"), ("dq", "q"), ("dk", "k"), ("dv", "v"))}
    mask = m = None
    if masked:
        mask = torch.rand(b, nk, generator=torch.Generator().manual_seed(3)) > 0.3
        mask[0, :33] = False                       # (the first key tile of sample 0 entirely masked)
        m = mask.to(device="cuda", dtype=torch.uint8).contiguous()
    mp = m.data_ptr() if m is not None else None
    st = lambda t: (C.c_int64 * 3)(*t.stride()[:3])
    qv, kv, vv, gv = (ins[n][1] for n in ("q", "k", "v", "dout"))
    ov, dqv, dkv, dvv = (outs[n][1] for n in ("out", "dq", "dk", "dv"))
    assert ov.stride() == gv.stride() and dqv.stride() == qv.stride() and dkv.stride() == kv.stride() and dvv.stride() == vv.stride()
    lse = torch.empty(b, h, nq, device="cuda")
    ws = torch.empty(_lib.lib.tmdiff_attn_bwd_workspace_bytes(b, h, nq, nk, d) // 4, device="cuda")
    assert ws.numel() >= b * h * nq
    _lib.check(_lib.lib.tmdiff_attn_fwd_lse(qv.data_ptr(), kv.data_ptr(), vv.data_ptr(), ov.data_ptr(), mp, b, h, nq, nk, d,
                                            st(qv), st(kv), st(vv), st(ov), scale, lse.data_ptr(), ops.stream_ptr()), "attn_fwd_lse")
    _lib.check(_lib.lib.tmdiff_attn_bwd(qv.data_ptr(), kv.data_ptr(), vv.data_ptr(), ov.data_ptr(), gv.data_ptr(), lse.data_ptr(),
                                        mp, dqv.data_ptr(), dkv.data_ptr(), dvv.data_ptr(), ws.data_ptr(), b, h, nq, nk, d,
                                        st(qv), st(kv), st(vv), st(ov), scale, ops.stream_ptr()), "attn_bwd")
    torch.cuda.synchronize()
    for n, (flat, view) in outs.items():
        wrong = int((flat[gaps[n]] != SENTINEL).sum())
        assert wrong == 0, f"{n}: {wrong} elements outside the [N, D] rows were written"
        assert bool(torch.isfinite(view).all()), f"{n}: non-finite values, so something outside the input rows was read"
    assert bool(torch.isfinite(lse).all())
    for n, (flat, view) in ins.items():            # the inputs are untouched, and so are the NaNs around them
        assert torch.equal(view.cpu(), host[n]), n
        assert int(torch.isnan(flat).sum()) == flat.numel() - math.prod(dims[n]), n
    ref = _reference(*(merge(host[n]) for n in ("q", "k", "v", "dout")), scale, h, mask)
    what = f"strided d{d} {'mask' if masked else 'nomask'}"
    _check(f"{what} out", merge(ov.cpu()), ref["f32"]["out"], ref["f64"]["out"])
    _lse_error(what, lse, ref["f64"]["lse"])
    got = {n: merge(outs[n][1]) for n in GRADS}
    for n in GRADS:
        _check_grad(f"{what} {n}", got[n], ref["f32"][n], ref["f64"][n])
    # the strides only move staging addresses, never the order of summation: the contiguous call on the same values (this
    # call's out and lse included) gives the same bits
    dense = ops.attention_bwd(merge(qv).contiguous(), merge(kv).contiguous(), merge(vv).contiguous(), merge(ov).contiguous(),
                              merge(gv).contiguous(), lse, scale, heads=h, key_mask=mask)
    for n, g in zip(GRADS, dense):
        assert torch.equal(got[n], g), f"{n}: {int((got[n] != g).sum())} elements differ from the contiguous call"


# ---- B4: masks on every forward route -----------------------------------------------------------------------------------------
MASK_ROUTES = [
    # (H, Nq, Nk, D, lead, route of the forward)
    (2, 130, 77, 16, 32, "generic"),
    (2, 130, 200, 32, 32, "generic"),
    (2, 130, 200, 64, 32, "pipelined"),
    (2, 130, 200, 64, 64, "pipelined"),          # the first two key tiles of sample 1 masked
    (2, 130, 77, 128, 32, "pipelined"),
    (2, 130, 77, 64, 32, "small-context"),
    (2, 130, 77, 80, 32, "generic"),             # DT = 3
]


@pytest.mark.parametrize("h,nq,nk,d,lead,route", MASK_ROUTES, ids=[f"{c[5]}-d{c[3]}-nk{c[2]}-lead{c[4]}" for c in MASK_ROUTES])
def test_masks_on_every_forward_route(h, nq, nk, d, lead, route):
    """Sample 0: every key masked; sample 1: the first `lead` keys masked; sample 2: only the last key kept.  Nk is no multiple
    of 32 (padded key slots in the last tile) and, at 200, crosses a key workgroup of the dK/dV kernel."""
    from tmdiff_amd import ops
    assert nk % 32 != 0
    # attn_forward's dispatch: the small-context kernel where the library says so, else the pipelined one at D = 64 / 128
    assert (ctx_qpw(3, h, nq, nk, d) > 0) == (route == "small-context")
    assert (d in (64, 128)) == (route != "generic")
    scale = d ** -0.5
    q, k, v, dout = randn(31, 3, nq, h * d), randn(32, 3, nk, h * d), randn(33, 3, nk, h * d), randn(34, 3, nq, h * d)
    mask = torch.zeros(3, nk, dtype=torch.bool)
    mask[1, lead:] = True
    mask[2, -1] = True
    c = _reference(q, k, v, dout, scale, h, mask)
    f32, f64 = c["f32"], c["f64"]
    out, lse, (dq, dk, dv) = W._device_backward(c)
    assert torch.equal(out, ops.attention(q.cuda(), k.cuda(), v.cuda(), scale, heads=h, key_mask=mask))
    what = f"{route} d{d} nk{nk} lead{lead}"
    # LSE: -FLT_MAX exactly on a fully masked sample (the backward recognises it by that value)
    assert torch.equal(lse[0].cpu(), torch.full((h, nq), FILL)), f"{what}: LSE of the fully masked sample is not -FLT_MAX"
    _lse_error(what, lse[1:], f64["lse"][1:])
    dq, dk, dv = dq.cpu(), dk.cpu(), dv.cpu()
    # sample 0: uniform P = 1 / Nk, no gradient to the scores; dv = (1 / Nk) sum_q dO within the elementwise bound of
    # test_gpu_attention_bwd.test_masked_keys: a float32 sum of Nq terms in any order, the roundings of 1 / Nk and of the product
    assert not dq[0].any() and not dk[0].any()
    g = dout[0].double()
    want = g.sum(0, keepdim=True).expand(nk, h * d) / nk
    bound = (nq + 2) * U24 * g.abs().sum(0, keepdim=True) / nk
    excess = float(((dv[0].double() - want).abs() / bound).max())
    print(f"{what} all-masked dv against (1/Nk) sum_q dO: worst error / bound {excess:.3f}")
    assert excess <= 1.0
    # sample 1: masked keys get exact zeros, the rest the yardstick bound
    assert not dk[1, :lead].any() and not dv[1, :lead].any()
    assert dk[1, lead:].any() and dv[1, lead:].any()
    for name, t in zip(GRADS, (dq, dk, dv)):
        _check_grad(f"{what} sample 1 {name}", t[1], f32[name][1], f64[name][1])
    # sample 2: one kept key, P = 1 on it
    assert not dk[2, :-1].any() and not dv[2, :-1].any()
    _check(f"{what} sample 2 dv of the kept key", dv[2, -1], f32["dv"][2, -1], f64["dv"][2, -1])
    assert not f64["dq"][2].any() and not f64["dk"][2].any()
    # dS = P (dP - Delta) with dP and Delta two float32 sums of the same D products in any order:
    # |dP - Delta| <= 2 D 2^-24 sum_d |dO_d V_d|; then dq = scale dS K_last, dk_last = scale sum_q dS_q Q_q
    qh, kh, vh, gh = (split(t, h)[2].double() for t in (q, k, v, dout))                 # [H, N, D]
    slack = 2 * d * U24 * (gh * vh[:, -1:, :]).abs().sum(-1, keepdim=True)            # [H, Nq, 1]
    bound_dq = scale * kh[:, -1:, :].abs() * slack                                      # [H, Nq, D]
    bound_dk = scale * (qh.abs() * slack).sum(1)                                        # [H, D]
    got_dq, got_dk = split(dq, h)[2].double(), split(dk, h)[2][:, -1, :].double()
    print(f"{what} sample 2: dq {'exactly 0' if not got_dq.any() else 'max |dq| / bound %.3f' % float((got_dq.abs() / bound_dq).max())}, "
          f"dk {'exactly 0' if not got_dk.any() else 'max |dk| / bound %.3f' % float((got_dk.abs() / bound_dk).max())}")
    assert bool((got_dq.abs() <= bound_dq).all()) and bool((got_dk.abs() <= bound_dk).all())


# ---- B5: stressed logits ------------------------------------------------------------------------------------------------------
# MARGIN: test_gpu_attention_edges.py derives 8 for the same two effects (one sequential fma chain where the CPU sums in vector
# lanes: 4 x; __expf / expf far from 0 and the per-tile rescale: 2 x).  On top of it the backward re-forms P = exp(S - LSE) from a
# STORED float32 LSE: its rounding alone is a relative error of up to |LSE| 2^-24 on every P of a row, hence on dS and on every
# gradient.  The float32 eager path never stores a statistic, so the yardstick has no counterpart to that term.
MARGIN = 8.0
STRESS_SHAPES = [(2, 2, 130, 100, 32), (2, 2, 130, 77, 80), (2, 2, 130, 200, 64), (2, 2, 130, 150, 128), (2, 2, 130, 77, 64)]
STRESS_IDS = ["generic-d32", "generic-d80", "dma-d64", "dma-d128", "ctx-d64"]


@functools.lru_cache(maxsize=None)
def _stress_case(kind, b, h, nq, nk, d):
    q, k, v = (merge(t) for t in stressed_inputs(kind, b, h, nq, nk, d))
    return _reference(q, k, v, randn(56, b, nq, h * d), d ** -0.5, h, None)


@pytest.mark.parametrize("kind", ["peaked", "offset", "mixed"])
@pytest.mark.parametrize("b,h,nq,nk,d", STRESS_SHAPES, ids=STRESS_IDS)
def test_stressed_logits_backward(b, h, nq, nk, d, kind):
    """Peaked, offset and mixed-magnitude logits: |LSE| reaches the hundreds.  Bound per gradient on rel-L2:
    MARGIN x yardstick + 2^-24 max|LSE| + float32 epsilon."""
    c = _stress_case(kind, b, h, nq, nk, d)
    f32, f64 = c["f32"], c["f64"]
    yard = {n: _rel_l2(f32[n], f64[n]) for n in GRADS}
    for n in GRADS:
        assert bool(torch.isfinite(f64[n]).all()), f"degenerate input: non-finite float64 {n}"
        assert float(f64[n].norm()) > 0, f"degenerate input: float64 {n} is zero"
        assert 0 < yard[n] < float("inf"), f"degenerate float32 yardstick for {n}: {yard[n]}"
    lse_term = U24 * float(f64["lse"].abs().max())
    _, _, grads = W._device_backward(c)
    failed = []
    for n, g in zip(GRADS, grads):
        assert bool(torch.isfinite(g).all()), n
        err, bound = _rel_l2(g, f64[n]), MARGIN * yard[n] + lse_term + EPS32
        print(f"stressed {kind:7s} D={d:3d} Nk={nk:3d} {n}: kernel {err:.3e}  float32 eager {yard[n]:.3e}  ratio {err / yard[n]:.2f}  "
              f"2^-24 max|LSE| {lse_term:.3e}  bound {bound:.3e}  error / bound {err / bound:.3f}")
        if err > bound:
            failed.append(f"{n}: rel-L2 {err:.3e} > {bound:.3e}")
    assert not failed, f"{kind} logits: " + "; ".join(failed)


# ---- B6: the LSE store with several query blocks per wave -------------------------------------------------------------------------
LSE_MULTI_BLOCK = [((16, 8, 2048, 77, 256), False), ((64, 8, 1025, 77, 1024), False), ((16, 8, 2048, 77, 256), True)]


@pytest.mark.parametrize("shape,masked", LSE_MULTI_BLOCK, ids=[f"{ids(s)}-{'mask' if m else 'nomask'}" for s, m in LSE_MULTI_BLOCK])
def test_lse_several_blocks_per_wave(shape, masked):
    """The small-context kernel stores LSE inside its per-block loop; only with more than 128 queries per workgroup does q0
    advance inside a wave.  The backward kernels do not depend on that choice, so no backward runs at these sizes."""
    from tmdiff_amd import ops
    b, h, nq, nk, qpw = shape
    d, scale = 64, 64 ** -0.5
    assert ctx_qpw(b, h, nq, nk) == qpw, "the launcher's queries-per-workgroup choice changed: pick shapes that reach it again"
    q, k, v = randn(21, b, nq, h * d), randn(22, b, nk, h * d), randn(23, b, nk, h * d)
    mask = None
    if masked:
        mask = torch.rand(b, nk, generator=torch.Generator().manual_seed(2)) > 0.3
        assert bool(mask.any(dim=1).all())
    qc, kc, vc = q.cuda(), k.cuda(), v.cuda()
    out, lse = ops.attention_lse(qc, kc, vc, scale, heads=h, key_mask=mask)
    assert torch.equal(out, ops.attention(qc, kc, vc, scale, heads=h, key_mask=mask))
    want = torch.empty(b, h, nq, dtype=torch.float64)
    for i in range(b):                              # scores only: no V, no backward
        sim = torch.matmul(split(q[i:i + 1], h).double(), split(k[i:i + 1], h).double().transpose(-1, -2)) * scale
        if mask is not None:
            sim = sim.masked_fill(~mask[i][None, None, None, :], FILL)
        want[i] = torch.logsumexp(sim, dim=-1)[0]
    _lse_error(f"{qpw // 128} query blocks per wave", lse, want)
    if qpw == 1024:
        # one (batch, head) of the same data run alone is one block per wave: the same operations on the same operands
        bi, hi = 37, 5
        sl = lambda t: t[bi:bi + 1, :, hi * d:(hi + 1) * d].contiguous()
        assert ctx_qpw(1, 1, nq, nk) == 128
        _, alone = ops.attention_lse(sl(qc), sl(kc), sl(vc), scale, heads=1)
        assert torch.equal(alone[0, 0], lse[bi, hi]), \
            f"8 blocks per wave vs 1: {int((alone[0, 0] != lse[bi, hi]).sum())} of {nq} LSE values differ"


# ---- B7: the remaining `need` combinations --------------------------------------------------------------------------------------
def test_need_dk_only_dv_only_and_nothing():
    c = W._case(W.MASK_CASE)
    _, _, full = W._device_backward(c)
    _, _, (dq, dk, dv) = W._device_backward(c, need=(False, True, False))       # a.dv NULL inside the dK/dV kernel
    assert dq is None and dv is None and torch.equal(dk, full[1])
    _, _, (dq, dk, dv) = W._device_backward(c, need=(False, False, True))       # a.dk NULL
    assert dq is None and dk is None and torch.equal(dv, full[2])
    _, _, none = W._device_backward(c, need=(False, False, False))
    assert tuple(none) == (None, None, None)


# ---- B8: autograd.gemm_nt at its edges --------------------------------------------------------------------------------------------
GEMM_SHAPES = [((1,), 7, 5),          # M = 1: the weight gradient's inner contraction has length 1
               ((3,), 768, 40),
               ((2, 77), 130, 1),     # N = 1: the input gradient's contraction has length 1
               ((2, 64), 128, 128)]
# variant: (bias, residual, the tensors that require a gradient)
GEMM_VARIANTS = {"bias": (True, False, "awb"), "nobias": (False, False, "aw"), "residual": (True, True, "awbr"),
                 "a_only": (True, True, "a"), "w_only": (True, True, "w")}
GEMM_OUTPUTS = (("da", "a"), ("dw", "w"), ("dbias", "b"), ("dresidual", "r"))


def _gemm_grads(fn, tensors, dout, req, dtype, device):
    leaves = {tag: None if t is None else t.to(dtype=dtype, device=device).clone().requires_grad_(tag in req)
              for tag, t in tensors.items()}
    y = fn(leaves["a"], leaves["w"], leaves["b"], leaves["r"])
    y.backward(dout.to(dtype=dtype, device=device))
    got = {"y": y.detach()}
    got.update({name: None if leaves[tag] is None else leaves[tag].grad for name, tag in GEMM_OUTPUTS})
    return got


def _linear(a, w, bias, residual):
    y = F.linear(a, w, bias)
    return y if residual is None else y + residual


@pytest.mark.parametrize("variant", sorted(GEMM_VARIANTS))
@pytest.mark.parametrize("lead,k,n", GEMM_SHAPES, ids=[f"{ids(s[0])}x{s[1]}x{s[2]}" for s in GEMM_SHAPES])
def test_gemm_nt_gradients_at_the_edges(lead, k, n, variant):
    """y, da, dw, dbias, dresidual of autograd.gemm_nt against float64 autograd of F.linear(a, w, bias) + residual; gradients
    that were not requested come back as None."""
    from tmdiff_amd import autograd
    has_bias, has_res, req = GEMM_VARIANTS[variant]
    tensors = {"a": randn(61, *lead, k), "w": randn(62, n, k) / k ** 0.5, "b": randn(63, n) if has_bias else None,
               "r": randn(64, *lead, n) if has_res else None}
    dout = randn(65, *lead, n)
    f64 = _gemm_grads(_linear, tensors, dout, req, torch.float64, "cpu")
    f32 = _gemm_grads(_linear, tensors, dout, req, torch.float32, "cpu")
    got = _gemm_grads(autograd.gemm_nt, tensors, dout, req, torch.float32, "cuda")
    what = f"gemm_nt {ids(lead)}x{k}x{n} {variant}"
    assert got["y"].shape == f64["y"].shape
    _check(f"{what} y", got["y"], f32["y"], f64["y"])
    for name, tag in GEMM_OUTPUTS:
        if tag in req:
            assert got[name] is not None and got[name].shape == f64[name].shape, name
            _check(f"{what} {name}", got[name], f32[name], f64[name])
        else:
            assert got[name] is None and f64[name] is None, f"{what}: {name} was not requested"
