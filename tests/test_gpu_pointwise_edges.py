"""The small operators around the convolutions (csrc/pointwise.hip, csrc/haar.hip, the stem / head / linear / channel-sum kernels
of csrc/backward.hip) on the paths the other tests never reach: scalar paths forced by odd sizes or by a base one float off a
16-byte boundary, partly live workgroups, the remainders of every unrolled loop, bank pointers with a row stride, broadcast
rows, the grid-stride loops of the Haar kernels, empty batches, stressed inputs.

The reference throughout is a plain fp64 restatement of the operator on the CPU, written from the formulas in the kernels'
header comments.  Unit-scale inputs are held to the tolerance the suite already holds that operator to (UNIT below).  Stressed
inputs are bounded as test_gpu_attention_edges.py does it: MARGIN x the error of the same formula evaluated in plain fp32 on the
CPU, measured in the test, with the unit-scale tolerance (relative to the largest value of the case) as the floor.

Calls through the C ABI use padded buffers: inputs lie between NaNs (a read outside them poisons the result), outputs between
sentinels, every one of which must survive.  Every line printed with the prefix "r08" is a measured figure
(profiles/r08_pointwise_edges.txt).
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close, rel_err
from oracle.haar_ref import haar_dwt2d as dwt_ref, haar_idwt2d as idwt_ref
from oracle.make_golden import randn

pytestmark = pytest.mark.gpu

UNIT = {"stem": 1e-6, "haar": 1e-6, "gamma": 1e-6, "head": 2e-6, "linear": 2e-6, "grad": 1e-5}
MARGIN = 8.0            # as the attention kernels: test_gpu_attention_edges.py
SENTINEL = -777.25
PAD = 64                # floats before and behind every padded buffer (a multiple of 4: `off` alone decides the alignment)
NAN = float("nan")
F64, F32 = torch.float64, torch.float32


# ---- helpers ----------------------------------------------------------------------------------------------------------------
def cu(t):
    return t.cuda().contiguous()


class Guard:
    """A window of `shape`, PAD + off floats into a flat device buffer filled with `fill` (NaN around inputs, SENTINEL around
    outputs).  off = 1 puts the window one float off a 16-byte boundary."""

    def __init__(self, shape, fill, off=0, data=None):
        n = math.prod(shape)
        self.flat = torch.full((PAD + off + n + PAD,), fill, device="cuda", dtype=F32)
        self.lo, self.hi = PAD + off, PAD + off + n
        self.view = self.flat[self.lo:self.hi].view(shape)
        self.ptr = self.flat.data_ptr() + 4 * self.lo
        assert (self.ptr % 16 == 0) == (off % 4 == 0)
        if data is not None:
            self.view.copy_(data)

    def result(self, what):
        """the window on the CPU, after checking that nothing around it was written and that it holds no NaN / inf"""
        for part in (self.flat[:self.lo], self.flat[self.hi:]):
            assert torch.equal(part, torch.full_like(part, SENTINEL)), f"{what}: wrote outside the output"
        got = self.view.cpu()
        assert bool(torch.isfinite(got).all()), f"{what}: non-finite output (something outside the inputs was read?)"
        return got


def gin(t, off=0):
    return None if t is None else Guard(tuple(t.shape), NAN, off, t)


def gout(shape, off=0):
    return Guard(tuple(shape), SENTINEL, off)


def ptr(g):
    return None if g is None else g.ptr


def call(name, *args):
    from tmdiff_amd import _lib, ops
    _lib.check(getattr(_lib.lib, name)(*args, ops.stream_ptr()), name)
    torch.cuda.synchronize()


def refused(name, *args):
    """status and message of a call that must not launch"""
    from tmdiff_amd import _lib, ops
    rc = getattr(_lib.lib, name)(*args, ops.stream_ptr())
    torch.cuda.synchronize()
    return rc, _lib.lib.tmdiff_last_error_string().decode()


def bank(kind, rows):
    """rows [B, C] (CPU) as a per-(sample, channel) bank -> (pointer, stride argument, the rows the kernel must see, keep-alive).
    dense: [B, C], stride 0;  bank: rows of C + 5 floats inside NaNs, 3 floats into the buffer;  bcast: row 0 for every sample."""
    if kind is None:
        return None, 0, None, None
    b, c = rows.shape
    if kind == "dense":
        t = cu(rows)
        return t.data_ptr(), 0, rows, t
    if kind == "bcast":
        t = cu(rows[:1])
        return t.data_ptr(), -1, rows[:1].expand(b, c), t
    assert kind == "bank"
    stride = c + 5
    buf = torch.full((b * stride + 8,), NAN, device="cuda", dtype=F32)
    buf.as_strided((b, c), (stride, 1), 3).copy_(rows)
    return buf.data_ptr() + 12, stride, rows, buf


def silu(x):
    return x * torch.sigmoid(x)


def dsilu(u):
    """d silu / du by autograd, in the dtype of u"""
    u = u.detach().clone().requires_grad_(True)
    (g,) = torch.autograd.grad(silu(u).sum(), u)
    return g


def unit(op, case, got, want, tol):
    m, l2 = rel_err(got, want)
    print(f"\nr08 unit {op} {case}: max-rel {m:.3e} rel-L2 {l2:.3e} (<= {tol:g})")
    assert_close(got, want, tol, tol, f"{op} {case}")


def stressed(op, case, got, want, want32, tol):
    """MARGIN x the fp32 CPU evaluation's own error, floor: the unit-scale tolerance relative to the largest value"""
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0, "degenerate reference"
    assert bool(torch.isfinite(got).all()), f"{op} {case}: non-finite output"
    yard, err = rel_err(want32, want), rel_err(got, want)
    ratio = [e / y if y > 0 else float("inf") if e > 0 else 0.0 for e, y in zip(err, yard)]
    print(f"\nr08 stress {op} {case}: fp32 CPU max-rel {yard[0]:.3e} rel-L2 {yard[1]:.3e}; kernel max-rel {err[0]:.3e} "
          f"rel-L2 {err[1]:.3e}; ratio {ratio[0]:.2f} / {ratio[1]:.2f}; bound {max(MARGIN * yard[0], tol):.3e}")
    assert_close(got, want, max(MARGIN * yard[0], tol), max(MARGIN * yard[1], tol), f"{op} {case} (stressed)")


# ---- stem: y[b, co, p] = act(w[co] * x[b, p] + bias[co]) * out_scale[b, co] ----------------------------------------------------
def stem_ref(x, w, bias, act, osc, dtype):
    """x [B, P], w / bias [C0], osc [B, C0] -> [B, C0, P]"""
    u = w.to(dtype)[None, :, None] * x.to(dtype)[:, None, :]
    if bias is not None:
        u = u + bias.to(dtype)[None, :, None]
    y = silu(u) if act else u
    return y if osc is None else y * osc.to(dtype)[:, :, None]


def stem_x(form, d, dtype):
    """the stem's input [B, P] in `dtype`: xin, or pan (broadcast over the N bands) - ms"""
    if form == "x":
        return d["xin"].to(dtype).flatten(1)
    return (d["pan"].to(dtype) - d["ms"].to(dtype)).flatten(1)


def stem_inputs(form, b, n, h, w, seed=100, scale=1.0):
    if form == "x":
        return {"xin": scale * randn(seed, b, n, h, w)}
    return {"pan": scale * randn(seed + 1, b, 1, h, w), "ms": scale * randn(seed + 2, b, n, h, w)}


def stem_call(d, w, bias, act, osc_kind, osc_rows, off, b, c0, n, h, wd):
    g = {k: gin(v, off) for k, v in d.items()}
    gw, gb = gin(w), gin(bias)
    y = gout((b, c0, n * h * wd), off)
    op, ostride, rows, keep = bank(osc_kind, osc_rows)
    call("tmdiff_stem_fwd_scaled", ptr(g.get("xin")), ptr(g.get("pan")), ptr(g.get("ms")), gw.ptr, ptr(gb), op, ostride, y.ptr,
         b, c0, n, h, wd, 1 if act else 0)
    return y.result("stem"), rows


# (form, silu, bias, out_scale kind, offset of inputs and output in floats)
STEM_VARIANTS = [("x", True, True, None, 0), ("pm", True, True, "dense", 0), ("x", False, True, "bank", 0),
                 ("pm", True, False, "bcast", 0), ("x", True, True, "bank", 1), ("pm", False, False, None, 1),
                 ("pm", True, True, "bank", 1)]


@pytest.mark.parametrize("c0", [1, 5, 8])
@pytest.mark.parametrize("n,h,wd", [(1, 2, 2), (3, 6, 10), (4, 5, 7), (5, 12, 20)],
                         ids=["P4", "P180", "HW35-scalar", "P1200-second-workgroup"])
def test_stem_edges(c0, n, h, wd):
    """H*W = 35 and every off = 1 variant run stem_kernel<1>; P = 1200 is 300 float4 items, so the second workgroup of
    stem_kernel<4> has 44 live threads; silu off, no bias, out_scale as a tensor / a bank pointer with a row stride / one row."""
    b = 2
    w, bias, osc = randn(110, c0), randn(111, c0), 1 + 0.3 * randn(112, b, c0)
    for form, act, has_bias, kind, off in STEM_VARIANTS:
        d = stem_inputs(form, b, n, h, wd)
        got, rows = stem_call(d, w, bias if has_bias else None, act, kind, osc, off, b, c0, n, h, wd)
        want = stem_ref(stem_x(form, d, F64), w, bias if has_bias else None, act, rows, F64)
        unit("stem", f"C0={c0} NHW={n}x{h}x{wd} {form} silu={act} bias={has_bias} scale={kind} off={off}", got, want, UNIT["stem"])


def test_stem_wrapper_out_scale_forms():
    """ops.stem with out_scale as a tensor and as a raw bank pointer + row stride gives the same bits as the C-ABI call."""
    from tmdiff_amd import ops
    b, c0, n, h, wd = 2, 5, 3, 6, 10
    w, bias, osc = randn(110, c0), randn(111, c0), 1 + 0.3 * randn(112, b, c0)
    d = stem_inputs("pm", b, n, h, wd)
    want = stem_ref(stem_x("pm", d, F64), w, bias, True, osc, F64).reshape(b, c0, n, h, wd)
    y_t = ops.stem(cu(w), cu(bias), c0, pan=cu(d["pan"]), ms=cu(d["ms"]), out_scale=cu(osc)).cpu()
    op, stride, _, keep = bank("bank", osc)
    y_p = ops.stem(cu(w), cu(bias), c0, pan=cu(d["pan"]), ms=cu(d["ms"]), out_scale=op, out_scale_stride=stride).cpu()
    unit("stem", "ops.stem(out_scale=tensor)", y_t, want, UNIT["stem"])
    assert torch.equal(y_t, y_p)
    y_plain = ops.stem(cu(w), None, c0, xin=cu(d["ms"]), silu=False).cpu()
    unit("stem", "ops.stem(silu=False, bias=None)", y_plain, stem_ref(d["ms"].flatten(1), w, None, False, None, F64).reshape(y_plain.shape),
         UNIT["stem"])


@pytest.mark.parametrize("form", ["x", "pm"])
def test_stem_stressed_preactivations(form):
    """Pre-activations up to +-100: __expf(-u) overflows to inf (silu -> -0) and underflows to 0 (silu -> u)."""
    b, c0, n, h, wd = 2, 5, 3, 6, 10
    w, bias, osc = randn(120, c0), randn(121, c0), 1 + 0.3 * randn(122, b, c0)
    d = stem_inputs(form, b, n, h, wd)
    w = w * (100.0 / float((w[None, :, None] * stem_x(form, d, F32)[:, None, :]).abs().max()))
    for off in (0, 1):
        got, _ = stem_call(d, w, bias, True, "dense", osc, off, b, c0, n, h, wd)
        want = stem_ref(stem_x(form, d, F64), w, bias, True, osc, F64)
        assert float(want.abs().max()) > 30
        stressed("stem", f"{form} |u|<=100 off={off}", got, want, stem_ref(stem_x(form, d, F32), w, bias, True, osc, F32), UNIT["stem"])


# ---- head: y[b, p] = sum_c (w[c] * scale[b, c]) * silu(x[b, c, p]) --------------------------------------------------------------
def head_ref(sx, w, rows, dtype):
    """sx = silu(x) [B, C, P] in `dtype`"""
    ws = w.to(dtype)[None, :].expand(sx.shape[0], -1) if rows is None else w.to(dtype)[None, :] * rows.to(dtype)
    return torch.einsum("bc,bcp->bp", ws, sx)


def head_call(x, w, kind, rows, off):
    b, c, p = x.shape
    gx, gw, y = gin(x, off), gin(w), gout((b, p), off)
    sp, sstride, seen, keep = bank(kind, rows)
    call("tmdiff_head_fwd", gx.ptr, gw.ptr, sp, sstride, y.ptr, b, c, p)
    return y.result("head"), seen


HEAD_VARIANTS = [("dense", 0), (None, 0), ("bank", 1), ("bcast", 0)]


@pytest.mark.parametrize("c", [1, 6, 257, 4096])
def test_head_edges(c):
    """C = 257 / 4096: the LDS fill loop takes 2 / 16 trips; P = 3 and 1030 run head_kernel<1> (1030: a last workgroup with 6 live
    threads), P = 1028 is 257 float4 items (one live thread in the second workgroup), off = 1 forces the scalar path at P = 1024."""
    b = 2
    w, s = randn(130, c) / c ** 0.5, 1 + 0.2 * randn(131, b, c)
    for p in (3, 1024, 1028, 1030):
        x = randn(132, b, c, p)
        sx = silu(x.double())
        for kind, off in HEAD_VARIANTS:
            got, seen = head_call(x, w, kind, s, off)
            unit("head", f"C={c} P={p} scale={kind} off={off}", got, head_ref(sx, w, seen, F64), UNIT["head"])


def test_head_stressed_activations():
    b, c, p = 2, 6, 1030
    w, s = randn(130, c), 1 + 0.2 * randn(131, b, c)
    x = (30.0 * randn(133, b, c, p)).clamp(-100.0, 100.0)
    x[0, 0, :4] = torch.tensor([100.0, -100.0, 88.8, -88.8])
    want, want32 = head_ref(silu(x.double()), w, s, F64), head_ref(silu(x), w, s, F32)
    for off in (0, 1):
        got, _ = head_call(x, w, "dense", s, off)
        stressed("head", f"|x|<=100 off={off}", got, want, want32, UNIT["head"])


# ---- linear: y = act(x @ w^T + bias) ------------------------------------------------------------------------------------------
def linear_ref(x, w, bias, act, dtype):
    y = F.linear(x.to(dtype), w.to(dtype), None if bias is None else bias.to(dtype))
    return silu(y) if act else y


def linear_call(x, w, bias, act):
    (b, i), o = x.shape, w.shape[0]
    gx, gw, gb, y = gin(x), gin(w), gin(bias), gout((b, o))
    call("tmdiff_linear_fwd", gx.ptr, gw.ptr, ptr(gb), y.ptr, b, i, o, 1 if act else 0)
    return y.result("linear")


# each list varied on its own from the base case (B, I, O) = (5, 100, 7)
LINEAR_CASES = [(5, i, 7) for i in (1, 63, 64, 65, 1023, 1024)] + [(b, 100, 7) for b in (1, 2, 3, 4, 5, 6)] + \
               [(5, 100, o) for o in (1, 3, 4, 5)]


@pytest.mark.parametrize("b,i,o", LINEAR_CASES, ids=[f"B{b}-I{i}-O{o}" for b, i, o in LINEAR_CASES])
def test_linear_edges(b, i, o):
    x, w, bias = randn(140, b, i), randn(141, o, i) / i ** 0.5, randn(142, o)
    for act in (False, True):
        for bv in (bias, None):
            got = linear_call(x, w, bv, act)
            unit("linear", f"B={b} I={i} O={o} act={act} bias={bv is not None}", got, linear_ref(x, w, bv, act, F64), UNIT["linear"])


@pytest.mark.parametrize("kind", ["preact100", "mixed"])
def test_linear_stressed(kind):
    b, i, o = 5, 100, 7
    x, w, bias = randn(143, b, i), randn(144, o, i) / i ** 0.5, randn(145, o)
    if kind == "preact100":       # pre-activations up to +-100 under SiLU
        x = x * (100.0 / float(F.linear(x, w).abs().max()))
    else:                         # magnitudes from 1e-3 to 1e3 inside every row of x
        x = x * 10.0 ** (6.0 * torch.rand(b, i, generator=torch.Generator().manual_seed(146)) - 3.0)
    for act in (False, True):
        got = linear_call(x, w, bias, act)
        stressed("linear", f"{kind} act={act}", got, linear_ref(x, w, bias, act, F64), linear_ref(x, w, bias, act, F32), UNIT["linear"])


# ---- timestep features --------------------------------------------------------------------------------------------------------
T_VALUES = [0.0, 1.0, 999.0, 1000.0, 0.5, 123.456, 999.75, 0.001, 500.25]


@pytest.mark.parametrize("b,dim", [(1, 2), (3, 7), (9, 32), (40, 33)])
def test_gamma_edges(b, dim):
    """Odd dim (the zero pad), dim = 2, B * dim = 1320 crossing one workgroup; integer t in {0, 1, 999, 1000} and fractional t at
    frequency 1, i.e. arguments of ~1000 rad.  The product t * f is rounded to fp32 as the kernel rounds it (that rounding is
    the definition's, worth ~6e-5 at 1000 rad), cos / sin of it are taken in fp64."""
    half = dim // 2
    for shift in (0, 4):
        t = torch.tensor([T_VALUES[(k + shift) % len(T_VALUES)] for k in range(b)], dtype=F32)
        freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=F32) / half)
        assert float(freqs[0]) == 1.0
        gt, gf, emb = gin(t), gin(freqs), gout((b, dim))
        call("tmdiff_gamma_embedding", gt.ptr, gf.ptr, emb.ptr, b, dim)
        got = emb.result("gamma")
        arg = (t[:, None] * freqs[None, :]).double()          # the fp32 product, then fp64
        want = torch.zeros(b, dim, dtype=F64)
        want[:, :half], want[:, half:2 * half] = torch.cos(arg), torch.sin(arg)
        if dim % 2:
            assert torch.equal(got[:, -1], torch.zeros(b)), "the pad column of an odd dim is not zero"
        gap = float((got.double() - want).abs().max())
        print(f"\nr08 unit gamma B={b} dim={dim} t0={float(t[0])}: max abs gap {gap:.3e} (<= {UNIT['gamma']:g})")
        assert gap <= UNIT["gamma"], f"gamma B={b} dim={dim}: max abs gap {gap:.3e}"


def test_limits_are_refused():
    """C = 4097 (head) and I = 1025 (linear) are errors, never launches."""
    from tmdiff_amd import ops
    from tmdiff_amd._lib import TmdiffError
    z = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(TmdiffError, match="head_fwd"):
        ops.head(z(1, 4097, 1, 1, 4), z(4097), z(1, 4097))
    with pytest.raises(TmdiffError, match="linear_fwd"):
        ops.linear(z(2, 1025), z(3, 1025), z(3))


# ---- Haar DWT / IDWT ----------------------------------------------------------------------------------------------------------
def plane_prologue(shift, scale, c, n, act):
    """(ctypes reference, keep-alive); shift / scale: (kind, rows [B, C]) or None"""
    from tmdiff_amd import _lib
    q = _lib.PlanePrologue()
    shp, shs, sh_rows, k1 = bank(*shift) if shift else (None, 0, None, None)
    scp, scs, sc_rows, k2 = bank(*scale) if scale else (None, 0, None, None)
    q.shift, q.scale, q.shift_stride, q.scale_stride = shp, scp, shs, scs
    q.C, q.n_per_channel, q.act = c, n, 1 if act else 0
    return q, (sh_rows, sc_rows), (k1, k2)


def prologue_ref(v, rows, n, act, dtype):
    """v [B * C * N, ., .] -> act(v + shift[b, c]) * scale[b, c]"""
    sh, sc = rows
    per_plane = lambda r: r.to(dtype).repeat_interleave(n, dim=1).reshape(-1)[:, None, None]
    t = v if sh is None else v + per_plane(sh)
    t = silu(t) if act else t
    return t if sc is None else t * per_plane(sc)


def dwt_call(x, ll_scale=0.5, hi_scale=1.5, off=0, want_high=True, pro=None, name="tmdiff_haar_dwt2d_pro"):
    planes, hh_, ww = x.shape
    gx = gin(x, off)
    outs = [gout((planes, hh_ // 2, ww // 2), off) for _ in range(4 if want_high else 1)]
    ptrs = [o.ptr for o in outs] + [None] * (4 - len(outs))
    extra = (C.byref(pro) if pro is not None else None,) if name.endswith("_pro") else ()
    call(name, gx.ptr, *ptrs, planes, hh_, ww, ll_scale, hi_scale, *extra)
    return [o.result("dwt band") for o in outs]


def idwt_call(lls, his, in_scale=2.0, off=0, pro=None, stacked=None):
    """lls: 1 or 2 low bands [planes, h, w]; his: three bands, or None (zero high bands), or stacked = [B, 3 * ppb, h, w]"""
    planes, h, w = lls[0].shape
    gl = [gin(t, off) for t in lls]
    outs = [gout((planes, 2 * h, 2 * w), off) for _ in lls]
    arr = lambda gs: (C.c_void_p * 2)(*[g.ptr for g in gs], *([None] * (2 - len(gs))))
    if stacked is not None:
        ppb = stacked.shape[1] // 3
        gs = gin(stacked, off)
        hp = (gs.ptr, gs.ptr + 4 * ppb * h * w, gs.ptr + 8 * ppb * h * w, ppb, 3 * ppb * h * w)
    elif his is not None:
        gh = [gin(t, off) for t in his]
        hp = (*[g.ptr for g in gh], 0, 0)
    else:
        hp = (None, None, None, 0, 0)
    call("tmdiff_haar_idwt2d_pro", arr(gl), len(lls), *hp, arr(outs), planes, h, w, in_scale, C.byref(pro) if pro is not None else None)
    return [o.result("idwt output") for o in outs]


HAAR_SMALL = [(1, 2, 2), (3, 6, 10), (2, 8, 16), (5, 4, 24)]      # W = 16, 24: float4 path; W = 2, 10: scalar path


@pytest.mark.parametrize("planes,hh_,ww", HAAR_SMALL)
def test_haar_small_shapes(planes, hh_, ww):
    """ll_scale and hi_scale != 1, the LL-only form, both alignments; where the float4 path runs, the same values through the
    scalar path (a copy one float off) give the same bits, and so do the per-operator ABI names."""
    x = randn(150, planes, hh_, ww)
    want = [s * t for s, t in zip((0.5, 1.5, 1.5, 1.5), dwt_ref(x.double()))]
    runs = {off: dwt_call(x, off=off) for off in (0, 1)}
    for off, got in runs.items():
        for name, g, wnt in zip(("ll", "lh", "hl", "hh"), got, want):
            unit("haar", f"dwt {planes}x{hh_}x{ww} {name} off={off}", g, wnt, UNIT["haar"])
    for a, b_ in zip(runs[0], runs[1]):
        assert torch.equal(a, b_), "dwt: the float4 and the scalar path differ in bits"
    for a, b_ in zip(runs[0], dwt_call(x, name="tmdiff_haar_dwt2d_fwd")):
        assert torch.equal(a, b_), "tmdiff_haar_dwt2d_fwd differs from tmdiff_haar_dwt2d"
    for off in (0, 1):
        only = dwt_call(x, off=off, want_high=False)
        assert len(only) == 1 and torch.equal(only[0], runs[0][0])
    # IDWT: one and two low bands, zero high bands
    h, w = hh_ // 2, ww // 2
    ll0, ll1, lh, hl, hh = (randn(151 + k, planes, h, w) for k in range(5))
    d = lambda t: t.double()
    want0, want1 = idwt_ref(2.0 * d(ll0), d(lh), d(hl), d(hh)), idwt_ref(2.0 * d(ll1), d(lh), d(hl), d(hh))
    zero = torch.zeros(planes, h, w, dtype=F64)
    want_z = idwt_ref(2.0 * d(ll0), zero, zero, zero)
    runs = {}
    for off in (0, 1):
        g0, g1 = idwt_call([ll0, ll1], [lh, hl, hh], off=off)
        unit("haar", f"idwt {planes}x{h}x{w} n_ll=2 out0 off={off}", g0, want0, UNIT["haar"])
        unit("haar", f"idwt {planes}x{h}x{w} n_ll=2 out1 off={off}", g1, want1, UNIT["haar"])
        (gz,) = idwt_call([ll0], None, off=off)
        unit("haar", f"idwt {planes}x{h}x{w} zero high bands off={off}", gz, want_z, UNIT["haar"])
        (g_one,) = idwt_call([ll0], [lh, hl, hh], off=off)
        assert torch.equal(g_one, g0), "idwt: n_ll = 1 and n_ll = 2 differ in bits"
        runs[off] = (g0, g1, gz)
    for a, b_ in zip(runs[0], runs[1]):
        assert torch.equal(a, b_), "idwt: the float4 and the scalar path differ in bits"
    out = gout((planes, hh_, ww))
    g = [gin(t) for t in (ll0, lh, hl, hh)]
    call("tmdiff_haar_idwt2d_fwd", *[t.ptr for t in g], out.ptr, planes, h, w, 2.0)
    assert torch.equal(out.result("idwt_fwd"), runs[0][0]), "tmdiff_haar_idwt2d_fwd differs from tmdiff_haar_idwt2d"


@pytest.mark.parametrize("h,w", [(3, 5), (2, 6), (4, 8)], ids=["scalar-stride270", "scalar-stride216", "float4"])
def test_haar_idwt_stacked_bands(h, w):
    """High bands as channel slices of [B, 3C, N, h, w] (hi_batch_stride set), two low bands.  3 x 5: the sample stride is no
    multiple of 4 floats, which only the float4 path needs."""
    b, c, n = 2, 3, 2
    ppb, planes = c * n, b * c * n
    ll0, ll1 = randn(160, planes, h, w), randn(161, planes, h, w)
    st = randn(162, b, 3 * ppb, h, w)
    lh, hl, hh = (st[:, k * ppb:(k + 1) * ppb].reshape(planes, h, w).double() for k in range(3))
    want = [idwt_ref(2.0 * t.double(), lh, hl, hh) for t in (ll0, ll1)]
    runs = {}
    for off in (0, 1):
        runs[off] = idwt_call([ll0, ll1], None, off=off, stacked=st)
        for k in range(2):
            unit("haar", f"idwt stacked {h}x{w} out{k} off={off}", runs[off][k], want[k], UNIT["haar"])
    dense = idwt_call([ll0, ll1], [t.float() for t in (lh, hl, hh)])
    for k in range(2):
        assert torch.equal(runs[0][k], runs[1][k]) and torch.equal(runs[0][k], dense[k]), "stacked / dense / scalar differ in bits"


GRID_STRIDE = [(9, 1024, 1024), (3, 1022, 1022)]     # 589 824 float4 items / 783 363 scalar items against 2048 x 256 threads


@pytest.mark.parametrize("planes,hh_,ww", GRID_STRIDE, ids=["float4", "scalar"])
def test_haar_dwt_grid_stride_loop(planes, hh_, ww):
    x = randn(170, planes, hh_, ww)
    assert planes * (hh_ // 2) * (ww // 2 // (4 if ww % 8 == 0 else 1)) > 2048 * 256
    want = [s * t for s, t in zip((0.5, 1.5, 1.5, 1.5), dwt_ref(x.double()))]
    for name, g, wnt in zip(("ll", "lh", "hl", "hh"), dwt_call(x), want):
        unit("haar", f"dwt grid-stride {planes}x{hh_}x{ww} {name}", g, wnt, UNIT["haar"])


@pytest.mark.parametrize("planes,hh_,ww", GRID_STRIDE, ids=["float4", "scalar"])
def test_haar_idwt_grid_stride_loop(planes, hh_, ww):
    h, w = hh_ // 2, ww // 2
    ll, lh, hl, hh = (randn(171 + k, planes, h, w) for k in range(4))
    want = idwt_ref(2.0 * ll.double(), lh.double(), hl.double(), hh.double())
    (got,) = idwt_call([ll], [lh, hl, hh])
    unit("haar", f"idwt grid-stride {planes}x{h}x{w}", got, want, UNIT["haar"])


# (shift kind, scale kind, act)
PROLOGUES = [("dense", None, False), (None, "dense", False), ("dense", "dense", True), ("dense", "dense", False),
             ("bank", "bank", True), ("bcast", "bank", True), ("bank", "bcast", False), (None, None, True)]


@pytest.mark.parametrize("b,c,n", [(2, 3, 2), (3, 8, 1)])
@pytest.mark.parametrize("hh_,ww", [(6, 10), (4, 16)], ids=["scalar", "float4"])
def test_haar_prologues(b, c, n, hh_, ww):
    """tmdiff_haar_dwt2d_pro / tmdiff_haar_idwt2d_pro: shift only, scale only, both, act on and off, bank rows with a stride, a
    broadcast row; n_per_channel = 2 makes plane -> (b, c) a real division.  Only the LL band / the first reconstruction get it."""
    planes, h, w = b * c * n, hh_ // 2, ww // 2
    x = randn(180, planes, hh_, ww)
    sh_rows, sc_rows = randn(181, b, c), 1 + 0.3 * randn(182, b, c)
    bands = dwt_ref(x.double())
    ll0, ll1, lh, hl, hh = (randn(183 + k, planes, h, w) for k in range(5))
    rec = [idwt_ref(2.0 * t.double(), lh.double(), hl.double(), hh.double()) for t in (ll0, ll1)]
    plain = dwt_call(x)
    for sh_kind, sc_kind, act in PROLOGUES:
        q, rows, keep = plane_prologue((sh_kind, sh_rows) if sh_kind else None, (sc_kind, sc_rows) if sc_kind else None, c, n, act)
        case = f"[{b},{c},{n}] {hh_}x{ww} shift={sh_kind} scale={sc_kind} act={act}"
        for off in (0, 1):
            got = dwt_call(x, off=off, pro=q)
            unit("haar", f"dwt prologue {case} off={off}", got[0], prologue_ref(0.5 * bands[0], rows, n, act, F64), UNIT["haar"])
            for k in (1, 2, 3):
                assert torch.equal(got[k], plain[k]), "a high band changed under the LL prologue"
            g0, g1 = idwt_call([ll0, ll1], [lh, hl, hh], off=off, pro=q)
            unit("haar", f"idwt prologue {case} out0 off={off}", g0, prologue_ref(rec[0], rows, n, act, F64), UNIT["haar"])
            unit("haar", f"idwt prologue {case} out1 off={off}", g1, rec[1], UNIT["haar"])


def test_haar_prologue_stressed():
    """LL + shift up to +-100 under SiLU."""
    b, c, n, hh_, ww = 2, 3, 2, 6, 16
    x = randn(190, b * c * n, hh_, ww)
    sh_rows, sc_rows = randn(191, b, c), 1 + 0.3 * randn(192, b, c)
    x = x * (95.0 / float(dwt_ref(x)[0].abs().max()))
    q, rows, keep = plane_prologue(("dense", sh_rows), ("dense", sc_rows), c, n, True)
    want = prologue_ref(dwt_ref(x.double())[0], rows, n, True, F64)
    want32 = prologue_ref(dwt_ref(x)[0], rows, n, True, F32)
    for off in (0, 1):
        stressed("haar", f"dwt prologue |ll + shift|<=100 off={off}", dwt_call(x, ll_scale=1.0, off=off, pro=q)[0], want, want32, UNIT["haar"])


@pytest.mark.parametrize("planes,hh_,ww", [(3, 6, 10), (2, 8, 16)], ids=["scalar", "float4"])
@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_haar_adjointness(planes, hh_, ww, scale):
    """<DWT x, y> = <x, IDWT y> on the device results, summed in fp64, to 1e-6 relative; with ll_scale = in_scale = `scale`, and
    in the LL-only form (IDWT with zero high bands).  y is correlated with DWT x, so neither product is small by cancellation."""
    x = randn(200, planes, hh_, ww)
    y = [a + 0.5 * randn(201 + k, planes, hh_ // 2, ww // 2) for k, a in enumerate(dwt_ref(x))]
    dot = lambda a, b_: float((a.double() * b_.double()).sum())
    dx = dwt_call(x, ll_scale=scale, hi_scale=1.0)
    (ay,) = idwt_call([y[0]], y[1:], in_scale=scale)
    lhs, rhs = sum(dot(a, b_) for a, b_ in zip(dx, y)), dot(x, ay)
    print(f"\nr08 unit haar adjoint {planes}x{hh_}x{ww} scale={scale}: {lhs:.9e} vs {rhs:.9e}, rel {abs(lhs - rhs) / abs(rhs):.2e}")
    assert abs(lhs - rhs) <= 1e-6 * max(abs(lhs), abs(rhs))
    (ll,) = dwt_call(x, ll_scale=scale, want_high=False)
    (ay,) = idwt_call([y[0]], None, in_scale=scale)
    lhs, rhs = dot(ll, y[0]), dot(x, ay)
    print(f"\nr08 unit haar adjoint LL-only {planes}x{hh_}x{ww} scale={scale}: {lhs:.9e} vs {rhs:.9e}, rel {abs(lhs - rhs) / abs(rhs):.2e}")
    assert abs(lhs - rhs) <= 1e-6 * max(abs(lhs), abs(rhs))


def unpack_units(units, c, shape):
    """packed bf16 units [B, C/8, positions, 8] (int16 storage) -> fp32 [B, C, *shape]"""
    return units.view(torch.bfloat16).float().permute(0, 1, 3, 2).reshape(units.shape[0], c, *shape)


@pytest.mark.parametrize("b,c,n,h,w", [(2, 8, 3, 3, 5), (1, 16, 2, 2, 4)])
@pytest.mark.parametrize("with_pro", [False, True], ids=["plain", "prologue"])
def test_haar_pack_bf16_producers(b, c, n, h, w, with_pro):
    """C = 8 and 16, with and without high bands and prologue: the packed LL band / first reconstruction is the fp32 producer's,
    rounded to bf16 (nearest even); the fp32 outputs are the fp32 producer's bits."""
    from tmdiff_amd import ops
    x = cu(randn(210, b, c, n, 2 * h, 2 * w))
    pro = dict(act=True, shift=cu(randn(211, b, c)), scale=cu(1 + 0.3 * randn(212, b, c))) if with_pro else None
    ref = ops.haar_dwt2d(x, want_high=True, ll_scale=0.5, hi_scale=1.5, ll_prologue=pro)
    got = ops.haar_dwt2d(x, want_high=True, ll_scale=0.5, hi_scale=1.5, ll_prologue=pro, pack_bf16=True)
    assert torch.equal(unpack_units(got[0], c, (n, h, w)), ref[0].bfloat16().float())
    for a, b_ in zip(got[1:], ref[1:]):
        assert torch.equal(a, b_)
    only = ops.haar_dwt2d(x, want_high=False, ll_scale=0.5, ll_prologue=pro, pack_bf16=True)
    assert only[1] is None and torch.equal(only[0], got[0])
    want_ll = 0.5 * dwt_ref(x.cpu().double())[0]
    if with_pro:
        want_ll = prologue_ref(want_ll.reshape(b * c * n, h, w), (pro["shift"].cpu(), pro["scale"].cpu()), n, True, F64).reshape(want_ll.shape)
    unit("haar", f"packed LL [{b},{c},{n}] {h}x{w} prologue={with_pro} (bf16: 2^-8)", unpack_units(got[0], c, (n, h, w)).cpu(), want_ll, 2.0 ** -8)
    ll0, ll1, bands = cu(randn(213, b, c, n, h, w)), cu(randn(214, b, c, n, h, w)), cu(randn(215, b, 3 * c, n, h, w))
    r0, r1 = ops.haar_idwt2d([ll0, ll1], None, None, None, in_scale=2.0, stacked_bands=bands, out0_prologue=pro)
    g0, g1 = ops.haar_idwt2d([ll0, ll1], None, None, None, in_scale=2.0, stacked_bands=bands, out0_prologue=pro, pack_bf16=True)
    assert torch.equal(unpack_units(g0, c, (n, 2 * h, 2 * w)), r0.bfloat16().float()) and torch.equal(g1, r1)


def test_haar_pack_bf16_wants_8_byte_aligned_pairs():
    """Both pack kernels move fp32 pairs as 8 bytes: x of the DWT and out1 of the IDWT.  A base that is only 4-byte aligned is an
    error without a launch; an 8-byte aligned one (not 16) is served and gives the bits of the aligned call."""
    from tmdiff_amd import ops
    b, c, n, h, w = 1, 8, 2, 3, 5
    x = cu(randn(220, b, c, n, 2 * h, 2 * w))
    units = torch.zeros(b, c // 8, n * h * w, 8, device="cuda", dtype=torch.int16)
    buf = torch.zeros(x.numel() + 4, device="cuda")
    args = lambda p: (p, units.data_ptr(), None, None, None, b, c, n, 2 * h, 2 * w, 0.5, 1.0, None)
    rc, msg = refused("tmdiff_haar_dwt2d_pack_bf16", *args(buf.data_ptr() + 4))
    assert rc != 0 and "8-byte" in msg and "haar_dwt2d_pack_bf16" in msg, (rc, msg)
    assert not bool(units.any()), "the refused call wrote its output"
    buf[2:2 + x.numel()].copy_(x.flatten())
    call("tmdiff_haar_dwt2d_pack_bf16", *args(buf.data_ptr() + 8))
    assert torch.equal(units, ops.haar_dwt2d(x, want_high=False, ll_scale=0.5, pack_bf16=True)[0])
    ll0, ll1, bands = cu(randn(221, b, c, n, h, w)), cu(randn(222, b, c, n, h, w)), cu(randn(223, b, 3 * c, n, h, w))
    u2 = torch.zeros(b, c // 8, n * 4 * h * w, 8, device="cuda", dtype=torch.int16)
    out = torch.full((4 * ll0.numel() + 4,), SENTINEL, device="cuda")
    args = lambda p: (ll0.data_ptr(), ll1.data_ptr(), bands.data_ptr(), u2.data_ptr(), p, b, c, n, h, w, 2.0, None)
    rc, msg = refused("tmdiff_haar_idwt2d_pack_bf16", *args(out.data_ptr() + 4))
    assert rc != 0 and "8-byte" in msg and "haar_idwt2d_pack_bf16" in msg, (rc, msg)
    assert torch.equal(out, torch.full_like(out, SENTINEL)) and not bool(u2.any()), "the refused call wrote its output"
    call("tmdiff_haar_idwt2d_pack_bf16", *args(out.data_ptr() + 8))
    r0, r1 = ops.haar_idwt2d([ll0, ll1], None, None, None, in_scale=2.0, stacked_bands=bands, pack_bf16=True)
    assert torch.equal(u2, r0) and torch.equal(out[2:-2], r1.flatten()) and bool((out[:2] == SENTINEL).all()) and bool((out[-2:] == SENTINEL).all())


# ---- channel_sum: out[c] = scale * sum_{b, p} x[b, c, p] ---------------------------------------------------------------------------
def channel_sum_call(x, scale):
    b, c, p = x.shape
    gx, out = gin(x), gout((c,))
    call("tmdiff_channel_sum", gx.ptr, out.ptr, b, c, p, scale)
    return out.result("channel_sum")


CHANNEL_SUM = [(2, 1, 5), (3, 3, 2049), (2, 5, 6151), (1, 2100, 300), (0, 4, 64)]


@pytest.mark.parametrize("b,c,p", CHANNEL_SUM)
def test_channel_sum_edges(b, c, p):
    """P = 2049: two slices of 1025 (unrolled trips and a tail in each); 6151: four slices of 1538, the last one shorter; C = 1;
    C = 2100 > 2048: one slice; B = 0: zeros.  The slices meet in float atomics, so the order of additions is not fixed."""
    from tmdiff_amd import ops
    x = randn(230, b, c, p)
    for scale in (1.0, 0.25, -1.7):
        got = channel_sum_call(x, scale)
        if b == 0:
            assert torch.equal(got, torch.zeros(c)), "channel_sum over no samples is not zero"
            continue
        unit("channel_sum", f"[{b},{c},{p}] scale={scale}", got, scale * x.double().sum((0, 2)), UNIT["grad"])
    got = ops.channel_sum(cu(x).reshape(b, c, p, 1), 0.25).cpu()        # (the wrapper: P from the trailing dims, also when B = 0)
    assert got.shape == (c,)
    if b == 0:
        assert torch.equal(got, torch.zeros(c))
    else:
        assert_close(got, 0.25 * x.double().sum((0, 2)), UNIT["grad"], UNIT["grad"], "ops.channel_sum")


@pytest.mark.parametrize("b,c,p", [s for s in CHANNEL_SUM if s[0]])
def test_channel_sum_large_mean(b, c, p):
    x = 1000.0 + randn(231, b, c, p)
    got = channel_sum_call(x, 0.25)
    stressed("channel_sum", f"[{b},{c},{p}] mean 1000", got, 0.25 * x.double().sum((0, 2)), 0.25 * x.sum((0, 2)), UNIT["grad"])


# ---- stem / head / linear backward ---------------------------------------------------------------------------------------------
def stem_bwd_ref(x, w, bias, gy, dtype):
    """x [B, P], gy [B, C0, P] -> dwb [B, C0, 2], dx [B, P] (d/dx of the stem's input)"""
    x, w, gy = x.to(dtype), w.to(dtype), gy.to(dtype)
    u = w[None, :, None] * x[:, None, :] + (0 if bias is None else bias.to(dtype)[None, :, None])
    g = gy * dsilu(u)
    return torch.stack([(g * x[:, None, :]).sum(-1), g.sum(-1)], dim=-1), (g * w[None, :, None]).sum(1)


STEM_BWD_SHAPES = [(1, 4, 5), (4, 8, 8), (3, 10, 10), (5, 2, 103)]       # P = 20, 256, 300, 1030; H * W = 20, 64, 100, 206


@pytest.mark.parametrize("n,h,wd", STEM_BWD_SHAPES, ids=["P20-N1", "P256", "P300", "P1030"])
@pytest.mark.parametrize("form", ["x", "pm"])
def test_stem_backward_edges(n, h, wd, form):
    from tmdiff_amd import ops
    b, c0 = 2, 5
    w, bias = randn(240, c0), randn(241, c0)
    d = stem_inputs(form, b, n, h, wd, seed=242)
    gy = randn(245, b, c0, n, h, wd)
    dev = {k: cu(v) for k, v in d.items()}
    for bv in (bias, None):
        want_dwb, want_dx = stem_bwd_ref(stem_x(form, d, F64), w, bv, gy.flatten(2), F64)
        bd = None if bv is None else cu(bv)
        dwb = ops.stem_bwd(cu(w), bd, cu(gy), **dev).cpu()
        unit("grad", f"stem_bwd {form} NHW={n}x{h}x{wd} bias={bv is not None} dw", dwb[..., 0], want_dwb[..., 0], UNIT["grad"])
        unit("grad", f"stem_bwd {form} NHW={n}x{h}x{wd} bias={bv is not None} db", dwb[..., 1], want_dwb[..., 1], UNIT["grad"])
        want_dx = want_dx.reshape(b, n, h, wd)
        if form == "x":
            dx, none = ops.stem_bwd_input(cu(w), bd, cu(gy), **dev)
            assert none is None
            unit("grad", f"stem_bwd_input x NHW={n}x{h}x{wd} bias={bv is not None}", dx.cpu(), want_dx, UNIT["grad"])
        else:
            for need_x, need_pan in ((True, True), (True, False), (False, True)):
                dms, dpan = ops.stem_bwd_input(cu(w), bd, cu(gy), need_x=need_x, need_pan=need_pan, **dev)
                assert (dms is not None) == need_x and (dpan is not None) == need_pan
                if need_x:
                    unit("grad", f"stem_bwd_input d_ms NHW={n}x{h}x{wd} pan={need_pan}", dms.cpu(), -want_dx, UNIT["grad"])
                if need_pan:
                    unit("grad", f"stem_bwd_input d_pan NHW={n}x{h}x{wd} ms={need_x}", dpan.cpu(), want_dx.sum(1, keepdim=True), UNIT["grad"])


def head_bwd_ref(x, w, rows, gy, dtype):
    """x [B, C, P], gy [B, P] -> dx [B, C, P], dws [B, C]"""
    x, gy = x.to(dtype), gy.to(dtype)
    ws = w.to(dtype)[None, :].expand(x.shape[0], -1) if rows is None else w.to(dtype)[None, :] * rows.to(dtype)
    return gy[:, None, :] * ws[:, :, None] * dsilu(x), (gy[:, None, :] * silu(x)).sum(-1)


@pytest.mark.parametrize("n,h,wd", STEM_BWD_SHAPES, ids=["P20", "P256", "P300", "P1030"])
def test_head_backward_edges(n, h, wd):
    from tmdiff_amd import ops
    b, c = 2, 3
    x, w, s, gy = randn(250, b, c, n, h, wd), randn(251, c), 1 + 0.2 * randn(252, b, c), randn(253, b, n, h, wd)
    for rows in (s, None):
        want_dx, want_dws = head_bwd_ref(x.flatten(2), w, rows, gy.flatten(1), F64)
        sd = None if rows is None else cu(rows)
        dx, dws = ops.head_bwd(cu(x), cu(w), sd, cu(gy))
        unit("grad", f"head_bwd NHW={n}x{h}x{wd} scale={rows is not None} dx", dx.cpu().flatten(2), want_dx, UNIT["grad"])
        unit("grad", f"head_bwd NHW={n}x{h}x{wd} scale={rows is not None} dws", dws.cpu(), want_dws, UNIT["grad"])
        none, dws2 = ops.head_bwd(cu(x), cu(w), sd, cu(gy), need_dx=False)
        assert none is None and torch.equal(dws2, dws)


def test_stem_head_backward_stressed():
    """Pre-activations up to +-100 under SiLU', and upstream gradients of mean 1000 under the sums over the positions."""
    from tmdiff_amd import ops
    b, c0, n, h, wd = 2, 5, 5, 2, 103
    w, bias = randn(260, c0), randn(261, c0)
    d = stem_inputs("pm", b, n, h, wd, seed=262)
    dev = {k: cu(v) for k, v in d.items()}
    x5, wh, s = randn(266, b, c0, n, h, wd), randn(267, c0), 1 + 0.2 * randn(268, b, c0)
    for kind in ("preact100", "mean1000"):
        gy, ws, xh = randn(265, b, c0, n, h, wd), w, x5
        if kind == "preact100":
            ws = w * (100.0 / float((w[None, :, None] * stem_x("pm", d, F32)[:, None, :]).abs().max()))
            xh = (30.0 * x5).clamp(-100.0, 100.0)
        else:
            gy = gy + 1000.0
        want, want32 = (stem_bwd_ref(stem_x("pm", d, dt), ws, bias, gy.flatten(2), dt) for dt in (F64, F32))
        dwb = ops.stem_bwd(cu(ws), cu(bias), cu(gy), **dev).cpu()
        stressed("grad", f"stem_bwd {kind} dw", dwb[..., 0], want[0][..., 0], want32[0][..., 0], UNIT["grad"])
        stressed("grad", f"stem_bwd {kind} db", dwb[..., 1], want[0][..., 1], want32[0][..., 1], UNIT["grad"])
        dms, dpan = ops.stem_bwd_input(cu(ws), cu(bias), cu(gy), need_x=True, need_pan=True, **dev)
        stressed("grad", f"stem_bwd_input {kind} d_ms", dms.cpu().flatten(1), -want[1], -want32[1], UNIT["grad"])
        stressed("grad", f"stem_bwd_input {kind} d_pan", dpan.cpu().flatten(1), want[1].reshape(b, n, -1).sum(1),
                 want32[1].reshape(b, n, -1).sum(1), UNIT["grad"])
        gh = gy[:, 0]
        want, want32 = (head_bwd_ref(xh.flatten(2), wh, s, gh.flatten(1), dt) for dt in (F64, F32))
        dx, dws = ops.head_bwd(cu(xh), cu(wh), cu(s), cu(gh))
        stressed("grad", f"head_bwd {kind} dx", dx.cpu().flatten(2), want[0], want32[0], UNIT["grad"])
        stressed("grad", f"head_bwd {kind} dws", dws.cpu(), want[1], want32[1], UNIT["grad"])


def linear_bwd_ref(x, w, bias, gy, act, dtype):
    x, w = (t.to(dtype).clone().requires_grad_(True) for t in (x, w))
    bv = None if bias is None else bias.to(dtype).clone().requires_grad_(True)
    y = F.linear(x, w, bv)
    (silu(y) if act else y).backward(gy.to(dtype))
    return x.grad, w.grad, None if bv is None else bv.grad


LINEAR_BWD = [(b, 100, o) for b in (1, 5) for o in (1, 4, 13, 16, 17, 29)] + [(b, i, 7) for b in (1, 5) for i in (63, 65)]


@pytest.mark.parametrize("b,i,o", LINEAR_BWD, ids=[f"B{b}-I{i}-O{o}" for b, i, o in LINEAR_BWD])
def test_linear_backward_edges(b, i, o):
    """linear_dx_kernel: each wave takes every 4th row o, 16 rows per unrolled trip, then a tail; I = 63 / 65: one / two k tiles."""
    from tmdiff_amd import ops
    x, w, bias, gy = randn(270, b, i), randn(271, o, i) / i ** 0.5, randn(272, o), randn(273, b, o)
    for act in (False, True):
        for bv in (bias, None):
            want = linear_bwd_ref(x, w, bv, gy, act, F64)
            got = ops.linear_bwd(cu(x), cu(w), None if bv is None else cu(bv), cu(gy), act=act, need_db=bv is not None)
            for name, g, wnt in zip(("dx", "dw", "db"), got, want):
                assert (g is None) == (wnt is None)
                if g is not None:
                    unit("grad", f"linear_bwd B={b} I={i} O={o} act={act} bias={bv is not None} {name}", g.cpu(), wnt, UNIT["grad"])
    dx, dw, db = ops.linear_bwd(cu(x), cu(w), cu(bias), cu(gy), act=True, need_dx=False, need_dw=False)
    assert dx is None and dw is None
    unit("grad", f"linear_bwd B={b} I={i} O={o} db alone", db.cpu(), linear_bwd_ref(x, w, bias, gy, True, F64)[2], UNIT["grad"])


def test_linear_backward_stressed():
    """linear_gu_kernel with SiLU' at pre-activations up to +-100."""
    from tmdiff_amd import ops
    b, i, o = 5, 100, 29
    x, w, bias, gy = randn(274, b, i), randn(275, o, i) / i ** 0.5, randn(276, o), randn(277, b, o)
    x = x * (100.0 / float(F.linear(x, w).abs().max()))
    want, want32 = linear_bwd_ref(x, w, bias, gy, True, F64), linear_bwd_ref(x, w, bias, gy, True, F32)
    got = ops.linear_bwd(cu(x), cu(w), cu(bias), cu(gy), act=True)
    for name, g, wnt, w32 in zip(("dx", "dw", "db"), got, want, want32):
        stressed("grad", f"linear_bwd |u|<=100 {name}", g.cpu(), wnt, w32, UNIT["grad"])


# ---- empty batches ------------------------------------------------------------------------------------------------------------
def test_empty_batch_forward_and_backward():
    """B = 0 through tmdiff_amd.autograd: empty outputs and input gradients, zero parameter gradients of the right shapes."""
    from tmdiff_amd import autograd as A
    c0, n, h, wd = 5, 3, 4, 6
    leaf = lambda t: cu(t).requires_grad_(True)
    for form in ("x", "pm"):
        w, bias = leaf(randn(280, c0, 1, 1, 1, 1)), leaf(randn(281, c0))
        ins = {k: leaf(v) for k, v in stem_inputs(form, 0, n, h, wd).items()}
        y = A.stem(w, bias, **ins)
        assert y.shape == (0, c0, n, h, wd)
        y.sum().backward()
        assert w.grad.shape == w.shape and bias.grad.shape == bias.shape
        assert not bool(w.grad.any()) and not bool(bias.grad.any())
        for k, t in ins.items():
            assert t.grad is not None and t.grad.shape == t.shape, k
    x, w, s = leaf(randn(282, 0, c0, n, h, wd)), leaf(randn(283, 1, c0, 1, 1, 1)), leaf(randn(284, 0, c0))
    y = A.head(x, w, s)
    assert y.shape == (0, n, h, wd)
    y.sum().backward()
    assert x.grad.shape == x.shape and s.grad.shape == s.shape and w.grad.shape == w.shape and not bool(w.grad.any())
    for act in (False, True):
        x, w, bias = leaf(randn(285, 0, 100)), leaf(randn(286, 7, 100)), leaf(randn(287, 7))
        y = A.linear(x, w, bias, act=act)
        assert y.shape == (0, 7)
        y.sum().backward()
        assert x.grad.shape == (0, 100) and w.grad.shape == (7, 100) and bias.grad.shape == (7,)
        assert not bool(w.grad.any()) and not bool(bias.grad.any())
