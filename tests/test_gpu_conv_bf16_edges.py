"""tmdiff_conv3d_fwd_bf16 (csrc/conv3d_bf16.hip) at its edges: every launch configuration of its dispatch for the fused, the
packed-input and the producer-packed route, one to eight bands (dead waves, a second workgroup with one live band), ragged and
single rows and columns, the W >= 16 boundary, one to eight input chunks, segment and group borders, both epilogues (dwordx4
through LDS; scalar for W % 4 != 0 or a y / residual 4 bytes off a 16-byte boundary), the packed second output with and without
y, the three 1x1x1 tiles at a full plane and one position more (conv_bf16_refs.CASES; test_conv_bf16_refs_host.py asserts what
each case reaches), guard bands around every output, and what the entry point refuses.  Every launch goes through
ops.make_conv_desc; ops.conv3d runs every case once more and ops.COUNTS shows that the bf16 entry point served it.  The
library's tmdiff_conv3d_bf16_workspace_bytes must equal the restated B * Cin * N * H * W * 2.

Exact tier.  On lattice inputs (x, w integers in [-4, 4], integer shifts, bias and residual, scales of 0.5 / 1 / 2, no activation)
every operand is a bf16 number and no fp32 operation of the kernel rounds (conv_bf16_refs.exactness_ok, proved on the host), so
y must EQUAL the fp64 reference and the second output's units the host-rounded ones, bit for bit and on every route: one lost,
doubled or misplaced product is an error of at least 1/2.

Rounding tier.  On real-valued data  |y - ref| <= (K + E) * 2^-24 * A + F  elementwise.  ref = the fp64 convolution of bf16(x')
and bf16(w) with the fp64 epilogue, x' taken from the device (ops.conv3d_prologue) and rounded on the host, so that both sides
multiply the same numbers; A = the same convolution and epilogue of absolute values.
  K = taps * cin_g: the products of bf16 numbers are exact in fp32; one accumulator of v_mfma_f32_32x32x16_bf16 takes K of them
      (plus the zero products of tap slot 27), one rounding per addition at the most -- the model test_gpu_dgrad_bf16.py holds the
      same instruction to.
  E, read from store_tile, store_tile_v and the 1x1x1 epilogue, which all evaluate  (acc + bias * bias_scale + res) * out_scale
      in this order:  1 for the product bias * bias_scale (bias_v / bs[r]), 1 for acc + bias, 1 for the residual (t += q; in
      store_tile the sum acc + bias + res associates the same way), 1 for the product with out_scale unless that is 1.  So
      E = 2 [bias] + [residual] + [out_scale != 1] <= 4 (conv_bf16_refs.epilogue_roundings); every partial result a rounding acts
      on is bounded by A / |out_scale|.
  F: the two prologues are NOT the same function where there is an activation.  Without SiLU both evaluate
      fl(fl(x + shift) * scale) and F = 0.  With SiLU the prologue pass (backward.hip, silu_f) divides, v / (1 + __expf(-v)), and
      this file's kernels (silu_bf) multiply by v_rcp_f32.  Both form the same d = fl(1 + __expf(-v)).  The pass gives
      (v / d)(1 + e1), |e1| <= 2^-24 (correctly rounded division); the kernels (v / d)(1 + e2)(1 + e3), |e2| <= 2^-23 (v_rcp_f32: 1
      ulp), |e3| <= 2^-24; each is then multiplied by the scale, one more 2^-24 either side.  delta = 2^-24 + 2^-23 + 2^-24 +
      2 * 2^-24 = 3 * 2^-23, at most 6 fp32 ulps of x'.  Only an operand whose fp32 x' lies that close to a bf16 rounding tie can
      round differently in the kernel than on the host (conv_bf16_refs.flip_flags takes 8 ulps), and F = |out_scale| * sum 2^-8
      |w_r| |x'| over those operands alone.  (A flipped operand moves by one bf16 ulp, 2^-8 to 2^-7 of |x'|; F takes the lower end
      and the rounding part has to cover the rest: the printed ratios say what is left.)
E, delta and F are derived, not tuned.  Fused and packed-input results must agree bit for bit on every case, so what holds for
one route holds for the other.
Second output: the dequantised units lie within 2^-8 |t| of t = act2(y_dev + shift2) * scale2 evaluated in fp64 on the device's
own y, plus the fp32 roundings of that chain (conv_bf16_refs.second_tolerance), SiLU included.

Worst |err| / bound observed on the MI355X (profiles/conv_bf16_edges.txt; fused and packed-input routes agree bit for bit, one
figure for both; y2 = the second output against its tolerance; flips = operands within 8 ulps of a tie):
    case                     inputs     K E flips  y          y2
    A-n5-w10-ragged          normal   432 4     0  2.773e-03  -
    A-cin64-16x16            normal  1728 4    34  1.010e-03  9.954e-01
    B-w20-n5-segments        normal   864 4     0  1.879e-03  -
    C-w9-two-segments        normal   432 2     0  2.673e-03  -
    C-w10-emit-act-scalar    normal   432 4     1  1.961e-03  9.874e-01
    A-w8-emit-aligned        normal   432 4     0  4.677e-03  9.959e-01
    k1-128-exact             normal    16 0     0  7.109e-02  -
    k1-128-plus1             normal    32 4     0  4.733e-02  -
    k1-64-plus1-3seg         normal    48 3     6  2.768e-02  -
    k1-32-plus1-segments     normal    32 0     0  4.415e-02  -
    A-cin64-16x16            sensor  1728 4    27  1.321e-03  9.952e-01
    B-w20-n5-segments        sensor   864 4     0  1.805e-03  -
    k1-64-plus1-3seg         sensor    48 3     6  4.203e-02  -
The certain bound of y is 14 to 1000 times what the kernels do on these data: its job is precision (an operand rounded twice, a
partial sum kept in bf16), the exact tier's job is every lost or misplaced term.  The second output sits at its tolerance
because the tolerance IS the rounding to bf16: half a bf16 ulp is 2^-8 |t| at the bottom of a binade, and among some 1e5
values one lies there; units two bf16 numbers off miss it at every element (test_conv_bf16_refs_host.py).
"""
import collections
import ctypes as C
import functools

import pytest
import torch

import conv_bf16_refs as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 64                   # elements of guard band either side of an output (256 bytes of fp32, 128 bytes of units)
NAN_UNIT = 0x7FC0            # a bf16 NaN
IDS = [c.name for c in R.CASES]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from tmdiff_amd import ops as _ops
    return _ops


def cu(t):
    return None if t is None else t.cuda().contiguous()


def worst_ratio(err, bound):
    """max of err / bound; where the bound is 0 (all terms zero) the error must be 0 as well"""
    err, bound = err.double(), bound.double()
    assert bool((err[bound == 0] == 0).all()), "an error where every term is zero"
    live = bound > 0
    return float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0


def _shifted(t):
    """A copy of t that starts 4 bytes off a 16-byte boundary (the idiom of test_gpu_cs.py)."""
    pad = torch.zeros(t.numel() + 1, device="cuda")
    view = pad[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


class Guarded:
    """A NaN-filled view of `shape` inside a larger NaN-filled allocation this test owns: GUARD elements either side and, for a
    misaligned view, the 4 bytes in front."""

    def __init__(self, shape, dtype=torch.float32, misalign=False):
        n = 1
        for s in shape:
            n *= s
        self.n, self.off = n, GUARD + (1 if misalign else 0)
        if dtype == torch.float32:
            self.buf = torch.full((n + 2 * GUARD + 4,), NAN, device="cuda", dtype=dtype)
        else:
            self.buf = torch.full((n + 2 * GUARD + 4,), NAN_UNIT, device="cuda", dtype=dtype)
        self.view = self.buf[self.off:self.off + n].view(shape)
        self.bits = torch.int32 if dtype == torch.float32 else torch.int16
        assert self.view.is_contiguous() and self.view.data_ptr() % 16 == (4 if misalign else 0)
        self.before = self.buf.view(self.bits).clone()

    def check(self, what, written=True):
        now = self.buf.view(self.bits)
        lo, hi = self.off, self.off + self.n
        assert torch.equal(now[:lo], self.before[:lo]) and torch.equal(now[hi:], self.before[hi:]), f"{what}: guard band written"
        if self.bits == torch.int32:
            nans = torch.isnan(self.view)
        else:
            nans = (self.view.to(torch.int32) & 0x7FFF) > 0x7F80
        if written:
            assert not bool(nans.any()), f"{what}: {int(nans.sum())} elements not written"
        else:
            assert bool(nans.all()), f"{what}: written to by a refused call"


def routes_of(case):
    if case.k == 1:
        return ("k1",)
    return ("fused", "packed") + (("producer",) if R.producer_route(case) else ())


def emit_kw(inp, case):
    if not case.emit:
        return {}
    return dict(y2_act=inp["emit_act"], y2_shift=cu(inp["emit_shift"]), y2_scale=cu(inp["emit_scale"]))


def prologue_kw(inp):
    kw = dict(in_shift=cu(inp["shift"]), in_scale=cu(inp["scale"]), in_act=bool(inp["act"]))
    return {k: v for k, v in kw.items() if v is not None and v is not False}


def run(ops, case, inp, route, keep_y=True):
    """One launch of tmdiff_conv3d_fwd_bf16 on a descriptor from ops.make_conv_desc, outputs inside guard bands: route "fused" (no
    workspace), "packed" (the pack pass's workspace), "producer" (the input as bf16 units built on the host), "k1".  The
    library's workspace size is the restated one.  (y fp32 or None, y2 units or None) on the CPU."""
    cfg = R.config_of(case)
    shape = (case.B, case.cout, case.N, case.H, case.W)
    plane = case.N * case.H * case.W
    what = f"{case.name} / {route}"
    wp = ops.pack_conv_weight_bf16(cu(inp["w"]), groups=case.groups)
    kw = dict(groups=case.groups, bias=cu(inp["bias"]), bias_scale=inp["bias_scale"], out_scale=inp["out_scale"], **emit_kw(inp, case))
    if route == "producer":
        assert not prologue_kw(inp)
        segs = [R.pack_units(inp["xs"][0]).cuda()]
        kw["x_bf16_shape"] = (case.N, case.H, case.W)
    else:
        segs = [cu(x) for x in inp["xs"]]
        kw.update(prologue_kw(inp))
    res = cu(inp["res"])
    if res is not None and case.misalign:
        res = _shifted(res)
    gy = Guarded(shape, misalign=case.misalign) if keep_y else None
    g2 = Guarded((case.B, case.cout // 8, plane, 8), torch.int16) if case.emit else None
    d = ops.make_conv_desc(segs, wp, case.cout, case.k, gy.view if gy else None, residual=res, y2=g2.view if g2 else None, **kw)
    assert ops.lib.tmdiff_conv3d_bf16_workspace_bytes(C.byref(d)) == cfg.workspace_bytes, what
    ws = torch.empty(cfg.workspace_bytes, device="cuda", dtype=torch.uint8) if route == "packed" else None
    ops.check(ops.lib.tmdiff_conv3d_fwd_bf16(C.byref(d), ws.data_ptr() if ws is not None else None, ops.stream_ptr()), what)
    torch.cuda.synchronize()
    for g, nm in ((gy, "y"), (g2, "y2")):
        if g is not None:
            g.check(f"{what}: {nm}")
    return (gy.view.cpu() if gy else None), (g2.view.cpu() if g2 else None)


@functools.lru_cache(maxsize=None)
def lattice(name):
    """(inputs, y fp64, units of the second output or None) of a case's lattice inputs: computed once, shared, left unchanged"""
    case = R.CASE[name]
    inp = R.lattice_inputs(case)
    ref = R.reference(case, inp)
    assert torch.equal(ref["y"].float().double(), ref["y"])
    units = None
    if case.emit:
        assert torch.equal(ref["t2"].float().double(), ref["t2"])
        units = R.pack_units(ref["t2"].float())
    return inp, ref["y"].float(), units


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_exact_on_the_lattice_with_guard_bands(ops, case):
    inp, want, units = lattice(case.name)
    for route in routes_of(case):
        y, y2 = run(ops, case, inp, route, keep_y=case.keep_y)
        what = f"{case.name} / {route}"
        if case.keep_y:
            assert torch.equal(y, want), f"{what}: {int((y != want).sum())} of {y.numel()} differ, first at " \
                                         f"{(y != want).nonzero()[0].tolist()}, worst {float((y - want).abs().max())}"
        if case.emit:
            assert torch.equal(y2, units), f"{what}: {int((y2 != units).sum())} second-output values of {y2.numel()} differ, first " \
                                           f"at {(y2 != units).nonzero()[0].tolist()}"
        if not case.keep_y:                        # the same units with y written as well
            y_k, y2_k = run(ops, case, inp, route, keep_y=True)
            assert torch.equal(y_k, want) and torch.equal(y2_k, y2), what


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_ops_conv3d_takes_the_bf16_entry_point(ops, case):
    """ops.conv3d(math="bf16") with its own choice of route and its own outputs: the same bits, one launch of the bf16 entry point"""
    inp, want, units = lattice(case.name)
    wp = ops.pack_conv_weight_bf16(cu(inp["w"]), groups=case.groups)
    res = cu(inp["res"])
    out = None
    if case.misalign:
        res, out = _shifted(res), _shifted(torch.full(want.shape, NAN))
    emit = None if not case.emit else dict(act=False, shift=cu(inp["emit_shift"]), scale=cu(inp["emit_scale"]))
    keep, ops.COUNTS = ops.COUNTS, collections.Counter()
    try:
        got = ops.conv3d([cu(x) for x in inp["xs"]], wp, case.cout, case.k, out=out, math="bf16", emit=emit, keep_y=case.keep_y,
                         groups=case.groups, bias=cu(inp["bias"]), bias_scale=inp["bias_scale"], residual=res,
                         out_scale=inp["out_scale"], **prologue_kw(inp))
        counts = dict(ops.COUNTS)
    finally:
        ops.COUNTS = keep
    assert counts == {"conv3d_fwd_bf16" if case.k == 3 else "conv3d_fwd_bf16_k1": 1}, counts
    y, y2 = (got if case.keep_y else (None, got)) if case.emit else (got, None)
    if case.keep_y:
        assert torch.equal(y.cpu(), want)
    if case.emit:
        assert y2.dtype == torch.int16 and torch.equal(y2.cpu(), units)


@functools.lru_cache(maxsize=None)
def real(name):
    return R.real_inputs(R.CASE[name])


@pytest.mark.parametrize("name,which", [(n, "normal") for n in R.ROUNDING_CASES] + [(n, "sensor") for n in R.SENSOR_CASES])
def test_rounding_bound_elementwise(ops, name, which):
    case = R.CASE[name]
    inp = real(name)[which]
    pkw = prologue_kw(inp)
    xs = [cu(x) for x in inp["xs"]]
    xp32 = (ops.conv3d_prologue(xs, **pkw) if pkw else torch.cat(xs, 1)).cpu()
    xq, wq = R.bf16_rne(xp32).double(), R.bf16_rne(inp["w"]).double()
    ref = R.reference(case, inp, xq, wq)["y"]
    bnd = R.bound(case, xq, wq, inp, xp32 if inp["act"] else None)
    flips = int(R.flip_flags(xp32).sum()) if inp["act"] else 0
    routes = routes_of(case)[:2]
    y, y2 = run(ops, case, inp, routes[0])
    for other in routes[1:]:
        y_o, y2_o = run(ops, case, inp, other)
        assert torch.equal(y, y_o), f"{name}: fused and packed-input variants must agree bit for bit"
        assert y2 is None or torch.equal(y2, y2_o), f"{name}: second outputs of the fused and packed-input variants differ"
    ratio = worst_ratio((y.double() - ref).abs(), bnd)
    line = f"edges {name:24s} {which:6s} K={R.taps_of(case) * (R.cin_of(case) // case.groups):5d} E={R.epilogue_roundings(inp)} " \
           f"flips={flips:4d}  y {ratio:.3e}"
    ratio2 = 0.0
    if case.emit:
        got = R.unpack_units(y2, y.shape).double()
        ratio2 = worst_ratio((got - R.second64(y, inp)).abs(), R.second_tolerance(y, inp))
        line += f"  y2 {ratio2:.3e}"
    print(line)
    assert ratio <= 1.0, line
    assert ratio2 <= 1.0, line


@pytest.mark.parametrize("name", R.REPEAT_CASES)
def test_two_calls_give_the_same_bits(ops, name):
    case = R.CASE[name]
    inp = real(name)["normal"]
    for route in routes_of(case)[:2]:
        a, b = run(ops, case, inp, route), run(ops, case, inp, route)
        assert torch.equal(a[0], b[0]) and (a[1] is None or torch.equal(a[1], b[1])), f"{name} / {route}"


def _refused(ops, status, segs, wp, cout, k, shape, **kw):
    """ops.conv3d(math="bf16") raises TmdiffError with `status` (-1 = TMDIFF_E_INVALID, -2 = TMDIFF_E_UNSUPPORTED) for both
    pack_input choices, and a NaN-filled out stays NaN"""
    from tmdiff_amd._lib import TmdiffError
    for pack_input in (False, True):
        g = Guarded(shape)
        with pytest.raises(TmdiffError, match=f"status {status}:"):
            ops.conv3d(segs, wp, cout, k, out=g.view, math="bf16", pack_input=pack_input, **kw)
        torch.cuda.synchronize()
        g.check(f"refusal {kw.keys()}", written=False)


def test_refusals_write_nothing(ops):
    from tmdiff_amd._lib import TmdiffError
    x16 = cu(torch.randn(1, 16, 4, 8, 8))
    w3 = ops.pack_conv_weight_bf16(cu(torch.randn(32, 16, 3, 3, 3)))
    w1 = ops.pack_conv_weight_bf16(cu(torch.randn(32, 16, 1, 1, 1)))
    any_w = torch.zeros(1 << 16, device="cuda", dtype=torch.int16)        # for shapes that have no packing at all
    shape = (1, 32, 4, 8, 8)
    # W % 4 == 0 with a second output that is not 16-byte aligned (straight on the descriptor: ops.conv3d allocates y2 itself)
    gy = Guarded(shape)
    flat = torch.full((32 // 8 * 256 * 8 + 8,), NAN_UNIT, device="cuda", dtype=torch.int16)
    y2 = flat[2:-6].view(1, 4, 256, 8)
    assert y2.data_ptr() % 16 == 4
    d = ops.make_conv_desc([x16], w3, 32, 3, gy.view, y2=y2)
    for ws in (None, torch.empty(ops.lib.tmdiff_conv3d_bf16_workspace_bytes(C.byref(d)), device="cuda", dtype=torch.uint8)):
        with pytest.raises(TmdiffError, match="status -1:"):
            ops.check(ops.lib.tmdiff_conv3d_fwd_bf16(C.byref(d), ws.data_ptr() if ws is not None else None, ops.stream_ptr()), "y2")
        torch.cuda.synchronize()
        gy.check("misaligned y2", written=False)
        assert bool((flat == NAN_UNIT).all())
    # a second output of a 1x1x1 convolution
    _refused(ops, -2, [x16], w1, 32, 1, shape, emit={})
    # a bf16-packed input together with a prologue, and for a 1x1x1 convolution
    xu = R.pack_units(torch.randn(1, 16, 4, 8, 8)).cuda()
    _refused(ops, -1, [xu], w3, 32, 3, shape, x_bf16_shape=(4, 8, 8), in_shift=cu(torch.zeros(1, 16)))
    _refused(ops, -1, [xu], w3, 32, 3, shape, x_bf16_shape=(4, 8, 8), in_act=True)
    _refused(ops, -1, [xu], w1, 32, 1, shape, x_bf16_shape=(4, 8, 8))
    # channel counts: cin_g = 12 (3x3x3), cin_g = 8 (1x1x1), cout_g = 16, segments that are no multiples of 8
    _refused(ops, -2, [cu(torch.randn(1, 12, 4, 8, 8))], any_w, 32, 3, shape)
    _refused(ops, -2, [cu(torch.randn(1, 8, 4, 8, 8))], any_w, 32, 1, shape)
    _refused(ops, -2, [x16], any_w, 16, 3, (1, 16, 4, 8, 8))
    _refused(ops, -2, [cu(torch.randn(1, 4, 4, 8, 8)), cu(torch.randn(1, 12, 4, 8, 8))], w3, 32, 3, shape)
    # a mask, dropout
    _refused(ops, -2, [x16], w3, 32, 3, shape, in_mask=torch.ones_like(x16))
    _refused(ops, -2, [x16], w3, 32, 3, shape, drop=(1234, 0.1))
    # groups = 2 on one tensor: every forward entry point takes groups 1 or 3 (include/tmdiff_hip.h; test_host_logic.py holds the
    # bf16 one to TMDIFF_E_INVALID for it), so the case is a refusal here
    _refused(ops, -1, [x16], w3, 64, 3, (1, 64, 4, 8, 8), groups=2)
