"""tmdiff_conv3d_wgrad_bf16 (csrc/wgrad_bf16.hip; ops.conv3d_wgrad_bf16): the 3x3x3 weight gradient from bf16-rounded g and x'
with fp32 sums, against fp64 -- of the rounded operands (only the summation order is left: a derived bound) and of the unrounded
ones (plus the rounding of two operands) --, the bias gradient from the unrounded g, determinism, and the shapes it declines."""
import collections
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from oracle.make_golden import randn

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
F64 = torch.float64
DROP = (1234, 0.2)

Case = collections.namedtuple("Case", "name b segc cout groups shp pro")
CASES = (
    Case("a-one-tile", 1, (8,), 32, 1, (4, 4, 8), False),              # one tile, one K slice per row
    Case("b-odd-bands-w12", 2, (8,), 32, 1, (5, 6, 12), False),        # odd band count; W % 8 != 0: half-masked K slices
    Case("c-groups3", 2, (24,), 96, 3, (4, 8, 8), False),
    Case("d-prologue-drop", 2, (8, 8, 16), 64, 1, (4, 8, 8), True),    # segments, SiLU + shift + scale + dropout, strided rows
    Case("e-splits", 3, (32,), 64, 1, (8, 16, 16), False),             # several split partials and the reduction
    Case("f-ragged-ci", 1, (40,), 32, 1, (4, 8, 8), False),            # Cin/groups % 32 != 0: a ragged N tile
)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from tmdiff_amd import ops as _ops
    return _ops


def cu(t):
    return t.cuda().contiguous()


def worst_ratio(err, bound):
    """max of err / bound; where the bound is 0 (all terms zero) the error must be 0 as well (tests/test_gpu_backward_edges.py)"""
    err, bound = err.double(), bound.double()
    assert bool((err[bound == 0] == 0).all()), "an error where every term is zero"
    live = bound > 0
    return float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0


def dw64(xp, g, cout, cin_g, groups):
    w = torch.zeros(cout, cin_g, 3, 3, 3, dtype=F64, requires_grad=True)
    with torch.enable_grad():
        F.conv3d(xp, w, padding=1, groups=groups).backward(g)
    return w.grad


def rne(t):
    return t.float().to(torch.bfloat16).double()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_wgrad_bf16_vs_fp64(ops, case):
    """1. exact model: x' (the library's own prologue output where there is a prologue / several segments, so both sides round the
    same fp32 numbers) and g rounded to bf16 on the host, dw in fp64 from them; bf16 products are exact in fp32, so only the
    order of the fp32 additions is left: |err| <= depth * 2^-24 * A per element, A the fp64 sum of |g_r x_r|, depth bounded by
    the number of terms K = B*N*H*W.  A dropped or misplaced term costs about A / K ~ 1e-3 A and more, the bound is at most
    K * 2^-24 = 3.7e-4 (case e) and below 4e-5 elsewhere.
    2. against fp64 of the unrounded operands: + (2^-8 + 2^-16) * A_unrounded (a relative error of at most 2^-9 per operand).
    3. dbias against fp64 of the unrounded g within K * 2^-24 * bias_scale * sum|g|.   4. two calls give the same bits.
    Measured worst ratios (MI355X): see profiles/train_bf16_grad.txt."""
    from tmdiff_amd import _lib, autograd as A_
    b, segc, cout, groups, shp = case.b, case.segc, case.cout, case.groups, case.shp
    cin, plane = sum(segc), math.prod(shp)
    K = b * plane
    xs = [randn(300 + i, b, c, *shp) for i, c in enumerate(segc)]
    g = randn(310, b, cout, *shp)
    xd, gd = [cu(x) for x in xs], cu(g)
    kw, keep = {}, []
    if case.pro:       # shift / scale rows are column blocks of wider banks: pointer + row stride, as autograd._rows hands them out
        sh_bank, sc_bank = cu(0.3 * randn(311, b, cin + 24)), cu(1 + 0.3 * randn(312, b, 2 * cin))
        sh, sc = sh_bank[:, 8:8 + cin], sc_bank[:, cin:]
        assert not sh.is_contiguous() and not sc.is_contiguous()
        keep = [sh_bank, sc_bank]
        kw = dict(in_act=True, drop=DROP, **A_._rows(sh, "shift"), **A_._rows(sc, "scale"))
    desc = ops.make_conv_desc(xd, 0, cout, 3, gd, groups=groups, bias_scale=2.0, **kw)
    wshape = (cout, cin // groups, 3, 3, 3)
    assert ops.wgrad_bf16_supported(desc)
    slots = _lib.lib.tmdiff_conv3d_wgrad_bf16_slots(C.byref(desc))
    if case.name.startswith("e"):
        assert slots >= 8, slots
    keep_counts = ops.COUNTS
    try:
        ops.COUNTS = collections.Counter()
        dw = ops.conv3d_wgrad_bf16(desc, gd, wshape)
        again = ops.conv3d_wgrad_bf16(desc, gd, wshape)
        dw_b, db = ops.conv3d_wgrad_bf16(desc, gd, wshape, want_bias=True)
        assert ops.COUNTS["conv3d_wgrad_bf16"] == 3 and ops.COUNTS["conv3d_wgrad"] == 0, dict(ops.COUNTS)
    finally:
        ops.COUNTS = keep_counts
    assert torch.equal(dw, again), "two calls differ in bits"
    assert torch.equal(dw, dw_b), "dw changes with the bias gradient on the side"
    for t, src in zip(xd + [gd], xs + [g]):
        assert torch.equal(t.cpu(), src), "an input was written"
    needs_xp = bool(case.pro) or len(segc) > 1
    xp = ops.conv3d_prologue(xd, **kw).cpu() if needs_xp else xs[0]
    if case.pro:
        dropped = float((xp == 0).double().mean())
        assert 0.1 < dropped < 0.3, dropped
    got = dw.cpu().double()
    cin_g = cin // groups
    # 1. the exact model
    xr, gr = rne(xp), rne(g)
    ref_r = dw64(xr, gr, cout, cin_g, groups)
    A_r = dw64(xr.abs(), gr.abs(), cout, cin_g, groups)
    depth = K
    ratio = worst_ratio((got - ref_r).abs(), depth * U24 * A_r)
    # 2. the unrounded operands
    x64, g64 = xp.double(), g.double()
    ref = dw64(x64, g64, cout, cin_g, groups)
    A = dw64(x64.abs(), g64.abs(), cout, cin_g, groups)
    ratio_u = worst_ratio((got - ref).abs(), (2.0 ** -8 + 2.0 ** -16) * A + depth * U24 * A_r)
    # 3. the bias gradient
    sg = g64.abs().sum((0, 2, 3, 4))
    ratio_b = worst_ratio((db.cpu().double() - 2.0 * g64.sum((0, 2, 3, 4))).abs(), K * U24 * 2.0 * sg)
    print(f"\nwgrad_bf16 {case.name}: K={K} slots={slots}: worst |err| / bound exact model {ratio:.3e}, unrounded {ratio_u:.3e}, "
          f"dbias {ratio_b:.3e}")
    assert ratio <= 1.0, f"exact model: {ratio:.3e} of the bound {depth} * 2^-24 * A"
    assert ratio_u <= 1.0, f"unrounded: {ratio_u:.3e} of the bound (2^-8 + 2^-16) * A + {depth} * 2^-24 * A_r"
    assert ratio_b <= 1.0, f"dbias: {ratio_b:.3e} of the bound {K} * 2^-24 * bias_scale * sum|g|"
    assert float((got - ref).abs().max()) > 0.0, "bf16 rounding must actually change the result"
    del keep


@pytest.mark.parametrize("what,ksize,cin,cout,groups", [
    ("ksize 1", 1, 32, 32, 1), ("Cin/groups 4", 3, 4, 32, 1), ("Cout/groups 16", 3, 8, 16, 1), ("groups 2", 3, 16, 64, 2)])
def test_wgrad_bf16_declines(ops, what, ksize, cin, cout, groups):
    """_supported() is 0 and the entry point returns TMDIFF_E_UNSUPPORTED without a launch: dw keeps its contents."""
    from tmdiff_amd import _lib
    x, g = cu(randn(320, 1, cin, 4, 4, 8)), cu(randn(321, 1, cout, 4, 4, 8))
    desc = ops.make_conv_desc([x], 0, cout, ksize, g, groups=groups)
    assert not ops.wgrad_bf16_supported(desc)
    assert _lib.lib.tmdiff_conv3d_wgrad_bf16_workspace_bytes(C.byref(desc)) == 0
    dw = torch.full((cout, cin // groups, ksize, ksize, ksize), 7.0, device="cuda")
    ws = torch.zeros(1 << 20, device="cuda")
    rc = _lib.lib.tmdiff_conv3d_wgrad_bf16(C.byref(desc), g.data_ptr(), dw.data_ptr(), None, ws.data_ptr(), ops.stream_ptr())
    assert rc == -2, (what, rc)          # TMDIFF_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((dw == 7.0).all()) and bool((ws == 0).all()), "something was launched"
    with pytest.raises(_lib.TmdiffError):
        ops.conv3d_wgrad_bf16(desc, g, tuple(dw.shape))
