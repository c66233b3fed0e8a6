"""The two backward kernels of the finetune path that no test compared with an independent reference on the shapes where they
alone run (csrc/backward.hip): the direct weight gradient conv3d_wgrad_kernel<3> / <1> with the prologue pass in front of it
(prologue_apply_kernel, also ops.conv3d_prologue on its own), the prologue backward prologue_bwd_kernel + rowsum_kernel, and
channel_sum_kernel at more than one slice.

The reference throughout is the operator restated in fp64 on the CPU.  Elementwise results (x', dL/dx) are held to the tolerance
the suite already holds SiLU outputs of this very prologue pass to (test_gpu_kernels.py, "side prologue vs torch": 2e-6 of the
largest value, 1e-6 in the L2 norm).  Every SUM (dw, dbias, d_shift, d_scale, channel sums) is held to a bound built from the fp64
sum of the absolute terms and a count read from the kernel:

    |got - ref| <= D * 2^-24 * sum |terms|        (D: the number of terms, or the longest chain of dependent additions)

which is the certain bound of fp32 accumulation; one lost or misplaced term costs about sum|terms| / (number of terms), 15 to
500 times more at the sizes used here.  The bounds are derived, not tuned: every line that starts with "edges" prints the worst
|err| / bound of a case.
"""
import collections
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close, rel_err
from oracle.make_golden import randn

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
ELEM_MAX, ELEM_L2 = 2e-6, 1e-6        # x' against fp64: max error / largest value, relative L2 (test_gpu_kernels.py)
ELEM_C = ELEM_MAX / U24               # the elementwise tolerance in units of 2^-24: 33.6
F64, F32 = torch.float64, torch.float32
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from tmdiff_amd import ops as _ops
    return _ops


def cu(t):
    return None if t is None else t.cuda().contiguous()


def cdiv(a, b):
    return -(-a // b)


def rand_mask(seed, *shape):
    """a host-drawn dropout mask: 0 or 1 / 0.8"""
    return (torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) > 0.2).float() / 0.8


def silu64(u):
    return u * torch.sigmoid(u)


def per_plane(rows, b):
    """[B, Cin] or [Cin] -> [B, Cin, 1, 1, 1] in fp64"""
    rows = rows.double()
    return (rows[None].expand(b, -1) if rows.dim() == 1 else rows)[:, :, None, None, None]


def prologue64(xs, shift, scale, mask, act):
    """x' = act(cat(x) + shift) * scale * mask in fp64 from fp32 CPU tensors (shift / scale: [B, Cin], [Cin] or None)"""
    u = torch.cat(xs, 1).double()
    b = u.shape[0]
    if shift is not None:
        u = u + per_plane(shift, b)
    u = silu64(u) if act else u
    if scale is not None:
        u = u * per_plane(scale, b)
    return u if mask is None else u * mask.double()


def stride_kw(shift, scale):
    """make_conv_desc's stride arguments: a [Cin] row is a bank of one row broadcast over the batch (stride < 0 -> 0)"""
    return dict(shift_stride=-1 if shift is not None and shift.dim() == 1 else 0,
                scale_stride=-1 if scale is not None and scale.dim() == 1 else 0)


def worst_ratio(err, bound):
    """max of err / bound; where the bound is 0 (all terms zero) the error must be 0 as well"""
    err, bound = err.double(), bound.double()
    assert bool((err[bound == 0] == 0).all()), "an error where every term is zero"
    live = bound > 0
    return float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0


# ---- 1. the forward prologue on its own: ops.conv3d_prologue ------------------------------------------------------------------
FWD_SEGS = [(5,), (3, 4), (8, 16, 8)]
FWD_PLANES = [(4, 10, 7), (3, 5, 7)]          # 280 = 4 * 70: the float4 branch;  105: the scalar branch


def fwd_inputs(segc, shp, b=2):
    cin = sum(segc)
    xs = [randn(100 + i, b, c, *shp) for i, c in enumerate(segc)]
    return xs, 0.3 * randn(110, b, cin), 1 + 0.3 * randn(111, b, cin), rand_mask(112, b, cin, *shp)


def fwd_variants():
    """(shift?, scale?, mask?, act?, rows as [Cin]?) -- every combination; the row form matters only where there is a row"""
    for has_sh in (False, True):
        for has_sc in (False, True):
            for has_m in (False, True):
                for act in (False, True):
                    for rows in ((False, True) if has_sh or has_sc else (False,)):
                        yield has_sh, has_sc, has_m, act, rows


def check_forward(ops, xs_dev, xs, sh, sc, mask, what):
    """every variant of the prologue on the device segments xs_dev (CPU values xs); returns the worst max-rel error"""
    worst = 0.0
    for has_sh, has_sc, has_m, act, rows in fwd_variants():
        shv = (sh[0] if rows else sh) if has_sh else None
        scv = (sc[0] if rows else sc) if has_sc else None
        mv = mask if has_m else None
        got = ops.conv3d_prologue(xs_dev, in_shift=cu(shv), in_scale=cu(scv), in_mask=cu(mv), in_act=act, **stride_kw(shv, scv)).cpu()
        want = prologue64(xs, shv, scv, mv, act)
        case = f"{what} shift={has_sh} scale={has_sc} mask={has_m} act={act} rows={'[Cin]' if rows else '[B,Cin]'}"
        assert_close(got, want, ELEM_MAX, ELEM_L2, case)
        worst = max(worst, rel_err(got, want)[0])
        if not act and not has_sh:        # no transcendental, no addition: the fp32 products, bit for bit
            exact = torch.cat(xs, 1)
            if has_sc:
                exact = exact * per_plane(scv, exact.shape[0]).float()
            if has_m:
                exact = exact * mv
            assert torch.equal(got, exact), f"{case}: not the fp32 products"
    return worst


@pytest.mark.parametrize("shp", FWD_PLANES, ids=["plane280-float4", "plane105-scalar"])
@pytest.mark.parametrize("segc", FWD_SEGS, ids=["1seg", "2seg", "3seg"])
def test_forward_prologue_vs_fp64(ops, segc, shp):
    """x' = act(cat(x) + shift) * scale * mask for one, two and three segments on both branches of prologue_apply_kernel, with
    and without each of shift, scale, mask and act, shift / scale as [B, Cin] and as one [Cin] row: against fp64 at the SiLU
    tolerance; without act and shift the result is x * scale * mask evaluated in fp32 on the CPU, exactly."""
    xs, sh, sc, mask = fwd_inputs(segc, shp)
    worst = check_forward(ops, [cu(x) for x in xs], xs, sh, sc, mask, f"prologue {segc} {shp}")
    print(f"\nedges prologue_fwd segs={segc} plane={math.prod(shp)}: worst max-rel {worst:.3e} (<= {ELEM_MAX:g})")


def off_by_one_float(t):
    """t's values in a window one float into a larger buffer: contiguous, 4 bytes off a 16-byte boundary"""
    buf = torch.full((t.numel() + 8,), NAN, device="cuda", dtype=F32)
    win = buf[1:1 + t.numel()].view(t.shape)
    win.copy_(t)
    assert win.is_contiguous() and win.data_ptr() % 16 == 4
    return win


@pytest.mark.parametrize("which", ["segment", "mask"])
def test_forward_prologue_alignment_fallback(ops, which):
    """plane % 4 == 0, but the middle segment (or the mask) starts one float off a 16-byte boundary, inside a larger buffer whose
    other floats are NaN: those planes (all planes) take the scalar branch, the others the float4 branch; same values."""
    segc, shp = (8, 16, 8), (4, 10, 7)
    xs, sh, sc, mask = fwd_inputs(segc, shp)
    xs_dev = [cu(x) for x in xs]
    if which == "segment":
        xs_dev[1] = off_by_one_float(xs_dev[1])
        worst = check_forward(ops, xs_dev, xs, sh, sc, mask, "prologue, segment 1 off by a float")
    else:
        md = off_by_one_float(cu(mask))
        got = ops.conv3d_prologue(xs_dev, in_shift=cu(sh), in_scale=cu(sc), in_mask=md, in_act=True).cpu()
        want = prologue64(xs, sh, sc, mask, True)
        assert_close(got, want, ELEM_MAX, ELEM_L2, "prologue, mask off by a float")
        worst = rel_err(got, want)[0]
    print(f"\nedges prologue_fwd unaligned {which}: worst max-rel {worst:.3e} (<= {ELEM_MAX:g})")


# ---- 2. the direct weight gradient against fp64 ------------------------------------------------------------------------------
def plan_wgrad(b, cin, cout, groups, n, h, w):
    """plan_wgrad's rule (csrc/backward.hip) restated: (boxes, boxes per split, splits).  2 x 8 x 8 boxes; the launch runs in rounds
    of 256 workgroups; the split count minimises rounds * (boxes per workgroup + 0.5), ties to the smaller count."""
    total = b * cdiv(n, 2) * cdiv(h, 8) * cdiv(w, 8)
    tiles = groups * cdiv(cout // groups, 32) * cdiv(cin // groups, 32)
    best_s, best_cost = 1, 1e30
    for s in range(1, min(total, 512) + 1):
        bps = cdiv(total, s)
        s_eff = cdiv(total, bps)
        cost = cdiv(tiles * s_eff, 256) * (bps + 0.5)
        if cost < best_cost - 1e-9:
            best_cost, best_s = cost, s_eff
    bps = cdiv(total, best_s)
    return total, bps, cdiv(total, bps)


Wg = collections.namedtuple("Wg", "name b segc cout k groups shp pro")
WGRAD_CASES = [
    Wg("one-ragged-box", 1, (4,), 4, 3, 1, (1, 3, 5), None),
    Wg("odd-N-ragged-HW-two-co-tiles", 2, (24,), 40, 3, 1, (3, 5, 10), None),
    Wg("whole-box-33-channels", 1, (33,), 33, 3, 1, (2, 8, 8), None),
    Wg("36-boxes-B3", 3, (8,), 8, 3, 1, (5, 9, 9), None),
    Wg("12-boxes-B1", 1, (8,), 8, 3, 1, (5, 9, 9), None),
    Wg("60-boxes-B5", 5, (8,), 8, 3, 1, (5, 9, 9), None),
    Wg("groups2-two-segments", 2, (16, 16), 32, 3, 2, (2, 8, 12), None),
    Wg("groups4-cin6-cout4", 1, (8, 8, 8), 16, 3, 4, (3, 6, 6), None),
    Wg("groups3-N3", 2, (12, 12, 12), 48, 3, 3, (3, 8, 10), None),
    Wg("prologue-mask", 2, (16, 8, 8), 32, 3, 1, (3, 6, 10), "mask"),
    Wg("prologue-dropout", 2, (16, 8, 8), 32, 3, 1, (3, 6, 10), "drop"),
    Wg("forced-winograd-shape", 2, (32,), 64, 3, 1, (8, 16, 16), None),
    Wg("k1", 2, (32,), 32, 1, 1, (4, 8, 16), None),
    Wg("k1-ragged", 1, (24,), 40, 1, 1, (3, 5, 10), None),
    Wg("k1-groups2", 3, (6,), 10, 1, 2, (5, 9, 9), None),
    # the only cases here whose workgroups walk more than one box (see test_direct_wgrad_vs_fp64)
    Wg("ragged-last-split", 37, (128,), 128, 3, 1, (1, 3, 5), None),
    Wg("k1-ragged-last-split", 37, (128,), 128, 1, 1, (1, 3, 5), None),
]
DROP = (987654321012, 0.2)


def dw64(xp, g, cout, cin_g, k, groups):
    w = torch.zeros(cout, cin_g, k, k, k, dtype=F64, requires_grad=True)
    with torch.enable_grad():
        F.conv3d(xp, w, padding=k // 2, groups=groups).backward(g)
    return w.grad


@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c.name for c in WGRAD_CASES])
def test_direct_wgrad_vs_fp64(ops, case):
    """conv3d_wgrad_kernel<3> / <1> + wgrad_reduce_kernel on shapes the Winograd weight gradient declines (ops.COUNTS and
    wgrad_wino_takes prove the routing): odd N (an empty second band plane in the last box), H / W no multiples of 8, channel
    counts below and across the 32 x 32 tile, one box, 2 / 3 / 4 groups, 1x1x1, several segments and the full prologue with a
    mask tensor and with in-kernel dropout in front.

    Reference: x' is taken from the device (ops.conv3d_prologue; the same seed draws the same dropout mask) where there is a
    prologue or more than one segment, so both sides multiply the same fp32 numbers and only the summation differs; dw is
    F.conv3d's weight gradient in fp64.  Bound per element: K * 2^-24 * A, K = B*N*H*W terms, A the same gradient of |x'| and
    |g|.  K <= 1024 but for the 5 x 9 x 9 shape at B = 3 (1215) and B = 5 (2025): the bound is at most 1.2e-4 A there and below
    6.2e-5 A elsewhere, while one lost term costs about A / K: >= 4.9e-4 A there, >= 1e-3 A elsewhere.

    forced-winograd-shape (K = 4096, ops.config.wgrad_wino off) uses D * 2^-24 * A with D the longest chain of dependent
    additions an element goes through: plan_wgrad gives 32 boxes over 2 tiles -> 32 splits of ONE box; a wave runs the 32 K-steps
    of its band plane, each an MFMA that adds 2 products (64 additions), the two band planes meet in LDS (+1), wgrad_reduce_kernel
    gives each of its 4 thread rows every 4th of the 32 slots (8 additions) and adds the rows as (p0 + p1) + (p2 + p3) (+2):
    D = 64 * boxes_per_split + 1 + ceil(splits / 4) + 2 = 75.

    The ragged last K-split: with the three B of the 5 x 9 x 9 shape (12, 36 and 60 boxes, one tile) plan_wgrad's rule never
    gives a workgroup more than one box -- up to 256 workgroups run in one round, so boxes_per_split = 1 costs 1.5 and nothing
    beats it; total_boxes % boxes_per_split == 0 for B = 1, 3 AND 5, and for every other shape above the last two.  A ragged
    split needs tiles * boxes > 256: the two last cases have 37 one-plane boxes under 16 tiles -> 13 splits of 3 boxes, the last
    one holding 1 (asserted below), which also runs the double-buffered box loop for 3 boxes and for 1.

    Two calls give the same bits; want_bias gives the same dw bits and dbias within K * 2^-24 * bias_scale * sum|g| of fp64."""
    from tmdiff_amd import _lib
    b, segc, cout, k, groups, shp = case.b, case.segc, case.cout, case.k, case.groups, case.shp
    cin, plane = sum(segc), math.prod(shp)
    K = b * plane
    xs = [randn(200 + i, b, c, *shp) for i, c in enumerate(segc)]
    g = randn(210, b, cout, *shp)
    kw = {}
    if case.pro:
        sh, sc = 0.3 * randn(211, b, cin), 1 + 0.3 * randn(212, b, cin)
        kw = dict(in_shift=cu(sh), in_scale=cu(sc), in_act=True)
        kw.update(dict(in_mask=cu(rand_mask(213, b, cin, *shp))) if case.pro == "mask" else dict(drop=DROP))
    xd, gd = [cu(x) for x in xs], cu(g)                   # (the descriptor holds bare pointers: the tensors outlive it)
    desc = ops.make_conv_desc(xd, 0, cout, k, gd, groups=groups, bias_scale=2.0, **kw)
    wshape = (cout, cin // groups, k, k, k)
    forced = case.name == "forced-winograd-shape"
    total, bps, splits = plan_wgrad(b, cin, cout, groups, *shp)
    # the restated plan is the library's: its workspace holds splits x (dw + dbias) partials and x'
    r4 = lambda v: (v + 3) // 4 * 4
    needs_xp = bool(case.pro) or len(segc) > 1
    assert _lib.lib.tmdiff_conv3d_wgrad_workspace_bytes(C.byref(desc)) == \
        4 * (r4(splits * cout * (cin // groups) * k ** 3) + r4(splits * cout) + (b * cin * plane if needs_xp else 0))
    if "ragged-last-split" in case.name:
        assert (total, bps, splits) == (37, 3, 13) and total % bps == 1
    else:
        assert bps == 1 and splits == total
    if forced:
        assert ops.wgrad_wino_takes(desc)
    keep_cfg, keep_counts = ops.config.wgrad_wino, ops.COUNTS
    try:
        if forced:
            ops.config.wgrad_wino = False
        assert not ops.wgrad_wino_takes(desc)
        ops.COUNTS = collections.Counter()
        dw = ops.conv3d_wgrad(desc, gd, wshape)
        assert ops.COUNTS["conv3d_wgrad"] == 1 and ops.COUNTS["conv3d_wgrad_wino"] == 0, dict(ops.COUNTS)
        again = ops.conv3d_wgrad(desc, gd, wshape)
        dw_b, db = ops.conv3d_wgrad(desc, gd, wshape, want_bias=True)
        assert ops.COUNTS["conv3d_wgrad"] == 3 and ops.COUNTS["conv3d_wgrad_wino"] == 0, dict(ops.COUNTS)
    finally:
        ops.config.wgrad_wino, ops.COUNTS = keep_cfg, keep_counts
    assert torch.equal(dw, again), "two calls differ in bits"
    assert torch.equal(dw, dw_b), "dw changes with the bias gradient on the side"
    for t, src in zip(xd + [gd], xs + [g]):
        assert torch.equal(t.cpu(), src), "an input was written"
    xp = (ops.conv3d_prologue(xd, **kw).cpu() if needs_xp else xs[0]).double()
    if case.pro == "drop":
        dropped = float((xp == 0).double().mean())
        assert 0.1 < dropped < 0.3, dropped
    g64 = g.double()
    ref = dw64(xp, g64, cout, cin // groups, k, groups)
    A = dw64(xp.abs(), g64.abs(), cout, cin // groups, k, groups)
    if forced:
        depth = 64 * bps + 1 + cdiv(splits, 4) + 2
        assert K == 4096 and depth == 75
    else:
        assert K <= (2025 if shp == (5, 9, 9) else 1024)
        depth = K
    ratio = worst_ratio((dw.cpu().double() - ref).abs(), depth * U24 * A)
    sg = g64.abs().sum((0, 2, 3, 4))
    ratio_b = worst_ratio((db.cpu().double() - 2.0 * g64.sum((0, 2, 3, 4))).abs(), K * U24 * 2.0 * sg)
    print(f"\nedges wgrad {case.name}: K={K} boxes={total} splits={splits} x {bps}, depth {depth}: worst |err| / bound dw {ratio:.3e}, "
          f"dbias {ratio_b:.3e}")
    assert ratio <= 1.0, f"dw: {ratio:.3e} of the bound {depth} * 2^-24 * A"
    assert ratio_b <= 1.0, f"dbias: {ratio_b:.3e} of the bound {K} * 2^-24 * bias_scale * sum|g|"


# ---- 3. the prologue backward against fp64 -----------------------------------------------------------------------------------
Pb = collections.namedtuple("Pb", "name b segc shp")
BWD_CASES = [
    Pb("plane280-float4-3seg", 2, (8, 16, 8), (4, 10, 7)),
    Pb("plane105-scalar", 3, (5,), (3, 5, 7)),
    Pb("plane4096-2slices", 1, (8,), (4, 32, 32)),
    Pb("plane8192-4slices", 1, (4,), (8, 32, 32)),
    Pb("plane4205-2slices-scalar", 1, (3,), (5, 29, 29)),
    Pb("plane4224-2slices-of-528", 2, (8,), (1, 64, 66)),
]
BWD_SLICES = [1, 1, 2, 4, 2, 2]
BWD_OPTIONS = ["base", "mask", "drop", "noact", "noshift", "noscale", "rows", "shift_only", "scale_only", "neither", "dx_none",
               "accumulate", "add"]
# every case plain; every option on the first case and on two sliced ones (float4 and scalar); the last case once more through
# the entry point without a workspace (one slice)
BWD_RUNS = [(i, "base") for i in range(len(BWD_CASES))] + [(i, o) for i in (0, 2, 4) for o in BWD_OPTIONS[1:]] + [(5, "no_workspace")]


def bwd_slices(b, cin, plane):
    """prologue_bwd_slices (csrc/backward.hip): workgroups per (b, c) plane -- ~1024 in all, at least 2048 elements each, <= 64"""
    return max(1, min(cdiv(1024, b * cin), plane // 2048, 64))


def bwd_depth(plane, slices):
    """Longest chain of dependent additions behind one d_shift / d_scale element, read from prologue_bwd_kernel: a slice is
    ceil(units / slices) units (float4 branch: unit = 4 elements) over 256 lanes, each lane adding its elements one by one;
    block_sum adds 6 shuffle steps and red[0] + red[1] + red[2] + red[3] (3); rowsum_kernel adds the slices one by one."""
    unit = 4 if plane % 4 == 0 else 1
    lane = unit * cdiv(cdiv(plane // unit, slices), 256)
    return lane + 6 + 3 + (slices if slices > 1 else 0)


def bwd_inputs(ci):
    c = BWD_CASES[ci]
    cin = sum(c.segc)
    xs = [randn(300 + i, c.b, n, *c.shp) for i, n in enumerate(c.segc)]
    return xs, randn(310, c.b, cin, *c.shp), 0.3 * randn(311, c.b, cin), 1 + 0.3 * randn(312, c.b, cin)


def bwd_math(ci, opt):
    """(shift, scale, act, mask kind) of an option; the options about what is asked for compute what "base" computes"""
    _, _, sh, sc = bwd_inputs(ci)
    return {"mask": (sh, sc, True, "mask"), "drop": (sh, sc, True, "drop"), "noact": (sh, sc, False, None),
            "noshift": (None, sc, True, None), "noscale": (sh, None, True, None),
            "rows": (sh[0], sc[0], True, None)}.get(opt, (sh, sc, True, None))


@functools.lru_cache(maxsize=None)
def device_keep_mask(ci):
    """the in-kernel dropout mask of DROP as the forward draws it: the prologue pass on ones with nothing else set gives
    keep / (1 - p), i.e. the mask with its factor; dividing by 1 / (1 - p) leaves zeros and ones"""
    from tmdiff_amd import ops
    c = BWD_CASES[ci]
    ones = [torch.ones(c.b, n, *c.shp, device="cuda") for n in c.segc]
    m = ops.conv3d_prologue(ones, drop=DROP).cpu()
    keep = m / (1.0 / (1.0 - DROP[1]))
    assert bool(((keep == 0) | ((keep - 1).abs() < 1e-6)).all()) and 0.1 < float((keep == 0).float().mean()) < 0.3
    return m


@functools.lru_cache(maxsize=None)
def bwd_ref(ci, mkey):
    """fp64 autograd of (x' * gp).sum(), x' = act(cat(x) + shift) * scale * mask: dx per segment, d_shift / d_scale [B, Cin], the
    sums of their absolute terms per plane and |gp * scale|.  One per (case, prologue), shared by the options."""
    c = BWD_CASES[ci]
    xs, gp, _, _ = bwd_inputs(ci)
    sh, sc, act, mk = bwd_math(ci, mkey)
    cin, b = sum(c.segc), c.b
    mask = {"mask": lambda: rand_mask(313, b, cin, *c.shp), "drop": lambda: device_keep_mask(ci), None: lambda: None}[mk]()
    leaves = [x.double().requires_grad_(True) for x in xs]
    expand = lambda r: None if r is None else (r[None].expand(b, -1) if r.dim() == 1 else r).double().clone().requires_grad_(True)
    shl, scl = expand(sh), expand(sc)
    with torch.enable_grad():
        u = torch.cat(leaves, 1)
        if shl is not None:
            u = u + shl[:, :, None, None, None]
        a = silu64(u) if act else u
        xp = a if scl is None else a * scl[:, :, None, None, None]
        xp = xp if mask is None else xp * mask.double()
        (xp * gp.double()).sum().backward()
    dx = torch.cat([t.grad for t in leaves], 1)
    gm = gp.double() if mask is None else gp.double() * mask.double()
    zeros = torch.zeros(b, cin, dtype=F64)
    return dict(dx=[t.grad for t in leaves], mask=mask,
                dsh=dx.sum((2, 3, 4)) if shl is None else shl.grad, dsc=(gm * a.detach()).sum((2, 3, 4)) if scl is None else scl.grad,
                s_sh=dx.abs().sum((2, 3, 4)), s_sc=(gm * a.detach()).abs().sum((2, 3, 4)),
                gscale=(gp.double() if scl is None else gp.double() * scl.detach()[:, :, None, None, None]).abs(), zeros=zeros)


def bwd_call(ops, desc, gp, dx, acc, want_shift, want_scale, add=None, workspace=True):
    if workspace:
        return ops.conv3d_prologue_bwd(desc, gp, dx, acc, want_shift, want_scale, add_segs=add)
    from tmdiff_amd import _lib                       # (ops always hands the workspace in: the plain entry point by hand)
    mk = lambda want: torch.empty(desc.B, desc.Cin, device="cuda") if want else None
    dsh, dsc = mk(want_shift), mk(want_scale)
    ptr = lambda t: None if t is None else t.data_ptr()
    dxp = (C.c_void_p * 3)(*[ptr(t) for t in dx], *([None] * (3 - len(dx))))
    accp = (C.c_int32 * 3)(*[1 if a else 0 for a in acc], *([0] * (3 - len(acc))))
    _lib.check(_lib.lib.tmdiff_conv3d_prologue_bwd(C.byref(desc), gp.data_ptr(), dxp, accp, ptr(dsh), ptr(dsc), ops.stream_ptr()),
               "conv3d_prologue_bwd")
    return dsh, dsc


@pytest.mark.parametrize("ci,opt", BWD_RUNS, ids=[f"{BWD_CASES[i].name}-{o}" for i, o in BWD_RUNS])
def test_prologue_backward_vs_fp64(ops, ci, opt):
    """prologue_bwd_kernel (+ rowsum_kernel): dL/dx per segment, d_shift[b, c], d_scale[b, c] against fp64 autograd on the float4
    and the scalar branch, with one slice and with 2 / 4 slices per plane (whole slices, a shorter last slice, an odd split of an
    odd plane), and per option: a mask tensor, in-kernel dropout (the mask the forward draws, recovered from the device), no
    act, no shift, no scale, shift and scale as one [Cin] row (d_shift / d_scale stay per (b, c), bit for bit those of the same row
    given B times), either or neither sum asked for, a segment without dx, accumulate, add_segs, no workspace (one slice).

    dx is elementwise: |dx - ref| <= 2e-6 * |gp * scale| per element, the SiLU tolerance of the forward (ELEM_MAX; SiLU' is
    formed from the same fast exponential); with accumulate / add_segs against prior + ref, plus the one rounding of that sum,
    2^-24 * |prior + ref|.  Outputs start as NaN, so an element nobody writes fails.
    d_shift / d_scale: |err| <= (D + c) * 2^-24 * sum|terms| over the plane, terms = gp * mask * scale * SiLU'(x + shift) and
    gp * mask * SiLU(x + shift); D = bwd_depth (elements per lane of a slice + 6 shuffle steps + 3 additions of the 4 waves'
    sums + the slices: 13, 10, 19, 21, 20, 23 for the six cases, 29 for the last one without a workspace) and c = 2e-6 / 2^-24
    = 33.6, the error each term may carry itself.  What is only read (x, gp, the mask, add_segs) is unchanged afterwards."""
    from tmdiff_amd import _lib
    c = BWD_CASES[ci]
    cin, plane, nseg = sum(c.segc), math.prod(c.shp), len(c.segc)
    xs, gp, _, _ = bwd_inputs(ci)
    sh, sc, act, mk = bwd_math(ci, opt)
    ref = bwd_ref(ci, opt if opt in ("mask", "drop", "noact", "noshift", "noscale", "rows") else "base")
    xd, gd, shd, scd = [cu(x) for x in xs], cu(gp), cu(sh), cu(sc)
    md = cu(ref["mask"]) if mk == "mask" else None
    kw = dict(in_shift=shd, in_scale=scd, in_act=act, in_mask=md, **stride_kw(sh, sc))
    if mk == "drop":
        kw["drop"] = DROP
    desc = ops.make_conv_desc(xd, 0, cin, 3, gd, **kw)
    slices = BWD_SLICES[ci]
    assert slices == bwd_slices(c.b, cin, plane)
    assert _lib.lib.tmdiff_conv3d_prologue_bwd_workspace_bytes(C.byref(desc)) == (2 * c.b * cin * slices * 4 if slices > 1 else 0)
    if opt == "no_workspace":
        slices = 1
    want_shift, want_scale = opt not in ("scale_only", "neither"), opt not in ("shift_only", "neither")
    dx = [torch.full_like(x, NAN) for x in xd]
    prior = [torch.zeros_like(x) for x in xs]
    acc, add = [False] * nseg, None
    if opt == "dx_none":
        dx[nseg - 1] = None
    elif opt == "accumulate":                     # the first segment holds another gradient already
        prior[0] = randn(320, *xs[0].shape)
        dx[0], acc[0] = cu(prior[0]), True
    elif opt == "add":                            # the last segment's other gradient is read from a tensor of its own
        prior[nseg - 1] = randn(321, *xs[nseg - 1].shape)
        add = [None] * (nseg - 1) + [cu(prior[nseg - 1])]
    dsh, dsc = bwd_call(ops, desc, gd, dx, acc, want_shift, want_scale, add, workspace=opt != "no_workspace")
    assert (dsh is not None) == want_shift and (dsc is not None) == want_scale
    # what is only read
    for t, src in zip(xd + [gd, md] + (add or []), xs + [gp, ref["mask"]] + ([None] * (nseg - 1) + [prior[nseg - 1]] if add else [])):
        assert t is None or torch.equal(t.cpu(), src), "an input was written"
    # dx
    worst_dx, c0 = 0.0, 0
    for i, n in enumerate(c.segc):
        if dx[i] is not None:
            want = prior[i].double() + ref["dx"][i]
            tol = ELEM_MAX * ref["gscale"][:, c0:c0 + n] + (U24 * want.abs() if (acc[i] or (add and add[i] is not None)) else 0.0)
            got = dx[i].cpu().double()
            assert bool(torch.isfinite(got).all()), f"segment {i}: dx holds elements nobody wrote"
            worst_dx = max(worst_dx, worst_ratio((got - want).abs(), tol))
        c0 += n
    # the sums
    depth = bwd_depth(plane, slices)
    assert depth == (29 if opt == "no_workspace" else [13, 10, 19, 21, 20, 23][ci])
    ratios = {}
    for name, got, want, terms in (("d_shift", dsh, ref["dsh"], ref["s_sh"]), ("d_scale", dsc, ref["dsc"], ref["s_sc"])):
        if got is not None:
            assert got.shape == (c.b, cin)
            ratios[name] = worst_ratio((got.cpu().double() - want).abs(), (depth + ELEM_C) * U24 * terms)
    print(f"\nedges prologue_bwd {c.name} {opt}: slices={slices} depth {depth}: worst |err| / bound dx {worst_dx:.3e}, " +
          ", ".join(f"{k} {v:.3e}" for k, v in ratios.items()))
    assert worst_dx <= 1.0, f"dx: {worst_dx:.3e} of 2e-6 * |gp * scale|"
    for name, r in ratios.items():
        assert r <= 1.0, f"{name}: {r:.3e} of ({depth} + {ELEM_C:.1f}) * 2^-24 * sum|terms|"
    if opt == "rows":                               # the same row given B times, densely: the same bits
        dense = lambda r: cu(r[None].expand(c.b, -1))
        shb, scb = dense(sh), dense(sc)
        d2 = ops.make_conv_desc(xd, 0, cin, 3, gd, in_shift=shb, in_scale=scb, in_act=act)
        dx2 = [torch.full_like(x, NAN) for x in xd]
        dsh2, dsc2 = ops.conv3d_prologue_bwd(d2, gd, dx2, acc, True, True)
        assert torch.equal(dsh, dsh2) and torch.equal(dsc, dsc2) and all(torch.equal(a, b_) for a, b_ in zip(dx, dx2))
    if opt in ("shift_only", "scale_only", "dx_none"):   # asking for less changes nothing of what is still asked for
        full = [torch.full_like(x, NAN) for x in xd]
        fsh, fsc = ops.conv3d_prologue_bwd(desc, gd, full, acc, True, True)
        assert (dsh is None or torch.equal(dsh, fsh)) and (dsc is None or torch.equal(dsc, fsc))
        assert all(a is None or torch.equal(a, b_) for a, b_ in zip(dx, full))


def test_prologue_backward_refuses_accumulate_with_add(ops):
    """accumulate on one segment and add_segs on another do not go into one launch: the wrapper says so (each is checked on
    its own above)."""
    xs, gp, sh, sc = bwd_inputs(0)
    xd, gd = [cu(x) for x in xs], cu(gp)
    desc = ops.make_conv_desc(xd, 0, gp.shape[1], 3, gd, in_shift=cu(sh), in_scale=cu(sc), in_act=True)
    dx = [torch.zeros_like(x) for x in xd]
    with pytest.raises(ValueError):
        ops.conv3d_prologue_bwd(desc, gd, dx, [True, False, False], True, True, add_segs=[None, torch.zeros_like(xd[1]), None])


# ---- 4. channel_sum ---------------------------------------------------------------------------------------------------------
CHANNEL_SUM = [(2, 3, 1), (1, 5, 2047), (2, 4, 2049), (3, 2, 5000), (0, 4, 64)]


@pytest.mark.parametrize("b,c,p", CHANNEL_SUM, ids=[f"B{b}-C{c}-P{p}" for b, c, p in CHANNEL_SUM])
def test_channel_sum_vs_fp64(ops, b, c, p):
    """out[c] = scale * sum_{b, p} x: one slice (P = 1, 2047), two slices of 1025 (P = 2049), three of 1667 with a last one of
    1666 (P = 5000), no sample at all (zeros).  The output starts as NaN: the kernel zeroes it, then every slice adds its part
    atomically.  Bound D * 2^-24 * |scale| * sum|x| with D from channel_sum_kernel: a lane adds at most ceil(slice / 256) values
    per sample (the unrolled trips add pairs first, which only shortens the chain), B samples; block_sum adds 6 shuffle steps
    and 3 additions of the waves' sums; one rounding of scale * s; the slices meet in `slices` atomic additions."""
    from tmdiff_amd import _lib
    slices = max(1, min(cdiv(2048, c), cdiv(p, 2048)))
    per = cdiv(p, slices)
    assert (slices, per) == {1: (1, 1), 2047: (1, 2047), 2049: (2, 1025), 5000: (3, 1667), 64: (1, 64)}[p]
    depth = b * cdiv(per, 256) + 6 + 3 + 1 + slices
    x = randn(400, b, c, p)
    xd = cu(x)
    for scale in (1.0, -1.7):
        out = torch.full((c + 2,), NAN, device="cuda")
        _lib.check(_lib.lib.tmdiff_channel_sum(xd.data_ptr() if b else None, out.data_ptr() + 4, b, c, p, scale, ops.stream_ptr()),
                   "channel_sum")
        got = out.cpu()
        assert bool(torch.isnan(got[0])) and bool(torch.isnan(got[-1])), "channel_sum wrote outside its output"
        got = got[1:-1]
        via_ops = ops.channel_sum(xd.reshape(b, c, p, 1, 1), scale).cpu()
        assert via_ops.shape == (c,)
        if b == 0:
            assert torch.equal(got, torch.zeros(c)) and torch.equal(via_ops, torch.zeros(c)), "channel_sum over no samples is not zero"
            continue
        want, terms = scale * x.double().sum((0, 2)), abs(scale) * x.double().abs().sum((0, 2))
        r0 = worst_ratio((got.double() - want).abs(), depth * U24 * terms)
        r1 = worst_ratio((via_ops.double() - want).abs(), depth * U24 * terms)
        print(f"\nedges channel_sum [{b},{c},{p}] scale={scale}: slices={slices} depth {depth}: worst |err| / bound {r0:.3e} (C ABI), "
              f"{r1:.3e} (ops)")
        assert r0 <= 1.0 and r1 <= 1.0, f"channel_sum: {max(r0, r1):.3e} of {depth} * 2^-24 * |scale| * sum|x|"
    assert torch.equal(xd.cpu(), x), "the input was written"
