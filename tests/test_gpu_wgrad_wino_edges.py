"""tmdiff_conv3d_wgrad_wino (csrc/wgrad_wino.hip) at its edges: the transform pass's padding and chunk borders, both box
geometries, one to four band tiles, single live channels in a tile or chunk, the reduce kernel's second input-channel chunk,
groups = 3 with cout_g < CoP, segment borders inside a 32-channel chunk, the staged x' path with a mask and with in-kernel
dropout, every class of split (wgrad_wino_refs.CASES; test_wgrad_wino_refs_host.py asserts what each case reaches), a poisoned
workspace, and what the entry point refuses.  Every call goes through ops.make_conv_desc and ops.conv3d_wgrad(family="wino");
ops.COUNTS shows which kernel ran, and the library's workspace byte count must equal the restated plan's (same split count).

Exact tier.  On lattice inputs (x integers in [-2, 2], g = 24 j, exact prologue parts) no fp32 operation of the kernel rounds
(wgrad_wino_refs.exactness_ok, proved on the host), so dw and dbias must EQUAL the fp64 reference, bit for bit: one lost,
doubled or misplaced term is an error of at least 1/8, whatever the sizes.

Rounding tier.  On real-valued data  |dw - ref| <= c * 2^-24 * M  elementwise, M = dw_abs64: the Winograd chain with every
matrix and operand replaced by its absolute value, so that every intermediate a rounding can act on is bounded by its part of
M.  c counts the roundings on the longest path from an input element to a dw element, read from the kernels:
    2   B^T x: o[0] = (4 d0 + d4) - 5 d2 -- a product or a sum, then the difference (4 d, 2 d are exact); the others likewise
    4   G' g:  the rounded constant (1/6, 1/24, ...), s02 or the product, the sum, the final sum / product
    1   the product g^ x^ inside the MFMA
    2 * bw * bps   one accumulator adds the 2 * bw positions of its two rows of a box (bw / 2 K-steps per row, two positions each),
        box after box, bps boxes of the plan's split range
    3   the four waves' sums, ((T0 + T1) + T2) + T3
    ceil(splits / 4) + 3   ww_reduce_kernel: a thread group adds every fourth split, then the four group sums
    3   A'^T: dst[18] = (p12 + 4 p34) + m5 with p12 = m1 + m2
so c = 2 * bw * bps + ceil(splits / 4) + 16 (Plan.depth): 49 for one 8 x 16 box per workgroup and up to four splits, 81 for
the case with two boxes per workgroup.  (1 + u)^c - 1 exceeds c u by c^2 u^2 / 2 < 3e-9 of it: nothing at these c.)
dbias:  |dbias - ref| <= D * 2^-24 * |bias_scale| * sum|g|,  D = 2 (a quad (x + y) + (z + w)) + 8 (a lane adds its eight live
quads) + 3 (butterfly over the eight lanes of a channel) + ceil(nbias / 8) + 7 (eight slices of the workgroup sums, then the
slices) + 1 (bias_scale) (Plan.bias_depth).  x' with SiLU is taken from the device (ops.conv3d_prologue, the pass this kernel
stages x' with; test_gpu_backward_edges.py holds it to fp64), so both sides multiply the same fp32 numbers.
c and D are derived, not tuned.  Worst |err| / bound observed on the MI355X ("edges" lines; direct = the direct kernel in the
same units, for information):
    case                   c   D   normal: dw (direct) dbias          sensor: dw (direct)    prologue: dw (direct)
    four-band-tiles        49  25  2.2e-03 (1.1e-03) 2.7e-03          9.0e-04 (8.4e-04)      3.0e-03 (1.6e-03)
    cin128-full-chunks     49  22  6.7e-03 (4.1e-03) 7.0e-03          2.6e-03 (2.7e-03)      7.3e-03 (3.6e-03)
    boxes7-16-tiles        81  28  2.7e-03 (1.0e-03) 4.6e-03          8.0e-04 (7.5e-04)      2.5e-03 (1.2e-03)
    groups3-cin40-cout33   49  25  3.6e-03 (1.4e-03) 5.2e-03          1.4e-03 (1.1e-03)      4.3e-03 (1.7e-03)
    segments-5-30-6        49  22  5.2e-03 (2.4e-03) 4.6e-03          2.3e-03 (1.7e-03)      6.1e-03 (2.9e-03)
(dbias does not depend on x: one figure per case.)  The certain bound is 140 to 1200 times what the kernel does on these data;
its job is precision on real-valued data -- an operand rounded to bf16 costs 2^-9 per term against c * 2^-24 = 3e-6 --
and the exact tier's job is every lost or misplaced term.
groups3-segments-10-10-4 (segment borders that are no group borders): the entry point takes such segments -- the transform
pass decodes every channel's segment itself -- and the result is exact; were it to refuse them, the test asserts the refusal.
"""
import collections
import ctypes as C
import functools

import pytest
import torch

import wgrad_wino_refs as R
from oracle.make_golden import randn

pytestmark = pytest.mark.gpu

U24 = R.U24
DROP = (987654321012, 0.2)
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from tmdiff_amd import ops as _ops
    return _ops


def cu(t):
    return None if t is None else t.cuda().contiguous()


def rand_mask(seed, *shape):
    """a host-drawn dropout mask: 0 or 1 / 0.8"""
    return (torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) > 0.2).float() / 0.8


def stride_kw(shift, scale):
    """make_conv_desc's stride arguments: a [Cin] row is a bank of one row broadcast over the batch (stride < 0 -> 0)"""
    return dict(shift_stride=-1 if shift is not None and shift.dim() == 1 else 0,
                scale_stride=-1 if scale is not None and scale.dim() == 1 else 0)


def worst_ratio(err, bound):
    """max of err / bound; where the bound is 0 (all terms zero) the error must be 0 as well (test_gpu_backward_edges.py)"""
    err, bound = err.double(), bound.double()
    assert bool((err[bound == 0] == 0).all()), "an error where every term is zero"
    live = bound > 0
    return float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0


def off_by_one_float(t):
    """t's values in a window one float into a larger buffer: contiguous, 4 bytes off a 16-byte boundary"""
    buf = torch.full((t.numel() + 8,), NAN, device="cuda", dtype=torch.float32)
    win = buf[1:1 + t.numel()].view(t.shape)
    win.copy_(t)
    assert win.is_contiguous() and win.data_ptr() % 16 == 4
    return win


def dev_kw(parts):
    """make_conv_desc's prologue keywords from CPU tensors (shift, scale, mask); the device tensors are returned to be kept alive"""
    sh, sc, mk = parts.get("shift"), parts.get("scale"), parts.get("mask")
    kw = dict(in_shift=cu(sh), in_scale=cu(sc), in_mask=cu(mk), in_act=bool(parts.get("act")), **stride_kw(sh, sc))
    return {k: v for k, v in kw.items() if v is not None and v is not False}


def run(ops, case, xd, gd, want_bias=False, bias_scale=1.0, family="wino", prologue=False, **kw):
    """ops.conv3d_wgrad on device tensors: the descriptor is supported, its workspace is the restated plan's, and COUNTS shows
    the Winograd kernel alone (family="direct": the direct kernel alone).  CPU results."""
    from tmdiff_amd import _lib
    pl = R.case_plan(case)
    desc = ops.make_conv_desc(xd, 0, case.cout, 3, gd, groups=case.groups, bias_scale=bias_scale, **kw)
    assert _lib.lib.tmdiff_conv3d_wgrad_wino_supported(C.byref(desc)) == 1
    assert _lib.lib.tmdiff_conv3d_wgrad_wino_workspace_bytes(C.byref(desc)) == pl.workspace_bytes(prologue), \
        f"{case.name}: the library's workspace is not the restated plan's ({pl.splits} splits x {pl.bps})"
    wshape = (case.cout, pl.cin_g, 3, 3, 3)
    keep, ops.COUNTS = ops.COUNTS, collections.Counter()
    try:
        out = ops.conv3d_wgrad(desc, gd, wshape, want_bias=want_bias, family=family)
        counts = dict(ops.COUNTS)
    finally:
        ops.COUNTS = keep
    wino = family == "wino"
    assert counts.get("conv3d_wgrad_wino", 0) == int(wino) and counts.get("conv3d_wgrad", 0) == int(not wino), counts
    return (out[0].cpu(), out[1].cpu()) if want_bias else out.cpu()


@functools.lru_cache(maxsize=None)
def lattice(name, variant="plain"):
    """(inputs, x' fp32, dw fp64, sum of g per channel fp64) of a case's lattice inputs: one per (case, variant), shared"""
    c = R.CASE[name]
    opts = {"plain": {}, "shift": dict(shift=True), "rows": dict(scale="rows"), "row": dict(scale="row"), "mask": dict(mask=True),
            "all": dict(shift=True, scale="rows", mask=True)}[variant]
    d = R.lattice_inputs(1000 + R.CASES.index(c), c.B, c.segc, c.cout, c.N, c.H, c.W, **opts)
    xp = R.prologue64(d["xs"], d["shift"], d["scale"], d["mask"]).float()
    ref, sg = R.dw_ref64(xp, d["g"], c.groups)
    assert torch.equal(ref.float().double(), ref)
    return d, xp, ref, sg


def segments_refused(ops, case, xd, gd):
    """True when the library does not take these segments: then family="wino" raises and family=None runs the direct kernel"""
    from tmdiff_amd import _lib
    desc = ops.make_conv_desc(xd, 0, case.cout, 3, gd, groups=case.groups)
    if _lib.lib.tmdiff_conv3d_wgrad_wino_supported(C.byref(desc)) == 1:
        return False
    wshape = (case.cout, sum(case.segc) // case.groups, 3, 3, 3)
    keep, ops.COUNTS = ops.COUNTS, collections.Counter()
    try:
        with pytest.raises(ValueError):
            ops.conv3d_wgrad(desc, gd, wshape, family="wino")
        ops.conv3d_wgrad(desc, gd, wshape)
        assert ops.COUNTS["conv3d_wgrad"] == 1 and ops.COUNTS["conv3d_wgrad_wino"] == 0, dict(ops.COUNTS)
    finally:
        ops.COUNTS = keep
    return True


# ---- 3a. the exact tier --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_exact_on_the_lattice(ops, case):
    """dw == fp64 reference and dbias == bias_scale * sum g, bit for bit, for bias_scale 1, 0.5 and -2; without the bias gradient
    the same dw bits; the inputs are only read; g = 0 gives dw = 0 and a zero input channel (the last one: the single live
    channel of its tile where there is one) gives dw[:, ci] = 0, everything else unchanged."""
    d, xp, ref, sg = lattice(case.name)
    pl = R.case_plan(case)
    xd, gd = [cu(x) for x in d["xs"]], cu(d["g"])
    if case.name == "groups3-segments-10-10-4" and segments_refused(ops, case, xd, gd):
        return
    want = ref.float()
    dw0 = run(ops, case, xd, gd)
    nbad = int((dw0 != want).sum())
    assert torch.equal(dw0, want), f"{case.name}: {nbad} of {want.numel()} dw elements differ, worst {float((dw0 - want).abs().max())}"
    for bs in (1.0, 0.5, -2.0):
        dw, db = run(ops, case, xd, gd, want_bias=True, bias_scale=bs)
        assert torch.equal(dw, dw0), f"{case.name}: dw changes with the bias gradient on the side (bias_scale {bs})"
        assert torch.equal(db, (bs * sg).float()), f"{case.name}: dbias, bias_scale {bs}: {db.tolist()} != {(bs * sg).tolist()}"
    for t, src in zip(xd + [gd], d["xs"] + [d["g"]]):
        assert torch.equal(t.cpu(), src), "an input was written"
    assert torch.equal(run(ops, case, xd, torch.zeros_like(gd)), torch.zeros_like(want)), "g = 0 does not give dw = 0"
    xz = [x.clone() for x in d["xs"]]
    xz[-1][:, -1] = 0
    wz = want.clone()
    wz[(case.groups - 1) * pl.cout_g:, pl.cin_g - 1] = 0
    dz = run(ops, case, [cu(x) for x in xz], gd)
    assert torch.equal(dz, wz), "a zero input channel: dw[:, ci] != 0 or another element changed"


PRO_RUNS = [(n, v) for n in R.PROLOGUE_CASES for v in ("shift", "rows", "row", "mask", "all")]


@pytest.mark.parametrize("name,variant", PRO_RUNS, ids=[f"{n}-{v}" for n, v in PRO_RUNS])
def test_exact_prologue_through_staged_input(ops, name, variant):
    """The staged x' path (prologue pass into the workspace, then one dense segment) with exact prologue parts: an integer shift,
    power-of-two scale rows as [B, Cin] and as one broadcast [Cin] row, a mask tensor of 0 / 1.25, all of them together; one,
    and three segments.  Exact."""
    case = R.CASE[name]
    d, xp, ref, sg = lattice(name, variant)
    xd, gd, kw = [cu(x) for x in d["xs"]], cu(d["g"]), dev_kw(d)
    dw, db = run(ops, case, xd, gd, want_bias=True, bias_scale=0.5, prologue=True, **kw)
    assert torch.equal(dw, ref.float()), f"{name} {variant}: {int((dw != ref.float()).sum())} dw elements differ"
    assert torch.equal(db, (0.5 * sg).float())


@pytest.mark.parametrize("name", ["cin128-full-chunks", "segments-5-30-6"])
def test_exact_with_in_kernel_dropout(ops, name):
    """drop = (seed, 0.2): the kept values are scaled by 1 / (1 - 0.2f) = 1.25 in fp32, which stays exact.  x' is what the forward
    convolution of the same descriptor keeps in xp_out (128 -> 32 channels: the staged kernel takes the shape), else the
    prologue pass's output; the keep mask is recovered from it; dw must equal the fp64 gradient on that x', bit for bit."""
    case = R.CASE[name]
    d, _, _, sg = lattice(name)
    pl = R.case_plan(case)
    xd, gd = [cu(x) for x in d["xs"]], cu(d["g"])
    x = torch.cat(d["xs"], 1)
    xp = ops.conv3d_prologue(xd, drop=DROP).cpu()
    if name == "cin128-full-chunks":
        w = cu(randn(7, case.cout, pl.cin_g, 3, 3, 3))
        kept = torch.full_like(cu(x), NAN)
        ops.conv3d(xd, ops.pack_conv_weight(w), case.cout, 3, xp_out=kept, drop=DROP)
        assert torch.equal(kept.cpu(), xp), "the forward's xp_out is not the prologue pass's x'"
    keep = (xp != 0) | (x == 0)
    assert torch.equal(xp, torch.where(keep, 1.25 * x, torch.zeros_like(x))), "x' is not 0 or 1.25 x"
    dropped = float(((xp == 0) & (x != 0)).float().sum() / (x != 0).float().sum())
    assert 0.1 < dropped < 0.3, dropped
    assert R.exactness_ok(xp, d["g"], pl)
    ref, _ = R.dw_ref64(xp, d["g"], case.groups)
    dw, db = run(ops, case, xd, gd, want_bias=True, prologue=True, drop=DROP)
    assert torch.equal(dw, ref.float()), f"{name}: {int((dw != ref.float()).sum())} dw elements differ"
    assert torch.equal(db, sg.float())


# ---- 3b. the rounding tier ---------------------------------------------------------------------------------------------------
ROUND_RUNS = [(n, k) for n in R.ROUNDING_CASES for k in ("normal", "sensor", "prologue")]


@pytest.mark.parametrize("name,kind", ROUND_RUNS, ids=[f"{n}-{k}" for n, k in ROUND_RUNS])
def test_rounding_bound(ops, name, kind):
    """|dw - ref| <= c * 2^-24 * M elementwise and |dbias - ref| <= D * 2^-24 * 2 sum|g| (module docstring) on N(0, 1) data, on
    sensor-scale data x = 1000 + 5 N(0, 1) (every B^T x cancels three digits) and behind the full prologue: shift, SiLU, scale,
    mask."""
    case = R.CASE[name]
    pl = R.case_plan(case)
    cin, shp = sum(case.segc), (case.N, case.H, case.W)
    xs = [randn(500 + i, case.B, c, *shp) for i, c in enumerate(case.segc)]
    g = randn(510, case.B, case.cout, *shp)
    parts = {}
    if kind == "sensor":
        xs = [1000.0 + 5.0 * x for x in xs]
    if kind == "prologue":
        parts = dict(shift=0.3 * randn(511, case.B, cin), scale=1 + 0.3 * randn(512, case.B, cin), mask=rand_mask(513, case.B, cin, *shp),
                     act=True)
    xd, gd, kw = [cu(x) for x in xs], cu(g), dev_kw(parts)
    dw, db = run(ops, case, xd, gd, want_bias=True, bias_scale=2.0, prologue=bool(parts), **kw)
    direct = run(ops, case, xd, gd, family="direct", prologue=bool(parts), **kw)
    xp = ops.conv3d_prologue(xd, **kw).cpu() if parts else torch.cat(xs, 1)
    ref, rb = R.dw_ref64(xp, g, case.groups, 2.0)
    M, Mb = R.dw_abs64(xp, g, pl, 2.0)
    c, D = pl.depth(), pl.bias_depth()
    ratio = worst_ratio((dw.double() - ref).abs(), c * U24 * M)
    ratio_d = float(((direct.double() - ref).abs() / (c * U24 * M).clamp_min(1e-300)).max())
    ratio_b = worst_ratio((db.double() - rb).abs(), D * U24 * Mb)
    print(f"\nedges wgrad_wino {name} {kind}: {pl.splits} splits x {pl.bps}, c = {c}, D = {D}: worst |err| / bound dw {ratio:.3e} "
          f"(direct {ratio_d:.3e}), dbias {ratio_b:.3e}")
    assert ratio <= 1.0, f"dw: {ratio:.3e} of the bound {c} * 2^-24 * M"
    assert ratio_b <= 1.0, f"dbias: {ratio_b:.3e} of the bound {D} * 2^-24 * bias_scale * sum|g|"


# ---- 3c. the workspace -------------------------------------------------------------------------------------------------------
def poison_workspace(ops, nbytes):
    """every byte of the cached "wgrad" workspace 0xFF: NaN bit patterns wherever a float is read that nobody wrote"""
    ws = ops._workspace(torch.device("cuda", torch.cuda.current_device()), nbytes, "wgrad")
    ws.fill_(0xFF)
    assert bool(torch.isnan(ws.view(torch.float32)).all())


@pytest.mark.parametrize("name", ["box8x8-six-padding-rows", "three-tiles-ragged-W12", "groups3-cin8-cout8"])
def test_result_does_not_depend_on_the_workspace(ops, name):
    """The transform pass writes every padding element itself: with the cached workspace full of NaN patterns before the call
    (8 x 8 box with six padding rows; 16-wide box with four padding columns; groups = 3 with 24 padding channels a group) dw and
    dbias are bit for bit those of the call before -- and the lattice reference."""
    case = R.CASE[name]
    d, _, ref, sg = lattice(name)
    xd, gd = [cu(x) for x in d["xs"]], cu(d["g"])
    dw, db = run(ops, case, xd, gd, want_bias=True)
    poison_workspace(ops, R.case_plan(case).workspace_bytes(False))
    dw2, db2 = run(ops, case, xd, gd, want_bias=True)
    assert torch.equal(dw2, dw) and torch.equal(db2, db), "the result depends on what the workspace held"
    assert torch.equal(dw2, ref.float()) and torch.equal(db2, sg.float())


def test_smaller_shape_after_a_larger_one(ops):
    """A larger shape, then a smaller one on the same (grow-only) workspace: the smaller result is its fresh result."""
    big, small = R.CASE["boxes7-16-tiles"], R.CASE["three-tiles-ragged-W12"]
    ds, _, ref, sg = lattice(small.name)
    xs, gs = [cu(x) for x in ds["xs"]], cu(ds["g"])
    poison_workspace(ops, R.case_plan(big).workspace_bytes(False))
    fresh = run(ops, small, xs, gs, want_bias=True)
    db_, _, refb, _ = lattice(big.name)
    assert torch.equal(run(ops, big, [cu(x) for x in db_["xs"]], cu(db_["g"])), refb.float())
    after = run(ops, small, xs, gs, want_bias=True)
    assert torch.equal(after[0], fresh[0]) and torch.equal(after[1], fresh[1])
    assert torch.equal(after[0], ref.float()) and torch.equal(after[1], sg.float())


# ---- 3d. refusals ------------------------------------------------------------------------------------------------------------
REFUSED = {
    # name: (B, Cin, Cout, N, H, W, groups, ksize)
    "N6": (1, 4, 4, 6, 8, 8, 1, 3),
    "N20": (1, 4, 4, 20, 8, 8, 1, 3),
    "W6": (1, 4, 4, 4, 8, 6, 1, 3),
    "groups2": (1, 4, 4, 4, 8, 8, 2, 3),
    "ksize1": (1, 4, 4, 4, 8, 8, 1, 1),
    "bf16-input": (1, 8, 4, 4, 8, 8, 1, 3),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refusals(ops, name):
    """N no multiple of 4, N > 16, W no multiple of 4, groups = 2, a 1x1x1 convolution, a bf16-packed input: the support query
    says 0, routing says "direct", family=None launches the direct kernel, family="wino" raises ValueError before anything
    runs, and the entry point itself returns an error and leaves dw as it was.  (The bf16-packed input is not launched with
    family=None: the direct kernel reads fp32 tensors and has no check of its own for this.)"""
    from tmdiff_amd import _lib, routing
    B, cin, cout, N, H, W, groups, k = REFUSED[name]
    gd = cu(randn(601, B, cout, N, H, W))
    bf16 = name == "bf16-input"
    if bf16:
        xd = [torch.zeros(B, cin // 8, N * H * W, 8, dtype=torch.int16, device="cuda")]
        desc = ops.make_conv_desc(xd, 0, cout, k, gd, groups=groups, x_bf16_shape=(N, H, W))
    else:
        xd = [cu(randn(600, B, cin, N, H, W))]
        desc = ops.make_conv_desc(xd, 0, cout, k, gd, groups=groups)
    wshape = (cout, cin // groups, k, k, k)
    assert _lib.lib.tmdiff_conv3d_wgrad_wino_supported(C.byref(desc)) == 0
    assert routing.wgrad_family(B, (cin,), cout, N, H, W, groups, k, False, **({"x_bf16": 1} if bf16 else {})) == "direct"
    assert not ops.wgrad_wino_takes(desc)
    keep, ops.COUNTS = ops.COUNTS, collections.Counter()
    try:
        if not bf16:
            ops.conv3d_wgrad(desc, gd, wshape)
            assert ops.COUNTS["conv3d_wgrad"] == 1 and ops.COUNTS["conv3d_wgrad_wino"] == 0, dict(ops.COUNTS)
        with pytest.raises(ValueError):
            ops.conv3d_wgrad(desc, gd, wshape, family="wino")
        assert ops.COUNTS["conv3d_wgrad_wino"] == 0, "a refused launch was counted"
    finally:
        ops.COUNTS = keep
    dw = torch.full(wshape, 7.0, device="cuda")
    ws = torch.zeros(1 << 16, device="cuda")
    rc = _lib.lib.tmdiff_conv3d_wgrad_wino_bias(C.byref(desc), gd.data_ptr(), dw.data_ptr(), None, ws.data_ptr(), ops.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and bool((dw == 7.0).all()), "a refused descriptor: dw was written"


def test_unaligned_gradient_is_refused(ops):
    """g one float into a larger buffer (not 16-byte aligned): the transform pass reads float4, so the entry point refuses;
    nothing is computed."""
    from tmdiff_amd import _lib
    case = R.CASE["box8x8-six-padding-rows"]
    d, _, _, _ = lattice(case.name)
    xd, gd = [cu(x) for x in d["xs"]], off_by_one_float(cu(d["g"]))
    desc = ops.make_conv_desc(xd, 0, case.cout, 3, cu(d["g"]), groups=case.groups)
    with pytest.raises((ValueError, _lib.TmdiffError)):
        ops.conv3d_wgrad(desc, gd, (case.cout, 4, 3, 3, 3), family="wino")
    dw = torch.full((case.cout, 4, 3, 3, 3), 7.0, device="cuda")
    ws = torch.zeros(R.case_plan(case).workspace_bytes(False) // 4, device="cuda")
    rc = _lib.lib.tmdiff_conv3d_wgrad_wino_bias(C.byref(desc), gd.data_ptr(), dw.data_ptr(), None, ws.data_ptr(), ops.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and bool((dw == 7.0).all()) and bool((ws == 0).all()), "an unaligned g: something was computed"
