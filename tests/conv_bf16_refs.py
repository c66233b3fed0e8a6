"""Host-side references for the bf16 forward convolution tmdiff_conv3d_fwd_bf16 (csrc/conv3d_bf16.hip): its dispatch restated,
inputs on which none of its fp32 operations rounds, the fp64 reference with prologue and epilogue in the kernel's order, bf16
rounding and the packed-unit layout on the host, and the elementwise bound of the rounding tier.  CPU only; nothing here imports
tmdiff_amd.  test_conv_bf16_refs_host.py proves these helpers, test_gpu_conv_bf16_edges.py uses them.

The operation (header of conv3d_bf16.hip):  x' = act(x + shift[b, c]) * scale[b, c] in fp32, rounded to bf16 (nearest even);
w rounded to bf16 once;  y = (sum_{ci, tap} w x' + bias * bias_scale + residual) * out_scale with fp32 accumulation and an fp32
epilogue;  the optional second output  y2 = bf16(act2(y + shift2[b, co]) * scale2[b, co])  as units of 8 channels,
[B, Cout / 8, N * H * W, 8] (ops.make_conv_desc) -- the layout a packed INPUT has as well.
"""
import collections

import torch

F64 = torch.float64
U24 = 2.0 ** -24
TN = 4                        # bands per workgroup of the 3x3x3 kernels (one per wave)
DELTA_ULPS = 8                # see flip_flags


def cdiv(a, b):
    return -(-a // b)


# ---- the cases ---------------------------------------------------------------------------------------------------------------
# shift / scale: a [B, Cin] bank of the input prologue; act: SiLU in the prologue (rounding tier only: the exact tier has no
# activation); bias / res: the epilogue's inputs; misalign: y and the residual start 4 bytes off a 16-byte boundary; emit: the
# second output -- None, "plain" (no shift, scale or act), "affine" (shift2 and scale2), "act" (affine + SiLU, rounding tier
# only); keep_y=False: the kernel's y is NULL.  bias_scale and out_scale follow from bias / res (scales_of).
Case = collections.namedtuple("Case", "name B segs cout groups k N H W shift scale act bias res misalign keep_y emit")


def _c(name, B, segs, cout, N, H, W, groups=1, k=3, shift=False, scale=False, act=False, bias=False, res=False, misalign=False,
       keep_y=True, emit=None):
    return Case(name, B, tuple(segs), cout, groups, k, N, H, W, shift, scale, act, bias, res, misalign, keep_y, emit)


CASES = [
    # <2,2,8,8>: cout_g a multiple of 64
    _c("A-n1-one-chunk", 1, (8,), 64, 1, 8, 8),
    _c("A-n5-w10-ragged", 1, (16,), 64, 5, 9, 10, bias=True, res=True),
    _c("A-n8-w12-cin24", 1, (24,), 64, 8, 6, 12, shift=True, scale=True, res=True),
    _c("A-cin64-16x16", 1, (64,), 64, 8, 16, 16, act=True, bias=True, res=True, emit="act"),
    _c("A-cout128-b3-n3", 3, (16,), 128, 3, 8, 8, bias=True),
    _c("A-w8-emit-misaligned", 2, (16,), 64, 4, 8, 8, bias=True, res=True, misalign=True, emit="affine"),
    _c("A-w8-emit-aligned", 2, (16,), 64, 4, 8, 8, bias=True, res=True, emit="affine"),
    _c("A-emit-only-n5", 1, (16,), 64, 5, 8, 8, bias=True, keep_y=False, emit="affine"),
    # <4,1,8,16>: the other channel counts at W >= 16
    _c("B-w16-boundary", 1, (16,), 32, 4, 8, 16, res=True),
    _c("B-w20-n5-segments", 2, (8, 16, 8), 32, 5, 9, 20, shift=True, scale=True, bias=True, res=True),
    _c("B-w17-cout96", 1, (16,), 96, 3, 5, 17, bias=True),
    _c("B-w16-emit-3seg", 2, (8, 16, 8), 32, 3, 8, 16, res=True, emit="affine"),
    _c("B-w20-emit-only-res", 1, (8,), 32, 4, 8, 20, res=True, keep_y=False, emit="plain"),
    # <2,1,8,8>: ... at W < 16
    _c("C-w15", 1, (16,), 32, 4, 8, 15),
    _c("C-w7-h1-b3", 3, (8,), 32, 2, 1, 7),
    _c("C-w9-two-segments", 1, (8, 8), 32, 8, 8, 9, scale=True, res=True),
    _c("C-w1", 1, (16,), 32, 3, 3, 1, bias=True),
    _c("C-w8-misaligned", 2, (16,), 32, 4, 8, 8, bias=True, res=True, misalign=True),
    _c("C-w8-aligned", 2, (16,), 32, 4, 8, 8, bias=True, res=True),
    _c("C-w12-emit-plain", 1, (16,), 32, 4, 7, 12, emit="plain"),
    _c("C-w10-emit-act-scalar", 1, (16,), 32, 4, 5, 10, act=True, bias=True, res=True, emit="act"),
    # groups = 3: one segment per group, and one tensor
    _c("g3-three-segments", 1, (16, 16, 16), 96, 4, 8, 8, groups=3, bias=True),
    _c("g3-one-tensor-cout192", 2, (48,), 192, 3, 6, 8, groups=3, emit="plain"),
    # 1x1x1: a workgroup takes 4 * NS * 32 positions -- 128 (cout_g % 128 == 0), 256 (% 64 == 0), 512 (the others)
    _c("k1-128-exact", 1, (16,), 128, 2, 8, 8, k=1, act=True),
    _c("k1-128-plus1", 2, (32,), 128, 1, 3, 43, k=1, bias=True, res=True),
    _c("k1-64-exact", 1, (16,), 64, 4, 8, 8, k=1, res=True),
    _c("k1-64-plus1-3seg", 1, (16, 16, 16), 64, 1, 1, 257, k=1, shift=True, scale=True, act=True, bias=True),
    _c("k1-32-exact", 1, (16,), 32, 8, 8, 8, k=1, bias=True),
    _c("k1-32-plus1-segments", 1, (8, 24), 32, 1, 19, 27, k=1, scale=True),
    _c("k1-one-position", 2, (16,), 32, 1, 1, 1, k=1, bias=True, res=True),
    _c("k1-g3-cin48", 1, (144,), 96, 3, 5, 7, groups=3, k=1, bias=True),
]
CASE = {c.name: c for c in CASES}
# the rounding tier: the three 3x3x3 configurations (each run fused and packed), the three 1x1x1 configurations, the act cases
ROUNDING_CASES = ["A-n5-w10-ragged", "A-cin64-16x16", "B-w20-n5-segments", "C-w9-two-segments", "C-w10-emit-act-scalar",
                  "A-w8-emit-aligned", "k1-128-exact", "k1-128-plus1", "k1-64-plus1-3seg", "k1-32-plus1-segments"]
SENSOR_CASES = ["A-cin64-16x16", "B-w20-n5-segments", "k1-64-plus1-3seg"]
# one ragged case per configuration (repeatability)
REPEAT_CASES = ["A-n5-w10-ragged", "B-w20-n5-segments", "C-w9-two-segments", "k1-128-plus1", "k1-64-plus1-3seg",
                "k1-32-plus1-segments"]


def seed_of(case):
    return 4000 + CASES.index(case)


def cin_of(case):
    return sum(case.segs)


def taps_of(case):
    return case.k ** 3


def out_elements(case):
    return case.B * case.cout * case.N * case.H * case.W


def scales_of(case):
    """(bias_scale, out_scale): 0.5 on a bias; the output doubled where there is a residual, halved where there is a bias alone"""
    return (0.5 if case.bias else 1.0), (2.0 if case.res else (0.5 if case.bias else 1.0))


def producer_route(case):
    """a packed input from a producer stands for one tensor without prologue, 3x3x3 only"""
    return case.k == 3 and len(case.segs) == 1 and not (case.shift or case.scale)


# ---- the dispatch at the end of tmdiff_conv3d_fwd_bf16, restated ---------------------------------------------------------------
Config = collections.namedtuple("Config", "kernel NS MSUB TH TW tiles_n tiles_h tiles_w tiles_co blocks vec4 workspace_bytes")


def config_of(case):
    """kernel "k3" (fused, packed-input and producer-packed routes share the tile) or "k1"; the tile <NS, MSUB, TH, TW> (k1: NS
    and MSUB, a workgroup covers 4 * NS * 32 positions: TH = 1, TW = that count); tile counts; vec4: the host's choice of the
    dwordx4 epilogue (taken by the packed-input kernel only); the pack pass's workspace, 2 bytes per input element (0 where its
    grid of B * Cin / 8 rows is refused)."""
    cin, cout_g = cin_of(case), case.cout // case.groups
    plane = case.N * case.H * case.W
    vec4 = case.W % 4 == 0 and not case.misalign and plane < 2 ** 24
    ws = case.B * cin * plane * 2 if (cin % 8 == 0 and case.B * (cin // 8) <= 65535) else 0
    if case.k == 1:
        ns, msub = (1, 4) if cout_g % 128 == 0 else ((2, 2) if cout_g % 64 == 0 else (4, 1))
        tw = 4 * ns * 32
        tiles_w, tiles_co = cdiv(plane, tw), cout_g // (32 * msub)
        return Config("k1", ns, msub, 1, tw, 1, 1, tiles_w, tiles_co, case.B * case.groups * tiles_w * tiles_co, vec4, ws)
    ns, msub, th, tw = (2, 2, 8, 8) if cout_g % 64 == 0 else ((4, 1, 8, 16) if case.W >= 16 else (2, 1, 8, 8))
    tn, th_n, tw_n, tco = cdiv(case.N, TN), cdiv(case.H, th), cdiv(case.W, tw), cout_g // (32 * msub)
    return Config("k3", ns, msub, th, tw, tn, th_n, tw_n, tco, case.B * case.groups * tn * th_n * tw_n * tco, vec4, ws)


# ---- bf16 on the host ----------------------------------------------------------------------------------------------------------
def bf16_bits(t):
    """fp32 -> the 16 bits of the nearest bf16 number, ties to even, by integer arithmetic on the fp32 pattern (finite inputs)"""
    u = t.contiguous().float().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return (((r & 0xFFFF) ^ 0x8000) - 0x8000).to(torch.int16)


def bf16_value(bits):
    """the fp32 value of bf16 bit patterns (an int16 tensor)"""
    u = (bits.to(torch.int64) & 0xFFFF) << 16
    return ((u ^ 0x80000000) - 0x80000000).to(torch.int32).view(torch.float32)


def bf16_rne(t):
    return bf16_value(bf16_bits(t))


def pack_units(t):
    """[B, C, N, H, W] -> the bf16 units [B, C / 8, N * H * W, 8] (int16 storage), rounding to nearest even"""
    B, C = t.shape[:2]
    return bf16_bits(t.reshape(B, C // 8, 8, -1).permute(0, 1, 3, 2).contiguous())


def unpack_units(units, shape):
    """the fp32 values [B, C, N, H, W] of bf16 units [B, C / 8, N * H * W, 8]"""
    return bf16_value(units).permute(0, 1, 3, 2).reshape(shape).contiguous()


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def _bank(t):
    return None if t is None else t.double()[:, :, None, None, None]


def lattice_inputs(case, seed=None):
    """Inputs on which no operation of the kernel rounds: x and w integers in [-4, 4], integer bias and residual in [-8, 8], an
    integer input shift in [-2, 2], integer second-output shift in [-4, 4], every scale a row of 0.5 / 1 / 2, no activation."""
    gen = torch.Generator().manual_seed(seed_of(case) if seed is None else seed)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen).float()
    B, cin, shp = case.B, cin_of(case), (case.N, case.H, case.W)
    bs, os_ = scales_of(case)
    d = dict(xs=[ri(-4, 4, B, c, *shp) for c in case.segs], w=ri(-4, 4, case.cout, cin // case.groups, *(case.k,) * 3),
             shift=ri(-2, 2, B, cin) if case.shift else None, scale=2.0 ** ri(-1, 1, B, cin) if case.scale else None, act=False,
             bias=ri(-8, 8, case.cout) if case.bias else None, res=ri(-8, 8, B, case.cout, *shp) if case.res else None,
             bias_scale=bs, out_scale=os_, emit_shift=None, emit_scale=None, emit_act=False)
    if case.emit in ("affine", "act"):
        d["emit_shift"], d["emit_scale"] = ri(-4, 4, B, case.cout), 2.0 ** ri(-1, 1, B, case.cout)
    return d


def real_inputs(case, seed=None):
    """The two input sets of the rounding tier.  "normal": N(0, 1) data, weights N(0, 1) / sqrt(taps * cin_g), so that outputs are
    of order 1.  "sensor": x = 1000 + 5 N(0, 1) with a shift of -1000 (a bank is added whatever the case says), so that the
    fp32 add of the prologue carries the whole signal.  The case's act / emit act are on."""
    gen = torch.Generator().manual_seed(7000 + (seed_of(case) if seed is None else seed))
    rn = lambda *shape: torch.randn(*shape, generator=gen)
    ru = lambda *shape: torch.rand(*shape, generator=gen) + 0.5
    B, cin, shp = case.B, cin_of(case), (case.N, case.H, case.W)
    cin_g = cin // case.groups
    bs, os_ = scales_of(case)
    d = dict(xs=[rn(B, c, *shp) for c in case.segs], w=rn(case.cout, cin_g, *(case.k,) * 3) / (taps_of(case) * cin_g) ** 0.5,
             shift=0.5 * rn(B, cin) if case.shift else None, scale=ru(B, cin) if case.scale else None, act=case.act,
             bias=rn(case.cout) if case.bias else None, res=rn(B, case.cout, *shp) if case.res else None,
             bias_scale=bs, out_scale=os_, emit_shift=None, emit_scale=None, emit_act=case.emit == "act")
    if case.emit in ("affine", "act"):
        d["emit_shift"], d["emit_scale"] = 0.5 * rn(B, case.cout), ru(B, case.cout)
    s = dict(d)
    s["xs"] = [1000.0 + 5.0 * rn(B, c, *shp) for c in case.segs]
    s["shift"] = torch.full((B, cin), -1000.0)
    return {"normal": d, "sensor": s}


def prologue64(inp):
    """x' = act(cat(x) + shift) * scale in fp64"""
    u = torch.cat(inp["xs"], 1).double()
    if inp["shift"] is not None:
        u = u + _bank(inp["shift"])
    if inp["act"]:
        u = u * torch.sigmoid(u)
    if inp["scale"] is not None:
        u = u * _bank(inp["scale"])
    return u


# ---- the reference -------------------------------------------------------------------------------------------------------------
def conv64(xp, w, groups):
    """sum_{ci, tap} w[co, ci, tap] x'[ci, pos + tap - centre] in fp64, zero outside the image: tap by tap, group by group"""
    B, cin, N, H, W = xp.shape
    cout, cin_g, k = w.shape[0], w.shape[1], w.shape[2]
    p = k // 2
    xpad = torch.zeros(B, groups, cin_g, N + 2 * p, H + 2 * p, W + 2 * p, dtype=F64)
    xpad[:, :, :, p:p + N, p:p + H, p:p + W] = xp.double().reshape(B, groups, cin_g, N, H, W)
    wg = w.double().reshape(groups, cout // groups, cin_g, k, k, k)
    out = torch.zeros(B, groups, cout // groups, N, H, W, dtype=F64)
    for dz in range(k):
        for dy in range(k):
            for dx in range(k):
                out += torch.einsum("bgcnhw,goc->bgonhw", xpad[:, :, :, dz:dz + N, dy:dy + H, dx:dx + W], wg[:, :, :, dz, dy, dx])
    return out.reshape(B, cout, N, H, W)


def epilogue64(conv, inp, absolute=False):
    """(conv + bias * bias_scale + residual) * out_scale; absolute: of absolute values"""
    ab = (lambda t: t.abs()) if absolute else (lambda t: t)
    y = conv
    if inp["bias"] is not None:
        y = y + ab(inp["bias"].double() * inp["bias_scale"])[None, :, None, None, None]
    if inp["res"] is not None:
        y = y + ab(inp["res"].double())
    return y * (abs(inp["out_scale"]) if absolute else inp["out_scale"])


def second64(y, inp):
    """act2(y + shift2) * scale2 in fp64 (before the rounding to bf16)"""
    t = y.double()
    if inp["emit_shift"] is not None:
        t = t + _bank(inp["emit_shift"])
    if inp["emit_act"]:
        t = t * torch.sigmoid(t)
    if inp["emit_scale"] is not None:
        t = t * _bank(inp["emit_scale"])
    return t


def reference(case, inp, xq=None, wq=None):
    """dict(y=, t2=) in fp64: the convolution of x' (xq: the operand as the kernel multiplies it, default the fp64 prologue of the
    inputs) with w (wq likewise), the epilogue, and for a case with a second output its value before the rounding to bf16"""
    xq = prologue64(inp) if xq is None else xq
    y = epilogue64(conv64(xq, inp["w"] if wq is None else wq, case.groups), inp)
    return dict(y=y, t2=second64(y, inp) if case.emit else None)


def epilogue_roundings(inp):
    """E: the fp32 roundings between the accumulator and y (store_tile, store_tile_v, conv1_bf16_kernel): the product bias *
    bias_scale, the sum acc + bias, the sum with the residual, the product with out_scale (exact when that is 1)"""
    return 2 * (inp["bias"] is not None) + (inp["res"] is not None) + (inp["out_scale"] != 1.0)


def flip_flags(xp32):
    """Operands whose fp32 x' lies within DELTA_ULPS = 8 fp32 ulps of a bf16 rounding tie (low 16 bits 0x8000).  Two evaluations
    of x' that differ by a relative delta <= 3 * 2^-23 (test_gpu_conv_bf16_edges.py derives it) differ by at most
    delta * |x'| / ulp < 3 * 2^-23 * 2^24 = 6 ulps; 8 leaves room for the second-order terms.  Only such operands can round to
    different bf16 numbers in the two evaluations."""
    low = xp32.contiguous().view(torch.int32).to(torch.int64) & 0xFFFF
    return (low - 0x8000).abs() <= DELTA_ULPS


def bound(case, xq, wq, inp, xp32=None):
    """(K + E) * 2^-24 * A + F, elementwise.  K = taps * cin_g products and sums behind an accumulator; A = the same convolution
    and epilogue of absolute values; F = |out_scale| * sum 2^-8 |w_r| |x'| over the operands flip_flags marks (xp32: the fp32 x'
    of the prologue pass, given only where the kernel evaluates the prologue by another function: SiLU)."""
    conv_abs = conv64(xq.abs(), wq.abs(), case.groups)
    K = taps_of(case) * (cin_of(case) // case.groups)
    out = (K + epilogue_roundings(inp)) * U24 * epilogue64(conv_abs, inp, absolute=True)
    if xp32 is not None:
        out = out + abs(inp["out_scale"]) * conv64(2.0 ** -8 * xp32.double().abs() * flip_flags(xp32), wq.abs(), case.groups)
    return out


def second_tolerance(y_dev, inp):
    """One bf16 ulp as a relative 2^-8 of t = act2(y + shift2) * scale2, plus the fp32 roundings of the chain on the device's own
    y: the sum u = y + shift2 (2^-24 |u|, carried through a slope of at most 1.1 and the scale), the scale product (2^-24 |t|) and
    for SiLU exp(-u) (its argument scaled by log2 e: |u| 2^-24, v_exp_f32 1 ulp = 2^-23), 1 + e (2^-24), v_rcp_f32 (1 ulp =
    2^-23) and the product (2^-24): (|u| + 7) 2^-24 |t| in all."""
    u = y_dev.double() + (_bank(inp["emit_shift"]) if inp["emit_shift"] is not None else 0.0)
    t = second64(y_dev, inp)
    sc = _bank(inp["emit_scale"]).abs() if inp["emit_scale"] is not None else 1.0
    if inp["emit_act"]:
        chain = U24 * ((u.abs() + 7.0) * t.abs() + 1.1 * u.abs() * sc)
    else:
        chain = U24 * (t.abs() + u.abs() * sc)
    return 2.0 ** -8 * t.abs() + chain


# ---- exactness of the lattice tier -----------------------------------------------------------------------------------------------
def exactness_ok(case):
    """On lattice_inputs(case) every operand is a bf16 number and every value the kernel forms is an fp32 number: x' and w are
    multiples of 1/2 of at most 8 bits; every product is a multiple of 1/2, the epilogue's terms multiples of 1/4, the second
    output's of 1/8; and the sum of the absolute terms behind any value, max|x'| * max|w| * taps * cin_g plus the epilogue terms
    (16 * taps * cin_g without a prologue), stays below 2^24 quanta, so that every partial sum in any order is an fp32 number."""
    inp = lattice_inputs(case)
    xp = prologue64(inp)
    assert torch.equal(bf16_rne(xp.float()).double(), xp), "x' is not a bf16 number"
    assert torch.equal(bf16_rne(inp["w"]).double(), inp["w"].double()), "w is not a bf16 number"
    assert torch.equal(xp * 2, (xp * 2).round()) and torch.equal(inp["w"], inp["w"].round())
    K = taps_of(case) * (cin_of(case) // case.groups)
    acc = float(xp.abs().max()) * float(inp["w"].abs().max()) * K
    assert acc <= (16 if not (case.shift or case.scale) else 48) * K
    bs, os_ = inp["bias_scale"], inp["out_scale"]
    for s in (bs, os_):
        assert s in (0.5, 1.0, 2.0)
    total = acc + (8 * bs if case.bias else 0) + (8 if case.res else 0)
    assert total * 4 < 2.0 ** 24 and total * max(os_, 1.0) * 4 < 2.0 ** 24, total          # quanta of 1/4 before and after out_scale
    if case.emit:
        t = (total * os_ + 4) * 2                                                       # |y + shift2| * scale2, quanta of 1/8
        assert t * 8 < 2.0 ** 24, t
        for r in (inp["emit_shift"], inp["emit_scale"]):
            assert r is None or torch.equal(r * 2, (r * 2).round())
    return True
