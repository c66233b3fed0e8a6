"""Host-side references for the Winograd weight gradient tmdiff_conv3d_wgrad_wino (csrc/wgrad_wino.hip): its plan restated,
inputs on which its fp32 arithmetic is exact, the fp64 reference and the term-magnitude bound of the Winograd chain.  CPU only;
nothing here imports tmdiff_amd.  test_wgrad_wino_refs_host.py proves these helpers, test_gpu_wgrad_wino_edges.py uses them.

The algorithm (F(3, 4) along the bands, points 0, +-1, +-2, inf):  dw = A'^T [ (G' g) (.) (B^T x') ], summed per plane k over
every position of every band tile; x' carries one band of halo either side of a tile of four output bands.
"""
import collections

import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64
U24 = 2.0 ** -24

BT = [[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]]
G24 = [[6, 0, 0, 0], [-4, -4, -4, -4], [-4, 4, -4, 4], [1, 2, 4, 8], [1, -2, 4, -8], [0, 0, 0, 24]]      # 24 G'
AT = [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 1]]
TR_W = 64                     # columns per workgroup of the transform pass

FAULTS = ("lastbox", "halo", "column", "swap", "tap", "chunk2", "biasidx")


def cdiv(a, b):
    return -(-a // b)


def r4(v):
    return (v + 3) // 4 * 4


def choose_splits(total_boxes, units, per_round, overhead, smax):
    """common.h choose_splits: the split count among 1 .. min(smax, boxes) that minimises rounds * (boxes per workgroup +
    overhead), rounds = ceil(units * splits / per_round); ties to the smaller count; no split is empty.  (splits, boxes per split)"""
    best_s, best_cost = 1, 1e30
    for s in range(1, min(smax, total_boxes) + 1):
        bps = cdiv(total_boxes, s)
        s_eff = cdiv(total_boxes, bps)
        cost = cdiv(units * s_eff, per_round) * (bps + overhead)
        if cost < best_cost - 1e-9:
            best_cost, best_s = cost, s_eff
    bps = cdiv(total_boxes, best_s)
    return cdiv(total_boxes, bps), bps


class Plan(collections.namedtuple("Plan", "B cin cout N H W groups T bw Hb Wb CiP CoP Q tiles_co tiles_ci nbh nbw nboxes splits bps "
                                          "nbias wchunks cchunks xh_floats gh_floats")):
    @property
    def cin_g(self):
        return self.cin // self.groups

    @property
    def cout_g(self):
        return self.cout // self.groups

    @property
    def last_range(self):
        """boxes of the last split range"""
        return self.nboxes - (self.splits - 1) * self.bps

    def workspace_bytes(self, prologue):
        """(x^ + g^) * 4 + tail: the partial sums and the bias sums, each rounded up to 16 bytes, and x' where there is a prologue"""
        part = r4(self.splits * self.groups * 54 * self.CoP * self.CiP)
        bias = r4(self.nbias * self.groups * self.CoP)
        xp = self.B * self.cin * self.N * self.H * self.W if prologue else 0
        return (self.xh_floats + self.gh_floats) * 4 + (part + bias + xp) * 4

    def depth(self):
        """c of the rounding tier (test_gpu_wgrad_wino_edges.py derives it): roundings on the longest path of one dw element"""
        return 2 + 4 + 1 + 2 * self.bw * self.bps + 3 + cdiv(self.splits, 4) + 3 + 3

    def bias_depth(self):
        """D of the bias path: 2 (a quad) + 8 (a lane's quads) + 3 (butterfly) + ceil(nbias / 8) + 7 (slices) + 1 (bias_scale)"""
        return 2 + 8 + 3 + cdiv(self.nbias, 8) + 7 + 1


def plan(B, seg_c, cout, N, H, W, groups):
    """ww_plan (csrc/wgrad_wino.hip) restated"""
    cin = sum(seg_c)
    T = N // 4
    bw = 8 if W <= 8 else 16
    Hb, Wb = cdiv(H, 8) * 8, cdiv(W, bw) * bw
    cin_g, cout_g = cin // groups, cout // groups
    tiles_ci, tiles_co = cdiv(cin_g, 32), cdiv(cout_g, 32)
    CiP, CoP = tiles_ci * 32, tiles_co * 32
    Q = B * T
    nbh, nbw = Hb // 8, Wb // bw
    nboxes = Q * nbh * nbw
    splits, bps = choose_splits(nboxes, groups * tiles_co * tiles_ci * 6, 512, 1.0, 256)
    wchunks = cdiv(W, TR_W)
    return Plan(B, cin, cout, N, H, W, groups, T, bw, Hb, Wb, CiP, CoP, Q, tiles_co, tiles_ci, nbh, nbw, nboxes, splits, bps,
                Hb * B * T * wchunks, wchunks, cdiv(cin_g, 64),
                groups * 6 * Q * (Hb + 2) * (Wb + 2) * CiP, groups * 6 * Q * Hb * Wb * CoP)


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def lattice_inputs(seed, B, seg_c, cout, N, H, W, shift=False, scale=None, mask=False):
    """Inputs on which every fp32 operation of the kernel is exact: x integers in [-2, 2] (about four in ten are 0, so that some
    taps see a zero halo neighbour and some do not), g = 24 j with j in {-1, 0, 1}; optional exact prologue parts: an integer
    shift [B, Cin] in {-1, 0, 1}, scale rows of 0.5 / 1 / 2 ("rows": [B, Cin], "row": one [Cin] row), a mask of 0 or 1.25.
    dict(xs=[fp32 per segment], g=, shift=, scale=, mask=); the absent parts are None."""
    gen = torch.Generator().manual_seed(seed)
    cin = sum(seg_c)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen).float()
    xs = [ri(-2, 2, B, c, N, H, W) * (torch.rand(B, c, N, H, W, generator=gen) > 0.25).float() for c in seg_c]
    g = 24.0 * ri(-1, 1, B, cout, N, H, W)
    out = dict(xs=xs, g=g, shift=None, scale=None, mask=None)
    if shift:
        out["shift"] = ri(-1, 1, B, cin)
    if scale is not None:
        rows = 2.0 ** ri(-1, 1, B, cin)
        out["scale"] = rows if scale == "rows" else rows[0].clone()
    if mask:
        out["mask"] = 1.25 * (torch.rand(B, cin, N, H, W, generator=gen) > 0.2).float()
    return out


def prologue64(xs, shift=None, scale=None, mask=None, act=False):
    """x' = act(cat(x) + shift) * scale * mask in fp64 (shift / scale: [B, Cin], [Cin] or None)"""
    u = torch.cat(xs, 1).double()
    rows = lambda r: (r[None].expand(u.shape[0], -1) if r.dim() == 1 else r).double()[:, :, None, None, None]
    if shift is not None:
        u = u + rows(shift)
    if act:
        u = u * torch.sigmoid(u)
    if scale is not None:
        u = u * rows(scale)
    return u if mask is None else u * mask.double()


# ---- the transforms ----------------------------------------------------------------------------------------------------------
def band_tiles(t, halo):
    """[B, C, N, H, W] -> [B, C, T, 6 or 4, H, W]: the bands of every tile of four; with halo one band either side, zero outside"""
    if halo:
        return F.pad(t, (0, 0, 0, 0, 1, 1)).unfold(2, 6, 4).permute(0, 1, 2, 5, 3, 4)
    return t.unfold(2, 4, 4).permute(0, 1, 2, 5, 3, 4)


def transforms64(xp, g, absolute=False):
    """B^T x' [B, Cin, T, 6, H, W] and G' g [B, Cout, T, 6, H, W] in fp64; absolute: |B^T| |x'| and |G'| |g|"""
    bt, g24 = torch.tensor(BT, dtype=F64), torch.tensor(G24, dtype=F64)
    xt, gt = band_tiles(xp.double(), True), band_tiles(g.double(), False)
    if absolute:
        bt, g24, xt, gt = bt.abs(), g24.abs(), xt.abs(), gt.abs()
    return torch.einsum("kj,bctjhw->bctkhw", bt, xt), torch.einsum("kn,botnhw->botkhw", g24, gt) / 24.0


def transforms_f32(xp, g):
    """the same two transforms in numpy.float32 with the kernel's own expressions and constants (ww_transform_kernel)"""
    f = np.float32
    d = band_tiles(xp.float(), True).numpy().astype(f)
    d0, d1, d2, d3, d4, d5 = (d[:, :, :, j] for j in range(6))
    a42, b31, c42, e31 = d4 - f(4) * d2, d3 - f(4) * d1, d4 - d2, d3 - d1
    xh = np.stack([(f(4) * d0 + d4) - f(5) * d2, a42 + b31, a42 - b31, c42 + f(2) * e31, c42 - f(2) * e31,
                   (f(4) * d1 + d5) - f(5) * d3], 3)
    q = band_tiles(g.float(), False).numpy().astype(f)
    g0, g1, g2, g3 = (q[:, :, :, j] for j in range(4))
    c6, c12, c24, c3 = f(1) / f(6), f(1) / f(12), f(1) / f(24), f(1) / f(3)
    s02, s13 = g0 + g2, g1 + g3
    ev, od = g0 * c24 + g2 * c6, g1 * c12 + g3 * c3
    gh = np.stack([f(0.25) * g0, (s02 + s13) * -c6, (s13 - s02) * c6, ev + od, ev - od, g3], 3)
    assert xh.dtype == f and gh.dtype == f
    return xh, gh


def fma32(a, b, c):
    """fma in fp32, emulated: a product of two fp32 numbers is exact in fp64, and so is its sum with an fp32 number of similar
    size; one rounding to fp32"""
    return np.float32(np.float64(a) * np.float64(b) + np.float64(c))


def contraction_safe():
    """The compiler may contract a * b + c of the g^ expressions into fused multiply-adds.  On the lattice (g in {-24, 0, 24}) every
    contracted form of ev, od, ev + od and ev - od gives the same exact integers: all 81 quadruples, every choice of fused product."""
    f = np.float32
    vals = (-24, 0, 24)
    for a in vals:
        for b in vals:
            for da, db in ((24, 6), (12, 3)):           # ev = g0 / 24 + g2 / 6;  od = g1 / 12 + g3 / 3
                fa, fb, ca, cb = f(a), f(b), f(1) / f(da), f(1) / f(db)
                exact = a // da + b // db               # (24 is a multiple of every denominator)
                forms = (fa * ca + fb * cb, fma32(fa, ca, fb * cb), fma32(fb, cb, fa * ca))
                if any(float(v) != exact for v in forms):
                    return False
    return True


def quantum_bits(t):
    """the smallest k <= 12 with t * 2^k integral everywhere"""
    for k in range(13):
        s = t * 2.0 ** k
        if bool((s == s.round()).all()):
            return k
    raise AssertionError("not a dyadic lattice")


def exactness_ok(xp, g, pl):
    """The fp32 transforms of the kernel do not round on (x', g): restated in numpy.float32 they equal the fp64 transforms, under
    every contraction the compiler may choose; and no sum rounds either: every product is a multiple of a power of two q, and the
    sum of the absolute terms behind any dw element (dw_abs64) stays below 2^24 q, so every partial sum, in any order, is an
    fp32 number."""
    xh64, gh64 = transforms64(xp, g)
    xh32, gh32 = transforms_f32(xp, g)
    assert np.array_equal(xh32.astype(np.float64), xh64.numpy()), "B^T x' rounds in fp32"
    assert np.array_equal(gh32.astype(np.float64), gh64.numpy()), "G' g rounds in fp32"
    assert contraction_safe()
    gvals = set(g.unique().tolist())
    assert gvals <= {-24.0, 0.0, 24.0}, gvals                               # (what contraction_safe covers)
    q = 2.0 ** -(quantum_bits(xh64) + quantum_bits(gh64))
    M, _ = dw_abs64(xp, g, pl)
    assert float(M.max()) / q < 2.0 ** 24, f"sum of absolute terms {float(M.max())} at quantum {q}"
    assert float(g.double().abs().sum((0, 2, 3, 4)).max()) < 2.0 ** 24
    return True


# ---- the references ----------------------------------------------------------------------------------------------------------
def dw_ref64(xp, g, groups, bias_scale=1.0):
    """(dw [Cout, Cin/g, 3, 3, 3], dbias [Cout]) in fp64: F.conv3d's autograd on x' (fp64), dbias = bias_scale * sum g"""
    cout, cin_g = g.shape[1], xp.shape[1] // groups
    w = torch.zeros(cout, cin_g, 3, 3, 3, dtype=F64, requires_grad=True)
    with torch.enable_grad():
        F.conv3d(xp.double(), w, padding=1, groups=groups).backward(g.double())
    return w.grad, bias_scale * g.double().sum((0, 2, 3, 4))


def winograd64(xp, g, pl, bias_scale=1.0, fault=None, absolute=False):
    """The kernel's algorithm restated in fp64, stage by stage: the two transforms into the padded channels-last arrays
    x^ [group][k][q][Hb + 2][Wb + 2][CiP] and g^ [group][k][q][Hb][Wb][CoP]; per box of 8 x bw positions and plane k the nine
    (dh, dw) sums; the boxes of each split range added; the splits added, A'^T applied per 64-channel chunk; the bias gradient
    from per-workgroup sums laid out [groups][CoP].  absolute: every matrix and operand replaced by its absolute value (the
    term-magnitude bound M).  fault: one deliberate mistake of FAULTS (see fault_applies) -- the power of the checks.
    (dw [Cout, Cin/g, 3, 3, 3], dbias [Cout])"""
    assert fault is None or fault in FAULTS
    B, cin, N, H, W = xp.shape
    cout, groups, cin_g, cout_g = g.shape[1], pl.groups, pl.cin_g, pl.cout_g
    assert (B, cin, cout, N, H, W) == (pl.B, pl.cin, pl.cout, pl.N, pl.H, pl.W)
    bt, g24, at = torch.tensor(BT, dtype=F64), torch.tensor(G24, dtype=F64), torch.tensor(AT, dtype=F64)
    xt, gt = band_tiles(xp.double(), True), band_tiles(g.double(), False)
    if absolute:
        bt, g24, at, xt, gt = bt.abs(), g24.abs(), at.abs(), xt.abs(), gt.abs()
    if fault == "halo":                     # the band below every tile but the first is taken for outside the image
        xt = xt.clone()
        xt[:, :, 1:, 0] = 0
    xh = torch.einsum("kj,bctjhw->bctkhw", bt, xt)
    gh = torch.einsum("kn,botnhw->botkhw", g24, gt) / 24.0
    xhat = torch.zeros(groups, 6, pl.Q, pl.Hb + 2, pl.Wb + 2, pl.CiP, dtype=F64)
    ghat = torch.zeros(groups, 6, pl.Q, pl.Hb, pl.Wb, pl.CoP, dtype=F64)
    for gi in range(groups):
        xhat[gi, :, :, 1:H + 1, 1:W + 1, :cin_g] = xh[:, gi * cin_g:(gi + 1) * cin_g].permute(3, 0, 2, 4, 5, 1).reshape(6, pl.Q, H, W, cin_g)
        ghat[gi, :, :, :H, :W, :cout_g] = gh[:, gi * cout_g:(gi + 1) * cout_g].permute(3, 0, 2, 4, 5, 1).reshape(6, pl.Q, H, W, cout_g)
    if fault == "column":                   # the last image column of the padded row is written as padding
        xhat[:, :, :, :, W, :] = 0
    if fault == "swap":                     # two channels of a 32-channel tile change places
        if cin_g >= 2:
            xhat[..., [0, 1]] = xhat[..., [1, 0]]
        else:
            ghat[..., [0, 1]] = ghat[..., [1, 0]]
    # per box (q, hb, wb; wb fastest), plane and tap
    part = torch.zeros(groups, pl.nboxes, 6, 9, pl.CoP, pl.CiP, dtype=F64)
    gb = ghat.reshape(groups, 6, pl.Q, pl.nbh, 8, pl.nbw, pl.bw, pl.CoP)
    for dh in range(3):
        for dw in range(3):
            sw = dw - 1 if (fault == "tap" and (dh, dw) == (1, 1)) else dw          # the centre tap reads its left neighbour's column
            xb = xhat[:, :, :, dh:dh + pl.Hb, sw:sw + pl.Wb].reshape(groups, 6, pl.Q, pl.nbh, 8, pl.nbw, pl.bw, pl.CiP)
            part[:, :, :, dh * 3 + dw] = torch.einsum("gkqahbwo,gkqahbwc->gqabkoc", gb, xb).reshape(groups, pl.nboxes, 6, pl.CoP, pl.CiP)
    ws = torch.zeros(pl.splits, groups, 6, 9, pl.CoP, pl.CiP, dtype=F64)
    for s in range(pl.splits):
        b0, b1 = s * pl.bps, min(pl.nboxes, (s + 1) * pl.bps)
        if fault == "lastbox" and s == pl.splits - 1:     # the last range stops one box early
            b1 -= 1
        ws[s] = part[:, b0:b1].sum(1)
    full = torch.einsum("nk,gktoc->gocnt", at, ws.sum(0))                        # [groups][CoP][CiP][dn][tap]
    dwt = torch.zeros(cout, cin_g, 27, dtype=F64)
    for gi in range(groups):
        for cc in range(pl.cchunks):
            if fault == "chunk2" and cc >= 1:             # the reduction handles the first 64 input channels only
                continue
            c0, c1 = cc * 64, min(cin_g, cc * 64 + 64)
            dwt[gi * cout_g:(gi + 1) * cout_g, c0:c1] = full[gi, :cout_g, c0:c1].reshape(cout_g, c1 - c0, 27)
    # the bias gradient: one sum per (b, tile, row, column chunk) and channel of [groups][CoP]
    gp = torch.zeros(B, groups, pl.CoP, pl.T, 4, pl.Hb, pl.wchunks * TR_W, dtype=F64)
    gp[:, :, :cout_g, :, :, :H, :W] = gt.reshape(B, groups, cout_g, pl.T, 4, H, W)
    bias_part = gp.reshape(B, groups, pl.CoP, pl.T, 4, pl.Hb, pl.wchunks, TR_W).sum((4, 7)).permute(0, 3, 4, 5, 1, 2)
    tot = bias_part.reshape(pl.nbias, groups, pl.CoP).sum(0)
    dbias = torch.zeros(cout, dtype=F64)
    for gi in range(groups):
        for cl in range(cout_g):
            i = (gi * pl.CoP if fault == "biasidx" else gi * cout_g) + cl
            if i < cout:
                dbias[i] = abs(bias_scale) * tot[gi, cl] if absolute else bias_scale * tot[gi, cl]
    return dwt.reshape(cout, cin_g, 3, 3, 3), dbias


def dw_abs64(xp, g, pl, bias_scale=1.0):
    """M[co, ci, dn, dh, dw] = sum_k |A'^T[dn][k]| sum_{b, tile, h, w} (|G'| |g|)_k (|B^T| |x'|)_k  and  |bias_scale| sum |g|"""
    return winograd64(xp, g, pl, bias_scale, absolute=True)


def fault_applies(fault, pl):
    """halo: more than one band tile; chunk2: more than 64 input channels per group; biasidx: a group after the first whose
    [CoP] row is not full; swap: two live channels on either side; the others always"""
    return {"halo": pl.T > 1, "chunk2": pl.cin_g > 64, "biasidx": pl.groups > 1 and pl.cout_g < pl.CoP,
            "swap": pl.cin_g >= 2 or pl.cout_g >= 2}.get(fault, True)


# ---- the cases of the GPU module: (B, segments, Cout, N, H, W, groups) --------------------------------------------------------
Case = collections.namedtuple("Case", "name B segc cout N H W groups")
CASES = [
    Case("smallest", 1, (1,), 1, 4, 1, 4, 1),
    Case("box8x8-six-padding-rows", 1, (4,), 4, 4, 2, 8, 1),
    Case("W4-Hb16-two-tiles", 2, (3,), 5, 8, 9, 4, 1),
    Case("four-band-tiles", 1, (8,), 8, 16, 8, 16, 1),
    Case("three-tiles-ragged-W12", 1, (4,), 4, 12, 5, 12, 1),
    Case("W64-one-chunk", 1, (4,), 4, 4, 8, 64, 1),
    Case("W68-two-chunks", 1, (4,), 4, 4, 8, 68, 1),
    Case("cin33-cout33", 1, (33,), 33, 4, 8, 8, 1),
    Case("cin65-ragged-chunk", 1, (65,), 2, 4, 8, 8, 1),
    Case("cin128-full-chunks", 1, (128,), 32, 4, 8, 16, 1),
    Case("groups3-cin8-cout8", 1, (24,), 24, 4, 8, 8, 3),
    Case("groups3-cin40-cout33", 2, (120,), 99, 8, 8, 16, 3),
    Case("segments-5-30-6", 1, (5, 30, 6), 8, 4, 8, 16, 1),
    Case("segments-31-33", 1, (31, 33), 8, 4, 8, 8, 1),
    Case("groups3-segments-10-10-4", 1, (10, 10, 4), 6, 4, 8, 8, 3),
    Case("boxes1", 1, (32,), 32, 4, 8, 16, 1),
    Case("boxes2", 2, (32,), 32, 4, 8, 16, 1),
    Case("boxes3", 3, (32,), 32, 4, 8, 16, 1),
    Case("boxes5", 5, (32,), 32, 4, 8, 16, 1),
    Case("boxes6", 6, (32,), 32, 4, 8, 16, 1),
    Case("boxes7-16-tiles", 7, (128,), 128, 4, 8, 16, 1),
    Case("boxes5-32-tiles", 5, (256,), 128, 4, 8, 16, 1),
    Case("boxes14-16-tiles", 7, (128,), 128, 4, 8, 32, 1),
]
PROLOGUE_CASES = ["box8x8-six-padding-rows", "three-tiles-ragged-W12", "segments-5-30-6", "groups3-cin40-cout33"]
ROUNDING_CASES = ["four-band-tiles", "cin128-full-chunks", "boxes7-16-tiles", "groups3-cin40-cout33", "segments-5-30-6"]
CASE = {c.name: c for c in CASES}


def case_plan(c):
    return plan(c.B, c.segc, c.cout, c.N, c.H, c.W, c.groups)
