"""Host-side references for conv3d_wf (csrc/conv3d_wf.hip): its launch plan restated, the table of edge cases with what each one
reaches, inputs on which its fp32 arithmetic is exact, the term-magnitude bound that proves it, the fp64 reference of every
output, and deliberately wrong variants of that reference.  CPU only; nothing here imports tmdiff_amd.
test_conv3d_wf_refs_host.py proves these helpers, test_gpu_conv3d_wf_edges.py uses them.

The algorithm: F(4, 3) along the bands (six planes k, points 0, +-1, +-2, inf), the nine (dh, dw) taps summed directly:
y = A^T sum_{ci, dh, dw} (G w)[k] . (B^T x')[k], tile = four output bands, x' with one band of halo either side (zero outside
the image, the neighbouring tile's band inside), zero padding in h and w.  The composed-LL mode (ops.conv3d_wf_ll) runs the
same chain on the space-to-depth input with the 3 x 4 x 4 stride-2 kernel  s sum_{P, Q in {0, 1}} w[dn][a - P][b - Q],
s = ll_scale / 2: it equals the convolution followed by  ll_scale / 2 times the sum over every 2 x 2 block.
"""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64
TWO24 = 2.0 ** 24

BT = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
               [0, 4, 0, -5, 0, 1]], dtype=np.float64)
G = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
              [0, 0, 1]], dtype=np.float64)
G24 = np.rint(24 * G)                                     # 24 G is integral
AT = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=np.float64)

SPLITK_TARGET, SPLITK_LONG, SPLITK_FILL = 256, 1700, 384   # wf_ksplit's constants (TMDIFF_SPLITK, TMDIFF_SPLITK_LONG unset)


def cdiv(a, b):
    return -(-a // b)


# ---- the plan --------------------------------------------------------------------------------------------------------------
def wf_pair(N, W):
    return N == 8 and W == 8


def geometry(N, W):
    """(mode, band tiles, tile rows, tile columns) of GeoF: N = 8 -> 2 x 8 x 16, N = 4 -> 1 x 16 x 16; pair mode (N = 8 and
    W = 8): the 16 columns are two images of 8 columns side by side."""
    return ("pair", 2, 8, 16) if wf_pair(N, W) else (("n8", 2, 8, 16) if N == 8 else ("n4", 1, 16, 16))


def wf_form_ok(B, cin, cout, N, H, W, groups=1):
    return (groups in (1, 3) and cin > 0 and cout > 0 and cin % groups == 0 and cout % groups == 0 and (cin // groups) % 2 == 0 and
            (cout // groups) % 32 == 0 and N in (4, 8) and H > 0 and W > 0 and W % 4 == 0)


def wf_tiles(B, cout, N, H, W, groups=1):
    th = 8 if N == 8 else 16
    units = (B + 1) // 2 if wf_pair(N, W) else B * cdiv(W, 16)
    return units * groups * cdiv(H, th) * (cout // groups // 32)


def wf_ksplit(B, cin, cout, N, H, W, groups=1, pairs=False):
    """(split factor, taken from the doubling branch): the smallest divisor of the chunk count that brings the grid to 256
    workgroups, at least two chunks per range (pairs: whole pairs of chunks), and once more by two where that leaves fewer than
    384 workgroups and a range of at least 1700 K-steps (54 per chunk, the composed-LL mode 24)."""
    tiles, nchunks, ksteps = wf_tiles(B, cout, N, H, W, groups), cin // groups // 2, 24 if pairs else 54
    ok = lambda s: s >= 1 and nchunks % s == 0 and nchunks // s >= 2 and not (pairs and (nchunks // s) % 2)
    best = 1
    if tiles < SPLITK_TARGET:
        for s in range(2, nchunks // 2 + 1):
            if not ok(s):
                continue
            best = s
            if tiles * s >= SPLITK_TARGET:
                break
    if tiles * best < SPLITK_FILL and ok(2 * best) and (nchunks // (2 * best)) * ksteps >= SPLITK_LONG:
        return 2 * best, True
    return best, False


def wf_grouped_segs(segs, groups):
    return len(segs) == 3 and groups == 3 and segs[0] == segs[1] == segs[2]


Plan = collections.namedtuple("Plan", "B cin cout N H W groups llm mode TT TH TW tiles_h tiles_w tiles_co chunks tiles split doubled "
                                      "plain grouped_segs prologue_bytes splitk_bytes")


# ---- the cases -------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name B segs cout N H W groups opt rounding")
ACT = dict(act=True, shift=True, scale=True)          # a second output as the network asks for it: [B, Cout] bank rows, SiLU
LIN = dict(act=False, shift=True, scale=True)         # ... without SiLU: exact on the lattice


def _o(**kw):
    """keep_y / res / bias / bias_scale / out_scale: the epilogue; y2: the second output (act, shift, scale); s2d / ll / dwt: the
    quarter outputs; rc: channels of a folded 1x1x1; pro: the prologue (act, shift, scale); drop: in-kernel dropout with xp_out;
    dgrad: mode-3 weights (the case's extents are those of the data-gradient convolution, its weight the forward one's);
    llm: the composed-LL mode (H, W and the channels those of the full-resolution input) with its ll_scale; wstep: lattice step."""
    o = dict(keep_y=True, res=False, bias=True, bias_scale=1.0, out_scale=1.0, y2=None, s2d=False, ll=False, dwt=False, rc=0,
             pro=None, drop=False, dgrad=False, llm=False, ll_scale=0.5, wstep=24.0)
    assert set(kw) <= set(o), kw
    o.update(kw)
    return o


DROP = (1234, 0.2)       # kept values are scaled by 1 / (1 - 0.2f) = 1.25 in fp32, which stays exact

CASES = [
    # ---- N = 8, H in {1, 2, 3, 7, 9}, W in {4, 12, 20, 28, 36}
    Case("h1-w12", 2, (4,), 32, 8, 1, 12, 1, _o(), True),                                    # one row; three quads in the only tile
    Case("h9-w4", 1, (6,), 32, 8, 9, 4, 1, _o(res=True), True),                              # W = 4; ragged second row tile; 3 chunks
    Case("h2-w20", 1, (2,), 32, 8, 2, 20, 1, _o(res=True, bias=False), False),               # a residual without a bias; one chunk
    Case("h3-w28", 2, (4,), 64, 8, 3, 28, 1, _o(bias_scale=0.5), False),                     # a bias without a residual, bias_scale
    Case("h7-w36", 1, (8,), 32, 8, 7, 36, 1, _o(out_scale=0.5, y2=LIN), False),              # three column tiles, the last one quad
    # ---- N = 4, H in {1, 5, 15, 17}
    Case("n4-h1-w4", 1, (2,), 32, 4, 1, 4, 1, _o(), False),
    Case("n4-h5-w12", 2, (6,), 32, 4, 5, 12, 1, _o(res=True, y2=ACT), False),
    Case("n4-h15-w24", 1, (4,), 32, 4, 15, 24, 1, _o(), False),                                 # two quads in the last column tile
    Case("n4-h17-w36", 1, (2,), 32, 4, 17, 36, 1, _o(keep_y=False, res=True, y2=LIN), False),   # ragged second row tile
    # ---- pair mode: H in {1, 3, 8, 9}, B in {1, 2, 3}
    Case("pair-h1-b1", 1, (2,), 32, 8, 1, 8, 1, _o(), False),
    Case("pair-h3-b2", 2, (4,), 32, 8, 3, 8, 1, _o(res=True, y2=ACT), False),                 # the second image's own y2 rows
    Case("pair-h8-b3", 3, (6,), 32, 8, 8, 8, 1, _o(y2=LIN), True),
    Case("pair-h9-b3", 3, (2,), 64, 8, 9, 8, 1, _o(res=True, out_scale=2.0), False),
    Case("pair-grouped", 3, (4, 4, 4), 96, 8, 8, 8, 3, _o(res=True), False),                  # three segments = three groups, in place
    # ---- channels and split-K
    Case("split-2x2", 1, (8,), 32, 8, 8, 16, 1, _o(res=True, y2=ACT), False),                 # two ranges of two chunks
    Case("long-sum-16x16", 1, (128,), 32, 8, 16, 16, 1, _o(res=True), True),                  # 32 ranges of two chunks (see below)
    Case("doubling", 32, (256,), 128, 4, 1, 4, 1, _o(y2=LIN), True),                          # 128 tiles: 2 ranges, doubled to 4 x 32 chunks
    Case("cin256-unsplit", 96, (256,), 128, 4, 1, 4, 1, _o(), True),                          # 384 tiles: one range of 128 chunks
    # ---- the folded 1x1x1
    Case("fold32-n4", 1, (4,), 32, 4, 5, 12, 1, _o(rc=32), False),
    Case("fold96-ragged", 2, (6,), 32, 8, 9, 20, 1, _o(rc=96, y2=ACT, out_scale=0.5), False),
    Case("fold512-split", 1, (8,), 32, 8, 8, 16, 1, _o(rc=512), True),                        # range 0 alone adds it
    # ---- quarter outputs at the smallest legal planes (one chunk: the grid cannot split)
    Case("s2d-h2-w4", 1, (2,), 32, 8, 2, 4, 1, _o(y2=LIN, s2d=True), False),
    Case("s2d-h2-w4-res", 2, (2,), 32, 8, 2, 4, 1, _o(keep_y=False, res=True, y2=ACT, s2d=True), False),
    Case("ll-h2-w12", 2, (2,), 32, 8, 2, 12, 1, _o(keep_y=False, y2=LIN, ll=True), False),
    Case("ll-h2-w12-fold", 1, (2,), 32, 8, 2, 12, 1, _o(keep_y=False, y2=ACT, ll=True, rc=32), False),
    Case("ll-h2-w12-res-s2d", 1, (2,), 32, 8, 2, 12, 1, _o(keep_y=False, res=True, y2=LIN, ll=True, s2d=True), False),
    Case("dwt-h2-w12", 1, (2,), 32, 8, 2, 12, 1, _o(keep_y=False, y2=LIN, dwt=True), False),
    Case("dwt-h2-w12-fold", 2, (2,), 32, 8, 2, 12, 1, _o(keep_y=False, y2=ACT, dwt=True, rc=32), False),
    Case("dwt-multi-tile-res", 2, (2,), 64, 8, 16, 32, 1, _o(keep_y=False, res=True, y2=ACT, dwt=True), False),
    # ---- prologue forms (the prologue pass into the workspace)
    Case("pro-shift", 2, (4,), 32, 8, 3, 12, 1, _o(pro=dict(act=True, shift=True, scale=False)), False),
    Case("pro-scale", 1, (4,), 32, 4, 5, 4, 1, _o(pro=dict(act=False, shift=False, scale=True)), False),
    Case("concat-2seg", 2, (2, 4), 32, 8, 2, 12, 1, _o(res=True), False),                     # two segments, no prologue: a concatenation
    Case("drop-xpout", 2, (4,), 32, 8, 7, 12, 1, _o(pro=dict(act=False, shift=True, scale=False), drop=True), False),
    # ---- data-gradient packing (mode 3): Case.segs / cout are the gradient convolution's (the forward one's Cout / Cin)
    Case("dgrad-n8", 1, (4,), 32, 8, 3, 20, 1, _o(bias=False, dgrad=True), False),
    Case("dgrad-pair-groups3", 3, (12,), 96, 8, 3, 8, 3, _o(bias=False, dgrad=True), False),
    # ---- the composed-LL mode (H, W: the full-resolution input; the kernel sees 4 x the channels at half the extents)
    Case("llm-n8", 2, (2,), 32, 8, 6, 24, 1, _o(llm=True, wstep=48.0), False),
    Case("llm-n4", 1, (3,), 32, 4, 10, 8, 1, _o(llm=True, wstep=48.0, res=True, y2=LIN), False),
    Case("llm-pair-split", 3, (4,), 64, 8, 16, 16, 1, _o(llm=True, ll_scale=1.0, res=True, y2=ACT), False),   # 4 ranges of one chunk pair
    Case("llm-pair-split-half", 2, (4,), 32, 8, 2, 16, 1, _o(llm=True, wstep=48.0, keep_y=False, y2=LIN), False),
]
# "long-sum-16x16" is the shape the doubling branch was first looked for at (Cin/g = 128 on a 16 x 16 x 8 plane, B = 1, Cout = 32):
# its two tiles never reach 256 workgroups, so wf_ksplit ends at the largest divisor (32 ranges of two chunks) and the branch
# cannot be taken -- it needs tiles * s >= 256 with ranges of 32 chunks left.  "doubling" is the smallest grid that takes it.
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)


def kernel_extents(c):
    """(B, Cin, Cout, N, H, W, groups) as the kernel sees them"""
    cin = sum(c.segs)
    return (c.B, 4 * cin, c.cout, c.N, c.H // 2, c.W // 2, c.groups) if c.opt["llm"] else (c.B, cin, c.cout, c.N, c.H, c.W, c.groups)


def case_plan(c):
    """wf_forward's decisions restated for a case"""
    B, cin, cout, N, H, W, groups = kernel_extents(c)
    o = c.opt
    assert wf_form_ok(B, cin, cout, N, H, W, groups), c.name
    mode, TT, TH, TW = geometry(N, W)
    grouped = wf_grouped_segs(c.segs, groups)
    plain = (len(c.segs) == 1 or grouped) and o["pro"] is None and not o["drop"]
    split, doubled = wf_ksplit(B, cin, cout, N, H, W, groups, pairs=o["llm"])
    if o["ll"] or o["dwt"]:
        split, doubled = 1, False                  # (no workspace is lent; none of these cases would split anyway)
    plane = N * H * W
    return Plan(B, cin, cout, N, H, W, groups, o["llm"], mode, TT, TH, TW, cdiv(H, TH), 1 if mode == "pair" else cdiv(W, TW),
                cout // groups // 32, cin // groups // 2, wf_tiles(B, cout, N, H, W, groups), split, doubled, plain,
                plain and len(c.segs) == 3, 0 if plain else 4 * B * cin * plane, 4 * split * B * cout * plane if split > 1 else 0)


def reaches(c):
    """What a launch of the case runs, read from conv3d_wf.hip"""
    p, o = case_plan(c), c.opt
    pair = p.mode == "pair"
    return dict(
        mode=p.mode, llm=p.llm,
        h_below_tile=p.H < p.TH,                                   # every row tile is ragged: rows h >= H carry kOutside
        ragged_last_row_tile=p.tiles_h > 1 and p.H % p.TH != 0,
        last_col_quads=None if pair else ((p.W - 1) % p.TW) // 4 + 1,
        w4=p.W == 4,                                               # the raw box's 4-column left margin is wider than the plane
        col_tiles=p.tiles_w, co_tiles=p.tiles_co,
        pair_odd_batch=pair and p.B % 2 == 1, pair_single=pair and p.B == 1,
        chunks=p.chunks, single_chunk=p.chunks == 1, odd_chunks=p.chunks % 2 == 1,
        split=p.split, doubled=p.doubled, chunks_per_range=p.chunks // p.split,
        fold=o["rc"], fold_in_range0_only=bool(o["rc"]) and p.split > 1,
        prologue_pass=not p.plain, grouped_in_place=p.grouped_segs,
        quarter="dwt" if o["dwt"] else ("ll" if o["ll"] else ("s2d" if o["s2d"] else None)),
        tiles=p.tiles, blocks=p.tiles * p.split)


def outputs_of(c):
    """names of the tensors a launch of the case returns, in the order ops.conv3d_wf / conv3d_wf_ll return them"""
    o = c.opt
    if o["dwt"]:
        return ("y_ll", "lh", "hl", "hh")
    if o["ll"]:
        return ("y2", "y_ll")
    return (("y",) if o["keep_y"] else ()) + (("y2",) if o["y2"] is not None else ())


def silu_outputs(c):
    """... of which these went through SiLU"""
    o = c.opt
    if o["y2"] is None or not o["y2"]["act"]:
        return ()
    return ("y_ll",) if o["dwt"] else ("y2",)


def out_shape(c):
    B, _, cout, N, H, W, _ = kernel_extents(c)
    return (B, cout, N, H, W)


def weight_shape(c):
    """of the weight tensor as PyTorch holds it (dgrad: the FORWARD convolution's [its Cout, its Cin / groups, 3, 3, 3])"""
    cin = sum(c.segs)
    return (cin, c.cout // c.groups, 3, 3, 3) if c.opt["dgrad"] else (c.cout, cin // c.groups, 3, 3, 3)


def effective_weight(c, w):
    """the weight of the convolution the launch computes: w itself, or (dgrad) the forward weight transposed inside every group
    with every tap mirrored"""
    if not c.opt["dgrad"]:
        return w
    g = c.groups
    cf_out, cf_in = w.shape[0] // g, w.shape[1]
    v = w.reshape(g, cf_out, cf_in, 3, 3, 3).transpose(1, 2).flip(3, 4, 5)
    return v.reshape(g * cf_in, cf_out, 3, 3, 3).contiguous()


def step_of(c, name):
    """the lattice step of an output: products of integers and multiples of wstep, times out_scale; the 2 x 2 outputs a quarter"""
    o = c.opt
    s = o["wstep"] * o["out_scale"]
    if o["llm"]:
        return s * o["ll_scale"] * 0.5
    return s * 0.25 if name in ("y_ll", "lh", "hl", "hh") else s


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def _parts(c, t, draw):
    o = c.opt
    B, cin_k, cout, N, H, W, _ = kernel_extents(c)
    cin = sum(c.segs)
    t["bias"] = draw["bias"](cout) if o["bias"] else None
    t["res"] = draw["res"](*out_shape(c)) if o["res"] else None
    pro, y2 = o["pro"] or {}, o["y2"] or {}
    t["sh"] = draw["shift"](B, cin) if pro.get("shift") else None
    t["sc"] = draw["scale"](B, cin) if pro.get("scale") else None
    t["sh2"] = draw["shift2"](B, cout) if y2.get("shift") else None
    t["sc2"] = draw["scale2"](B, cout) if y2.get("scale") else None
    t["rc_x"], t["rc_w"] = (draw["rc_x"](B, o["rc"], N, H, W), draw["rc_w"](cout, o["rc"], 1, 1, 1)) if o["rc"] else (None, None)
    return t


def lattice(c, seed=0):
    """Inputs on which no fp32 operation of the kernel rounds (exactness_ok): x integers in [-2, 2] (four in ten zero),
    w = wstep j with j in {-1, 0, 1} (half of them zero; wstep = 24 makes G w integral, 48 in the composed-LL mode at
    ll_scale = 0.5, whose composed weights s sum w are multiples of 12 and whose G (s sum w) has the step 1/2), integer bias /
    residual / shifts, scales 2^-1 .. 2^1, integer rc_x, rc_w = wstep j.  The prologue of the exact tier has no SiLU, whatever
    the case says (pro_act=False); the second output keeps the case's."""
    g = torch.Generator().manual_seed(3000 + seed)
    o = c.opt
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()
    keep = lambda p, *shape: (torch.rand(*shape, generator=g) < p).float()
    shp = (c.N, c.H, c.W)
    t = dict(xs=[ri(-2, 2, c.B, s, *shp) * keep(0.6, c.B, s, *shp) for s in c.segs],
             w=o["wstep"] * ri(-1, 1, *weight_shape(c)) * keep(0.5, *weight_shape(c)), pro_act=False)
    pw2 = lambda *s: 2.0 ** ri(-1, 1, *s)
    return _parts(c, t, dict(bias=lambda *s: ri(-3, 3, *s), res=lambda *s: ri(-4, 4, *s), shift=lambda *s: ri(-1, 1, *s), scale=pw2,
                             shift2=lambda *s: ri(-2, 2, *s), scale2=pw2, rc_x=lambda *s: ri(-2, 2, *s),
                             rc_w=lambda *s: o["wstep"] * ri(-1, 1, *s) * keep(0.5, *s)))


def real(c, seed=0):
    """The rounding tier's inputs: normal data scaled as test_gpu_kernels.py scales its conv3d_wf inputs"""
    g = torch.Generator().manual_seed(4000 + seed)
    o = c.opt
    rn = lambda *shape: torch.randn(*shape, generator=g)
    shp = (c.N, c.H, c.W)
    fan = weight_shape(c)[1] * 27
    t = dict(xs=[rn(c.B, s, *shp) for s in c.segs], w=rn(*weight_shape(c)) / fan ** 0.5, pro_act=bool(o["pro"] and o["pro"]["act"]))
    return _parts(c, t, dict(bias=rn, res=rn, shift=lambda *s: rn(*s) * 0.3, scale=lambda *s: torch.rand(*s, generator=g) + 0.5,
                             shift2=lambda *s: rn(*s) * 0.3, scale2=lambda *s: torch.rand(*s, generator=g) + 0.5, rc_x=rn,
                             rc_w=lambda *s: rn(*s) / s[1] ** 0.5))


# ---- fp64 arithmetic -------------------------------------------------------------------------------------------------------
def _bc(v, C=None):
    return None if v is None else v.to(F64)[:, :C, None, None, None]


def silu64(v):
    return v * torch.sigmoid(v)


def prologue64(t):
    """x' = act(cat(segments) + shift) * scale in fp64 (dropout: the caller multiplies by the kernel's own keep mask)"""
    x = torch.cat(t["xs"], 1).to(F64)
    if t["sh"] is not None:
        x = x + _bc(t["sh"])
    if t["pro_act"]:
        x = silu64(x)
    return x if t["sc"] is None else x * _bc(t["sc"])


def s2d(y2):
    """[B, C, N, H, W] -> [B, 4 C, N, H/2, W/2], channel 4 c + 2 ph + pw"""
    b, c, n, h, w = y2.shape
    v = y2.reshape(b, c, n, h // 2, 2, w // 2, 2)
    return v.permute(0, 1, 4, 6, 2, 3, 5).reshape(b, 4 * c, n, h // 2, w // 2)


CHAIN_MUTATIONS = ("bandhalo", "bandmirror", "clamp_h", "clamp_w")
OTHER_MUTATIONS = ("lastquad", "lastsplit", "pairswap", "foldall", "llblock")
MUTATIONS = CHAIN_MUTATIONS + OTHER_MUTATIONS


def wino_chain(xp, w, groups=1, mutation=None, absolute=False):
    """The six-plane Winograd evaluation of conv3d(xp, w, padding=1, groups) in fp64 numpy, step by step as the kernel lays it
    out: xp [B, C, N, H, W], w [O, C / groups, 3, 3, 3] -> [B, O, N, H, W].  absolute: every matrix and operand replaced by its
    absolute value (the term-magnitude bound); also returns the largest |B^T d|, |G w| and |m|.  mutation: a CHAIN_MUTATION."""
    xp, w = np.asarray(xp, dtype=np.float64), np.asarray(w, dtype=np.float64)
    B, C, N, H, W = xp.shape
    O, T = w.shape[0], N // 4
    bt, g24, at = (np.abs(BT), np.abs(G24), np.abs(AT)) if absolute else (BT, G24, AT)
    if absolute:
        xp, w = np.abs(xp), np.abs(w)
    if mutation == "bandmirror":
        w = w[:, :, ::-1]
    pad = np.zeros((B, C, N + 2, H + 2, W + 2))
    pad[:, :, 1:-1, 1:-1, 1:-1] = xp
    if mutation == "clamp_h":              # the rows above and below the plane hold its first / last row
        pad[:, :, 1:-1, 0, 1:-1], pad[:, :, 1:-1, -1, 1:-1] = xp[:, :, :, 0], xp[:, :, :, -1]
    if mutation == "clamp_w":
        pad[:, :, 1:-1, 1:-1, 0], pad[:, :, 1:-1, 1:-1, -1] = xp[..., 0], xp[..., -1]
    d = np.stack([pad[:, :, 4 * t:4 * t + 6] for t in range(T)], 2)                 # [B, C, T, 6, H + 2, W + 2]
    if mutation == "bandhalo":             # the halo bands that lie in the neighbouring tile read as zero
        d = d.copy()
        d[:, :, :, 0], d[:, :, :, 5] = 0.0, 0.0
    xh = np.einsum("kj,bctjhw->kbcthw", bt, d, optimize=True)
    u = np.einsum("kn,ocnhw->kochw", g24, w, optimize=True) / 24.0                  # (24 G integral: exact on w = 24 j)
    cg, og = C // groups, O // groups
    m = np.zeros((6, B, O, T, H, W))
    for gi in range(groups):
        for dh in range(3):
            for dw in range(3):
                m[:, :, gi * og:(gi + 1) * og] += np.einsum("koc,kbcthw->kbothw", u[:, gi * og:(gi + 1) * og, :, dh, dw],
                                                            xh[:, :, gi * cg:(gi + 1) * cg, :, dh:dh + H, dw:dw + W], optimize=True)
    y = np.einsum("ak,kbothw->botahw", at, m, optimize=True).reshape(B, O, N, H, W)
    return (y, float(np.abs(xh).max()), float(np.abs(u).max()), float(np.abs(m).max())) if absolute else y


def applies(mutation, c):
    """Whether the mistake can show on the case at all"""
    p, o = case_plan(c), c.opt
    return {"bandhalo": c.N == 8, "lastquad": p.mode != "pair", "lastsplit": p.split > 1, "pairswap": p.mode == "pair" and c.B >= 2,
            "foldall": bool(o["rc"]) and p.split > 1, "llblock": (o["ll"] or o["dwt"] or o["llm"]) and c.H >= 4}.get(mutation, True)


def _ll_blocks(v, mutation):
    if mutation == "llblock":              # the block one row further down (the last one wraps)
        v = torch.roll(v, -1, dims=-2)
    return v[..., 0::2, 0::2], v[..., 0::2, 1::2], v[..., 1::2, 0::2], v[..., 1::2, 1::2]


def conv64(c, t, xp, mutation=None, cout=None, chain=False):
    """the convolution itself (the composed-LL mode: with its LL band), [B, O, N, H, W] of the kernel's output extents"""
    p, o = case_plan(c), c.opt
    w = effective_weight(c, t["w"].to(F64))
    if cout is not None:
        assert c.groups == 1
        w = w[:cout]
    if mutation == "lastsplit":            # the channels of the last range never summed
        per = (xp.shape[1] // c.groups) // p.split
        xp = xp.clone()
        for gi in range(c.groups):
            xp[:, (gi + 1) * (xp.shape[1] // c.groups) - per:(gi + 1) * (xp.shape[1] // c.groups)] = 0
    if chain or mutation in CHAIN_MUTATIONS:
        conv = torch.from_numpy(wino_chain(xp.numpy(), w.numpy(), c.groups, mutation if mutation in CHAIN_MUTATIONS else None))
    else:
        conv = F.conv3d(xp, w, None, padding=1, groups=c.groups)
    if o["llm"]:
        a, b, c_, d = _ll_blocks(conv, mutation)
        conv = ((a + b) + (c_ + d)) * (o["ll_scale"] * 0.5)
    if mutation == "lastquad":
        conv = conv.clone()
        conv[..., -4:] = 0
    if mutation == "pairswap":
        conv = conv.clone()
        for b0 in range(0, c.B - 1, 2):
            conv[[b0, b0 + 1]] = conv[[b0 + 1, b0]]
    return conv


def epilogue64(c, t, conv, mutation=None):
    """Every output of the case from the fp64 convolution `conv` (O <= Cout: the first O channels):
    v = (conv + W1 rc_x + bias * bias_scale [* 2 ll_scale in the composed-LL mode] + res) * out_scale;
    y2 = act(v + sh2) * sc2, plain or space-to-depth;  y_ll = LL(v) / 2;  the Haar form: y_ll = act(LL(v) / 2 + sh2) * sc2, lh, hl, hh."""
    o, O = c.opt, conv.shape[1]
    v = conv
    if o["rc"]:
        fold = torch.einsum("oc,bcnhw->bonhw", t["rc_w"].to(F64).reshape(c.cout, -1)[:O], t["rc_x"].to(F64))
        v = v + fold * (case_plan(c).split if mutation == "foldall" else 1)
    if t["bias"] is not None:
        v = v + (t["bias"].to(F64)[:O] * (o["bias_scale"] * (2.0 * o["ll_scale"] if o["llm"] else 1.0)))[None, :, None, None, None]
    if t["res"] is not None:
        v = v + t["res"].to(F64)[:, :O]
    v = v * o["out_scale"]
    out = {}
    sh2, sc2 = _bc(t["sh2"], O), _bc(t["sc2"], O)

    def second(val):
        val = val if sh2 is None else val + sh2
        val = silu64(val) if o["y2"]["act"] else val
        return val if sc2 is None else val * sc2

    if o["keep_y"]:
        out["y"] = v
    if o["y2"] is not None and not o["dwt"]:
        y2 = second(v)
        out["y2"] = s2d(y2) if o["s2d"] else y2
    if o["ll"] or o["dwt"]:
        a, b, c_, d = _ll_blocks(v, mutation)
        ll = ((a + b) + (c_ + d)) * 0.25
        if o["dwt"]:
            out.update(y_ll=second(ll), lh=((a - b) + (c_ - d)) * 0.5, hl=((a + b) - (c_ + d)) * 0.5, hh=((a - b) - (c_ - d)) * 0.5)
        else:
            out["y_ll"] = ll
    return out


def reference(c, t, mutation=None, cout=None, chain=False, xp=None):
    """{name: fp64 tensor} of every output the case asks for.  Without a mutation: torch.nn.functional.conv3d in double, then
    the epilogue (chain=True: the Winograd chain instead).  With one: the wrong variant.  cout: the first so many output
    channels only.  xp: the prologue output to use instead of prologue64(t) (dropout: the kernel's own x')."""
    assert mutation is None or (mutation in MUTATIONS and applies(mutation, c)), mutation
    xp = prologue64(t) if xp is None else xp.to(F64)
    return epilogue64(c, t, conv64(c, t, xp, mutation, cout, chain), mutation)


def exactness_ok(c, t, xp=None):
    """(ok, worst ratio): no fp32 operation of the launch rounds on these inputs.  Every value the kernel forms is a multiple of a
    unit u (a power of two) and is bounded by the absolute-value chain M, in which every matrix and operand is replaced by its
    absolute value -- so is every partial sum in any order: the K = 9 Cin/g products of a plane whatever the chunk and the split
    range they fall in, the sum of the ranges in the reduction kernel, the A^T row sums (at most 1 + 1 + 8 + 8 + 1 times a plane),
    the fold's rc_cin products, the 2 x 2 sums of the LL / Haar outputs.  A value with |v| <= M and M / u <= 2^24 is an fp32
    number.  Scaling by a power of two changes neither side; an addition takes the smaller unit and the sum of the bounds.
    The composed-LL mode multiplies G (s sum_{P, Q} w) by B^T X on the space-to-depth tensor: term by term at most s times the
    sum over the 2 x 2 block of the plain chain's bound, in units of s wstep / 24 (1/2 at ll_scale = 0.5 and wstep = 48)."""
    o = c.opt
    assert not t["pro_act"], "SiLU in the prologue is not exact"
    xp = prologue64(t) if xp is None else xp.to(F64)
    ux = 1.0 if t["sc"] is None else min(1.0, float(t["sc"].abs().min()))
    if o["drop"]:
        ux *= 0.125                        # 1.25 = 10 / 8
    w = effective_weight(c, t["w"].to(F64))
    if not bool((w / o["wstep"] == torch.round(w / o["wstep"])).all()) or not bool((xp / ux == torch.round(xp / ux)).all()):
        return False, float("inf")
    m, xh_max, u_max, m_max = wino_chain(xp.numpy(), w.numpy(), c.groups, absolute=True)
    m, u = torch.from_numpy(m), ux * min(1.0, o["wstep"] / 24.0)
    worst = max(xh_max / ux, u_max / min(1.0, o["wstep"] / 24.0), m_max / u)
    if o["llm"]:
        s = o["ll_scale"] * 0.5
        m = (m[..., 0::2, 0::2] + m[..., 0::2, 1::2] + m[..., 1::2, 0::2] + m[..., 1::2, 1::2]) * s
        u = ux * min(1.0, s * o["wstep"] / 24.0)
        worst = max(worst, 4 * s * u_max / min(1.0, s * o["wstep"] / 24.0), 4 * s * m_max / u)
    if o["rc"]:
        m = m + torch.einsum("oc,bcnhw->bonhw", t["rc_w"].to(F64).abs().reshape(c.cout, -1), t["rc_x"].to(F64).abs())
    if t["bias"] is not None:
        bs = o["bias_scale"] * (2.0 * o["ll_scale"] if o["llm"] else 1.0)
        m, u = m + (t["bias"].to(F64).abs() * bs)[None, :, None, None, None], min(u, bs)
    if t["res"] is not None:
        m = m + t["res"].to(F64).abs()
    m, u = m * o["out_scale"], min(u, 1.0) * o["out_scale"]
    worst = max(worst, float(m.max()) / u)
    sh2 = 0.0 if t["sh2"] is None else _bc(t["sh2"]).abs()
    if o["ll"] or o["dwt"]:
        m4 = m[..., 0::2, 0::2] + m[..., 0::2, 1::2] + m[..., 1::2, 0::2] + m[..., 1::2, 1::2]
        worst = max(worst, float(m4.max()) / u)
        if o["dwt"]:                       # LL' = (ll + sh2) * sc2
            worst = max(worst, float((m4 * 0.25 + sh2).max()) / min(u * 0.25, 1.0))
    if o["y2"] is not None and not o["dwt"]:
        worst = max(worst, float((m + sh2).max()) / min(u, 1.0))
    return worst <= TWO24, worst


def packed_ref(c, w):
    """G w as pack_conv_weight_wino(w, groups, mode 2 [| 1], planes 6) lays it out: [g][ci][dh * 3 + dw][k][co], fp64"""
    we = effective_weight(c, w.to(F64)).numpy()
    g = c.groups
    og, cg = we.shape[0] // g, we.shape[1]
    u = np.einsum("kn,ocnt->ockt", G24, we.reshape(g * og, cg, 3, 9), optimize=True) / 24.0       # [O, cg, k, tap]
    return torch.from_numpy(np.ascontiguousarray(u.reshape(g, og, cg, 6, 9).transpose(0, 2, 4, 3, 1))).reshape(-1)


def packed_ref_wfll(w, ll_scale):
    """pack_conv_weight_wfll: [ci][ph][pw][i * 2 + j][k][co] = G (s sum_{P, Q} w[dn][a - P][b - Q]), a = 1 + 2 i (ph = 0) or 2 i
    (ph = 1), b likewise by (pw, j), s = ll_scale / 2, fp64"""
    w = w.to(F64).numpy()
    cout, cin = w.shape[:2]
    out = np.zeros((cin, 2, 2, 4, 6, cout))
    for ph in range(2):
        for pw in range(2):
            for i in range(2):
                for j in range(2):
                    a4, b4 = (1 + 2 * i if ph == 0 else 2 * i), (1 + 2 * j if pw == 0 else 2 * j)
                    c3 = np.zeros((cout, cin, 3))
                    for P in range(2):
                        for Q in range(2):
                            dh, dw = a4 - P, b4 - Q
                            if 0 <= dh < 3 and 0 <= dw < 3:
                                c3 += w[:, :, :, dh, dw]
                    out[:, ph, pw, i * 2 + j] = np.einsum("kn,ocn->cko", G24, c3 * (ll_scale * 0.5)) / 24.0
    return torch.from_numpy(out).reshape(-1)


@functools.lru_cache(maxsize=None)
def lattice_case(name):
    """(inputs, fp64 reference) of a case's lattice inputs: computed once, shared, never modified (dropout: the reference is
    made by the GPU test from the kernel's own x')"""
    c = CASE[name]
    t = lattice(c)
    return t, (None if c.opt["drop"] else reference(c, t))


@functools.lru_cache(maxsize=None)
def real_case(name):
    c = CASE[name]
    t = real(c)
    return t, reference(c, t)
