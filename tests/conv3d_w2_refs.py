"""Host-side references for conv3d_w2 (csrc/conv3d_w2.hip): its plan restated, the table of edge cases with what each one
reaches, inputs on which its fp32 arithmetic is exact, the term-magnitude bound that proves it, the fp64 reference of every
output, and deliberately wrong variants of that reference.  CPU only; nothing here imports tmdiff_amd.
test_conv3d_w2_refs_host.py proves these helpers, test_gpu_conv3d_w2_edges.py uses them.

The algorithm: F(4, 3) along the bands (six planes kb, points 0, +-1, +-2, inf) times F(2, 3) along the width (four planes kw),
the three row taps dh summed directly:  y = (A^T_band (x) A^T_w) sum_dh sum_ci [ (G_band (x) G_w) w ] . [ (B^T_band (x) B^T_w) x' ],
tile = four output bands x one column pair, x' with one band / one column of zero halo either side.
"""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64
TWO24 = 2.0 ** 24

BT_B = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                 [0, 4, 0, -5, 0, 1]], dtype=np.float64)
BT_W = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
G_B = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
                [0, 0, 1]], dtype=np.float64)
G_W = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=np.float64)
AT_B = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=np.float64)
AT_W = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)

W2_XP, W2_NP, W2_KC, W2_CO = 384, 256, 16, 64      # the kernel's tile constants


def cdiv(a, b):
    return -(-a // b)


# ---- the plan --------------------------------------------------------------------------------------------------------------
class Plan(collections.namedtuple("Plan", "B cin cout N H W T Q TW Hp IP OP G_np G_xp G ptiles last_images nvalid "
                                          "xh_floats mh_floats")):
    @property
    def workspace_bytes(self):
        return (self.xh_floats + self.mh_floats) * 4

    def reaches(self, rc_cin=0):
        """What a launch of this plan runs, read from the kernels: the last GEMM tile (nvalid = its live positions; a wave owns
        positions 64 wv .. 64 wv + 63 in two blocks of 32), the lanes of the passes, the loop counts."""
        nv = self.nvalid
        return dict(
            partial_last_tile=self.last_images < self.G,        # fewer images than G: nvalid < G * OP
            ends_inside_block=nv % 32 != 0,                      # lanes of a live block fall back to position 0, stores go outside
            idle_waves=tuple(wv for wv in range(4) if 64 * wv >= nv),
            every_lane_live=nv == W2_NP,
            dma_past_images=self.G * self.IP < W2_XP,            # the DMA pieces read into the next quad / past the plane
            tw7="live" if self.TW == 8 else ("halo" if self.TW == 7 else "idle"),    # halo: idle, but lane 6's right neighbour
            odd_h=self.H % 2 == 1, stages=self.cin // W2_KC, in_blocks=self.cin // 32, cotiles=self.cout // W2_CO,
            rc_groups=rc_cin // 32, band_tiles=self.T)


def plan(B, cin, cout, N, H, W):
    """w2_plan (csrc/conv3d_w2.hip) restated"""
    T, TW, Hp = N // 4, W // 2, H + 2
    Q, IP, OP = B * T, Hp * TW, H * TW
    g_np, g_xp = W2_NP // OP, W2_XP // IP
    G = min(g_np, g_xp, Q)
    ptiles = cdiv(Q, G)
    last = Q - (ptiles - 1) * G
    return Plan(B, cin, cout, N, H, W, T, Q, TW, Hp, IP, OP, g_np, g_xp, G, ptiles, last, last * OP,
                24 * cin * Q * IP, 24 * cout * Q * OP)


# ---- the cases -------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name B cin cout N H W epi rounding claims")
ROWS = dict(act=True, shift="rows", scale="rows")        # a second output as the network asks for it: [B, Cout] bank rows, SiLU


def _epi(keep_y=True, res=False, y2=None, s2d=False, ll=False, dwt=False, rc=0, bias=True, bias_scale=1.0, out_scale=0.5, pro=None):
    return dict(keep_y=keep_y, res=res, y2=y2, s2d=s2d, ll=ll, dwt=dwt, rc=rc, bias=bias, bias_scale=bias_scale,
                out_scale=out_scale, pro=pro)


CASES = [
    # Q = 6, G = 4: the last tile holds 2 images, nvalid = 120 ends inside a block, waves 2 and 3 idle
    Case("partial-tile", 3, 128, 256, 8, 12, 10, _epi(res=True, y2=ROWS), True,
         dict(partial_last_tile=True, ends_inside_block=True, idle_waves=(2, 3), tw7="idle", band_tiles=2)),
    # Q = 5, G = 2: the last tile holds one image; w2_output_kernel<false, true, true>; a second output with a shift only
    Case("one-image-tail", 5, 128, 256, 4, 16, 16, _epi(keep_y=False, res=True, y2=dict(act=True, shift="rows", scale=None)), False,
         dict(partial_last_tile=True, ends_inside_block=False, idle_waves=(2, 3), tw7="live")),
    # OP = 256: one image per tile, every lane live, B = 1; bias_scale != 1
    Case("full-plane", 1, 128, 256, 4, 32, 16, _epi(bias_scale=0.5, out_scale=1.0), False,
         dict(partial_last_tile=False, every_lane_live=True, tw7="live", dma_past_images=True)),
    # the one-row output pass on an odd number of rows, nvalid = 30 < 32; y2 without SiLU from [C] rows shared over the batch
    Case("odd-rows", 2, 128, 256, 4, 5, 6, _epi(y2=dict(act=False, shift="row", scale="row")), False,
         dict(odd_h=True, ends_inside_block=True, idle_waves=(1, 2, 3))),
    # one column pair, nvalid = 4; a prologue without SiLU from shared [Cin] rows
    Case("min-plane", 1, 128, 256, 4, 4, 2, _epi(pro=dict(act=False, shift="row", scale="row")), False,
         dict(ends_inside_block=True, idle_waves=(1, 2, 3), tw7="idle")),
    # seven column pairs: lane tw == 7 past the plane, the right neighbour of the last pair
    Case("seven-pairs", 1, 128, 256, 4, 6, 14, _epi(res=True), False, dict(tw7="halo", ends_inside_block=True)),
    # ten stages, five 32-channel blocks of the input pass, five channel tiles; a prologue with SiLU on 4 bands
    Case("cin160-cout320", 2, 160, 320, 4, 8, 4, _epi(y2=ROWS, pro=ROWS), True,
         dict(stages=10, in_blocks=5, cotiles=5, band_tiles=1)),
    # the deep layers' channel count; a second output alone (<false, false, true>) with a scale only
    Case("cin256", 1, 256, 256, 8, 8, 8, _epi(keep_y=False, y2=dict(act=True, shift=None, scale="rows")), True, dict(stages=16)),
    # 32 stages, K = 1536; no bias
    Case("cin512", 1, 512, 256, 4, 4, 4, _epi(bias=False), True, dict(stages=32)),
    # the row-pair pass on a partial last tile, three rc groups: the tail of the two-slot prefetch
    Case("rc96-partial", 3, 128, 256, 8, 12, 10, _epi(keep_y=False, y2=ROWS, s2d=True, ll=True, rc=96), False,
         dict(partial_last_tile=True, rc_groups=3)),
    # the maximal fold on one column pair
    Case("rc512-min", 2, 128, 256, 8, 4, 2, _epi(y2=ROWS, rc=512), True, dict(rc_groups=16, tw7="idle", ends_inside_block=True)),
    # a fold on 4 bands
    Case("rc32-4bands", 2, 128, 256, 4, 4, 6, _epi(rc=32), False, dict(rc_groups=1, band_tiles=1)),
    # the row-pair pass at hq = 16, wq = 8: the whole Haar transform, SiLU on LL' only
    Case("dwt-full-plane", 1, 128, 256, 8, 32, 16, _epi(keep_y=False, y2=ROWS, dwt=True, out_scale=1.0), False,
         dict(every_lane_live=True, tw7="live", band_tiles=2)),
    # w2_output2_kernel<RES = true, RC = false> with seven pairs, odd batch
    Case("ll-res-odd-batch", 3, 128, 256, 8, 6, 14, _epi(keep_y=False, res=True, y2=ROWS, ll=True), False,
         dict(tw7="halo", partial_last_tile=False, ends_inside_block=True)),
]
CASE = {c.name: c for c in CASES}


def case_plan(c):
    return plan(c.B, c.cin, c.cout, c.N, c.H, c.W)


def outputs_of(c):
    """names of the tensors a launch of the case returns, in the order ops.conv3d_w2 returns them"""
    e = c.epi
    if e["dwt"]:
        return ("y_ll", "lh", "hl", "hh")
    if e["ll"]:
        return ("y2", "y_ll")
    return (("y",) if e["keep_y"] else ()) + (("y2",) if e["y2"] is not None else ())


def silu_outputs(c):
    """... of which these went through SiLU (compared at the Haar test's 2e-6 / 1e-6 in the exact tier)"""
    e = c.epi
    if e["y2"] is None or not e["y2"]["act"]:
        return ()
    return ("y_ll",) if e["dwt"] else ("y2",)


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def _rows(kind, B, C, draw):
    return None if kind is None else (draw(B, C) if kind == "rows" else draw(C))


def lattice(c, seed=0):
    """Inputs on which no fp32 operation of the three passes rounds (exactness_ok): x integers in [-2, 2] (about half of
    them zero), w = 48 j with j in {-1, 0, 1} (two in three zero: the absolute-value chain has to stay below 2^24 at Cin = 512
    and under the four-element sums of the LL band; packs exactly: test_w2_weight_pack_is_the_kron_of_the_two_g_matrices), integer bias,
    residual and shifts, scales 2^-1 .. 2^1, small-integer rc_x / rc_w.  The prologue of the exact tier has no SiLU, whatever
    the case says (pro_act=False); the second output keeps the case's.  out_scale / bias_scale are the case's powers of two."""
    g = torch.Generator().manual_seed(1000 + seed)
    e = c.epi
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()
    keep = lambda p, *shape: (torch.rand(*shape, generator=g) < p).float()
    t = dict(x=ri(-2, 2, c.B, c.cin, c.N, c.H, c.W) * keep(0.6, c.B, c.cin, c.N, c.H, c.W),
             w=48.0 * ri(-1, 1, c.cout, c.cin, 3, 3, 3) * keep(0.5, c.cout, c.cin, 3, 3, 3), pro_act=False)
    return _epilogue_parts(c, t, bias=lambda: ri(-3, 3, c.cout), res=lambda: ri(-4, 4, c.B, c.cout, c.N, c.H, c.W),
                           shift=lambda *s: ri(-1, 1, *s), scale=lambda *s: 2.0 ** ri(-1, 1, *s),
                           shift2=lambda *s: ri(-2, 2, *s), rc_x=lambda cx: ri(-2, 2, c.B, cx, c.N, c.H, c.W),
                           rc_w=lambda cx: ri(-2, 2, c.cout, cx, 1, 1, 1))


def real(c, seed=0):
    """The rounding tier's inputs: normal data scaled as test_gpu_conv3d_w2.py / _epilogue.py scale theirs"""
    g = torch.Generator().manual_seed(2000 + seed)
    e = c.epi
    rn = lambda *shape: torch.randn(*shape, generator=g)
    t = dict(x=rn(c.B, c.cin, c.N, c.H, c.W), w=rn(c.cout, c.cin, 3, 3, 3) / (27 * c.cin) ** 0.5,
             pro_act=bool(e["pro"] and e["pro"]["act"]))
    return _epilogue_parts(c, t, bias=lambda: rn(c.cout) * 0.3, res=lambda: rn(c.B, c.cout, c.N, c.H, c.W),
                           shift=lambda *s: rn(*s) * 0.2, scale=lambda *s: 1 + 0.1 * rn(*s), shift2=lambda *s: rn(*s) * 0.3,
                           rc_x=lambda cx: rn(c.B, cx, c.N, c.H, c.W), rc_w=lambda cx: rn(c.cout, cx, 1, 1, 1) / cx ** 0.5,
                           scale2=lambda *s: torch.rand(*s, generator=g) + 0.5)


def _epilogue_parts(c, t, bias, res, shift, scale, shift2, rc_x, rc_w, scale2=None):
    e = c.epi
    t["bias"] = bias() if e["bias"] else None
    t["res"] = res() if e["res"] else None
    pro, y2 = e["pro"] or {}, e["y2"] or {}
    t["sh"], t["sc"] = _rows(pro.get("shift"), c.B, c.cin, shift), _rows(pro.get("scale"), c.B, c.cin, scale)
    t["sh2"], t["sc2"] = _rows(y2.get("shift"), c.B, c.cout, shift2), _rows(y2.get("scale"), c.B, c.cout, scale2 or scale)
    t["rc_x"], t["rc_w"] = (rc_x(e["rc"]), rc_w(e["rc"])) if e["rc"] else (None, None)
    return t


# ---- fp64 arithmetic -------------------------------------------------------------------------------------------------------
def _bc(v, C=None):
    """[B, C] rows or one [C] row (shared over the batch) against [B, C, N, H, W]; the first C channels"""
    if v is None:
        return None
    v = v.to(F64)
    v = v[None] if v.dim() == 1 else v
    return v[:, :C, None, None, None]


def silu64(v):
    return v * torch.sigmoid(v)


def prologue64(t):
    """x' = act(x + shift) * scale in fp64"""
    x = t["x"].to(F64)
    if t["sh"] is not None:
        x = x + _bc(t["sh"])
    if t["pro_act"]:
        x = silu64(x)
    return x if t["sc"] is None else x * _bc(t["sc"])


def s2d(y2, transposed=False):
    """[B, C, N, H, W] -> [B, 4 C, N, H/2, W/2], channel 4 co + 2 ph + pw (transposed: 2 pw + ph)"""
    b, c, n, h, w = y2.shape
    v = y2.reshape(b, c, n, h // 2, 2, w // 2, 2)
    v = v.permute(0, 1, 6, 4, 2, 3, 5) if transposed else v.permute(0, 1, 4, 6, 2, 3, 5)
    return v.reshape(b, 4 * c, n, h // 2, w // 2)


def wino_chain(xp, w, mutation=None, absolute=False, band_fill=None):
    """The 24-plane Winograd evaluation of conv3d(xp, w, padding=1) in fp64 numpy, pass by pass as the kernel lays it out:
    xp [B, C, N, H, W], w [O, C, 3, 3, 3] -> [B, O, N, H, W].  absolute: every matrix and operand replaced by its absolute
    value (the term-magnitude bound); also returns the largest |x^| and |m^|.  mutation: one of the chain's MUTATIONS.
    band_fill [B, C]: what the halo bands n = -1 and n = N hold instead of zero."""
    xp, w = np.asarray(xp, dtype=np.float64), np.asarray(w, dtype=np.float64)
    B, C, N, H, W = xp.shape
    O, T, TW = w.shape[0], N // 4, W // 2
    mats = [BT_B, BT_W, G_B, G_W, AT_B, AT_W]
    if absolute:
        mats, xp, w = [np.abs(m) for m in mats], np.abs(xp), np.abs(w)
    btb, btw, gb, gw, atb, atw = mats
    pad = np.zeros((B, C, N + 2, H + 2, W + 2))
    if band_fill is not None:
        pad[:, :, 0, 1:-1, 1:-1] = pad[:, :, -1, 1:-1, 1:-1] = np.asarray(band_fill, dtype=np.float64)[:, :, None, None]
    pad[:, :, 1:-1, 1:-1, 1:-1] = xp
    if mutation == "zerorow_top":          # the padded row above the plane holds the plane's first row
        pad[:, :, 1:-1, 0, 1:-1] = xp[:, :, :, 0]
    if mutation == "zerorow_bottom":
        pad[:, :, 1:-1, -1, 1:-1] = xp[:, :, :, -1]
    d = np.stack([pad[:, :, 4 * t:4 * t + 6] for t in range(T)], 2)                 # [B, C, T, 6, Hp, W + 2]
    d = np.stack([d[..., 2 * tw:2 * tw + 4] for tw in range(TW)], 5)                # [B, C, T, 6, Hp, TW, 4]
    if mutation == "halo":                 # the pair's left halo column taken from the right side and the other way round
        d = d[..., [3, 1, 2, 0]]
    xh = np.einsum("kj,le,bctjhwe->klcbthw", btb, btw, d, optimize=True)            # [6, 4, C, B, T, Hp, TW]
    if mutation == "quadswap":             # the two channel quads of a K-step pair exchanged in x^ and not in U
        xh = xh[:, :, np.arange(C).reshape(-1, 2, 4)[:, ::-1].reshape(-1)]
    # [6, 4, dh, O, C]; the integer matrices 24 G_band and 2 G_w, then one division: exact in fp64 on weights 48 j
    u = np.einsum("kn,lv,ocnhv->klhoc", np.rint(24 * gb), np.rint(2 * gw), w, optimize=True) / 48.0
    if mutation == "kwswap":               # the planes kw = 1 and kw = 2 of U exchanged
        u = u[:, [0, 2, 1, 3]]
    mh = np.zeros((6, 4, O, B * T * H * TW))
    for dh in range(3):
        if mutation == "tap" and dh == 2:  # the last row tap skipped
            continue
        mh += np.matmul(u[:, :, dh], np.ascontiguousarray(xh[..., dh:dh + H, :]).reshape(6, 4, C, -1))
    mh = mh.reshape(6, 4, O, B, T, H, TW)
    if mutation == "lastimage":            # the last image of the last GEMM tile never stored
        mh[:, :, :, -1, -1] = 0.0
    y = np.einsum("ak,el,klobthw->botahwe", atb, atw, mh, optimize=True).reshape(B, O, N, H, W)
    return (y, float(np.abs(xh).max()), float(np.abs(mh).max())) if absolute else y


CHAIN_MUTATIONS = ("lastimage", "halo", "zerorow_top", "zerorow_bottom", "tap", "kwswap", "quadswap", "bandhalo")
EPILOGUE_MUTATIONS = ("rcskip", "rclast2", "s2d_t", "lhhl")
MUTATIONS = CHAIN_MUTATIONS + EPILOGUE_MUTATIONS


def applies(mutation, c):
    """Whether the mistake can show on the case at all"""
    e = c.epi
    return {"halo": c.W >= 4,                                 # (one column pair: both halo columns are the zero padding)
            "bandhalo": e["pro"] is not None and e["pro"]["shift"] is not None,
            "rcskip": e["rc"] > 0, "rclast2": e["rc"] > 0, "s2d_t": e["s2d"], "lhhl": e["dwt"]}.get(mutation, True)


def epilogue64(c, t, conv, mutation=None):
    """Every output of the case from the fp64 convolution `conv` [B, O, N, H, W] (O <= Cout: the first O channels):
    v = (conv + W1 rc_x + bias * bias_scale + res) * out_scale;  y2 = act(v + sh2) * sc2, plain or space-to-depth;
    y_ll = LL(v) / 2;  the Haar form: y_ll = act(LL(v) / 2 + sh2) * sc2, lh, hl, hh."""
    e, O = c.epi, conv.shape[1]
    v = conv
    if e["rc"]:
        groups = list(range(e["rc"] // 32))
        if mutation == "rcskip":
            del groups[1 if len(groups) > 1 else 0]
        if mutation == "rclast2":
            groups.append(groups[-1])
        w1, xr = t["rc_w"].to(F64).reshape(c.cout, -1)[:O], t["rc_x"].to(F64)
        for g in groups:
            v = v + torch.einsum("oc,bcnhw->bonhw", w1[:, 32 * g:32 * g + 32], xr[:, 32 * g:32 * g + 32])
    if t["bias"] is not None:
        v = v + (t["bias"].to(F64)[:O] * e["bias_scale"])[None, :, None, None, None]
    if t["res"] is not None:
        v = v + t["res"].to(F64)[:, :O]
    v = v * e["out_scale"]
    out = {}
    sh2, sc2 = _bc(t["sh2"], O), _bc(t["sc2"], O)

    def second(val):
        val = val if sh2 is None else val + sh2
        val = silu64(val) if e["y2"]["act"] else val
        return val if sc2 is None else val * sc2

    if e["keep_y"]:
        out["y"] = v
    if e["y2"] is not None and not e["dwt"]:
        y2 = second(v)
        out["y2"] = s2d(y2, transposed=mutation == "s2d_t") if e["s2d"] else y2
    if e["ll"] or e["dwt"]:
        a, b, c_, d = v[..., 0::2, 0::2], v[..., 0::2, 1::2], v[..., 1::2, 0::2], v[..., 1::2, 1::2]
        ll = (a + b + c_ + d) * 0.25
        if e["dwt"]:
            lh, hl = ((a - b) + (c_ - d)) * 0.5, ((a + b) - (c_ + d)) * 0.5
            if mutation == "lhhl":
                lh, hl = hl, lh
            out.update(y_ll=second(ll), lh=lh, hl=hl, hh=((a - b) - (c_ - d)) * 0.5)
        else:
            out["y_ll"] = ll
    return out


def reference(c, t, mutation=None, cout=None, chain=False):
    """{name: fp64 tensor} of every output the case asks for.  Without a mutation: torch.nn.functional.conv3d in double, then
    the epilogue (chain=True: the Winograd chain instead, for test_conv3d_w2_refs_host.py).  With one: the wrong variant.
    cout: the first so many output channels only (the host test's mutations do not need all 256)."""
    assert mutation is None or (mutation in MUTATIONS and applies(mutation, c)), mutation
    xp = prologue64(t)
    w = t["w"].to(F64)[:cout]
    if mutation is None and not chain:
        conv = F.conv3d(xp, w, None, padding=1)
    else:
        fill = None
        if mutation == "bandhalo":         # the halo bands went through the prologue: act(0 + shift) * scale
            z = dict(t, x=torch.zeros(c.B, c.cin, 1, 1, 1))
            fill = prologue64(z)[:, :, 0, 0, 0].expand(c.B, c.cin).numpy()
        conv = torch.from_numpy(wino_chain(xp.numpy(), w.numpy(), mutation if mutation in CHAIN_MUTATIONS else None, band_fill=fill))
    return epilogue64(c, t, conv, mutation)


def exactness_ok(c, t):
    """(ok, worst ratio): no fp32 operation of the passes rounds on these inputs.  Every value the kernel forms is a multiple of
    a unit u (a power of two) and is bounded by the absolute-value chain M, in which every matrix and operand is replaced by its
    absolute value -- so is every partial sum, in any order; a value with |v| <= M and M / u <= 2^24 is an fp32 number.  Scaling
    by a power of two changes neither side; an addition takes the smaller unit and the sum of the bounds."""
    e = c.epi
    assert not t["pro_act"], "SiLU in the prologue is not exact"
    xp = prologue64(t)
    ux = 1.0 if t["sc"] is None else min(1.0, float(t["sc"].abs().min()))       # x' = integer * scale; U = integers (w = 48 j)
    w = t["w"].to(F64)
    if not bool((w / 48 == torch.round(w / 48)).all()) or not bool((xp / ux == torch.round(xp / ux)).all()):
        return False, float("inf")
    m, xh_max, mh_max = wino_chain(xp.numpy(), w.numpy(), absolute=True)
    worst = max(xh_max, mh_max) / ux
    m, u = torch.from_numpy(m), ux
    if e["rc"]:
        m = m + torch.einsum("oc,bcnhw->bonhw", t["rc_w"].to(F64).abs().reshape(c.cout, -1), t["rc_x"].to(F64).abs())
    if t["bias"] is not None:
        m, u = m + (t["bias"].to(F64).abs() * e["bias_scale"])[None, :, None, None, None], min(u, e["bias_scale"])
    if t["res"] is not None:
        m = m + t["res"].to(F64).abs()
    m, u = m * e["out_scale"], min(u, 1.0) * e["out_scale"]
    worst = max(worst, float(m.max()) / u)
    m4 = m[..., 0::2, 0::2] + m[..., 0::2, 1::2] + m[..., 1::2, 0::2] + m[..., 1::2, 1::2] if c.H % 2 == 0 else None
    sh2 = 0.0 if t["sh2"] is None else _bc(t["sh2"]).abs()
    if e["dwt"]:                          # the four sums of a 2 x 2 block, halved or quartered; LL' = (ll + sh2) * sc2
        worst = max(worst, float(m4.max()) / u, float((m4 * 0.25 + sh2).max()) / min(u * 0.25, 1.0))
    elif e["y2"] is not None:             # (v + sh2) * sc2: the scale is a power of two
        worst = max(worst, float((m + sh2).max()) / min(u, 1.0))
    if e["ll"]:
        worst = max(worst, float(m4.max()) / u)
    return worst <= TWO24, worst


@functools.lru_cache(maxsize=None)
def lattice_case(name):
    """(inputs, fp64 reference) of a case's lattice inputs: computed once, shared, never modified"""
    c = CASE[name]
    t = lattice(c)
    return t, reference(c, t)


@functools.lru_cache(maxsize=None)
def real_case(name):
    c = CASE[name]
    t = real(c)
    return t, reference(c, t)
