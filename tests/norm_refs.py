"""References, elementwise error bounds, kernel-order emulations and guarded-buffer helpers for csrc/norm_bwd.hip
(layer_norm_bwd, group_norm_bwd, geglu_bwd, col_sum_parts_kernel) and the *_stats forwards of csrc/attention.hip, shared by
tests/test_norm_refs_host.py (CPU) and tests/test_gpu_norm_bwd_edges.py (GPU).  Not a test module.

Every backward is stated twice here.
  * `*_ref`: the formula in fp64 on the float32 inputs the kernel gets, the float32 mean / rstd it is handed included, so a
    backward kernel is judged on its own arithmetic and not on the rounding of the statistics; with it, per element, a bound on
    |kernel - ref| (below), u = 2^-24.
  * `*_emulate`: the kernel's arithmetic in NumPy float32, one rounding per operation, in the kernel's summation order (per
    lane sequential, butterfly over the wave, the waves in index order, the two-stage column sum).  The host test holds it
    below half of every bound, and shows that a dropped term, a skipped row or a lost partial leaves the bound.

The bounds are running-error bounds: a sum of k float32 additions of terms t_i is off by at most k u sum|t_i| (to first
order), a rounded product or difference adds one u each.
  LayerNorm, g = dy gamma, xhat = (x - mean) rstd, A1 = mean_D|g|, A2 = mean_D|g xhat|, NV = ln_nv(D) columns per lane:
      |dx - ref|     <= u rstd (NV + 18) (|g| + A1 + |xhat| A2)      (NV adds + 6 shuffle levels per row sum; 12 for xhat,
                                                                      the products, 1 / D and the three-term epilogue)
      |dgamma - ref| <= u (k + 4) sum_rows|dy xhat|,   |dbeta - ref| <= u (k + 1) sum_rows|dy|
      k = ceil(rpb / 4) + 3 + ceil(blocks / 8) + 7     (rows of a wave, 4 waves, a segment of partials, 8 segments)
  GroupNorm, t = gamma dy, n = cpg P, A1 = sum|t| / n, A2 = sum|t xhat| / n, k = ceil(P / 256) + 9 + cpg:
      |dx - ref|     <= u rstd (k + 12) (|t| + A1 + |xhat| A2)
      dgamma / dbeta as for LayerNorm with depth k + ceil(B / 8) + 7 over sum_{b,p}|dy xhat| and sum_{b,p}|dy|
  GEGLU / GELU, t the gate, a the linear half (1 for gelu_only), phi the normal density: absolute units
      da: u |dy| |t|        dgate: u |dy| |a| (1 + |t| phi(t))
    and a budget of GEGLU_R units, measured (not derived: it is erff / expf that decide): 4 x the worst error of torch's
    float32 evaluation on the CPU in the same units on the inputs of geglu_inputs (the margin of test_gpu_norm_bwd.py).
  Statistics, d the depth of the forward's sums (LayerNorm ceil(D / 64) + 6, GroupNorm ceil(n / 256) + 9), against the fp64
  statistics of the float32 input:
      |mean - ref| <= u (d + 2) mean|x|   =: dm
      |rstd - ref| / ref <= u (d + 6) + dm^2 / (2 (var + eps))
    The second term of the rstd bound is the two-pass variance's own: taken about a mean that is off by e, it is var + e^2
    exactly.  For x = 0.3 + 1.5 randn it is below 1e-4 u; for x = 100 + 0.01 randn (e up to 1e-4, var = 1e-4) it is the bound.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
LN_EPS, GN_EPS = 1e-5, 1e-6

# the budget of the GEGLU / GELU backward in the units above, per gradient: 4 x the float32-CPU ratio, rounded up to 0.5.
# Measured (torch CPU, the inputs of GEGLU_CASES x both modes and geglu_tail_inputs): da 3.877 units (gate 0.31 of (5, 260)),
# dgate 3.472 units (gate -0.049 of (5, 260)): 4 x 3.877 = 15.51 -> 16, 4 x 3.472 = 13.89 -> 14.
GEGLU_CPU_MEASURED = {"da": 3.877, "dgate": 3.472}
GEGLU_R = {"da": 16.0, "dgate": 14.0}

GATES = (-12.0, -6.0, -1e-3, 0.0, 1e-3, 6.0, 12.0, -0.5, 0.5, -3.0, 3.0, -9.5, 9.5)    # the tails of Phi / phi, 0, and between

#            rows  D
LN_D_CASES = ((6, 129), (5, 256),                   # NV = 4, both ends
              (6, 513), (5, 1000), (5, 1024),       # NV = 16, the last instantiation that holds the row in registers
              (5, 1025), (6, 2047),                 # NV = 32, the first that reads the row again; ragged
              (3, 4095))                            # NV = 64, ragged
LN_ROW_CASES = ((4097, 3),                          # rpb = 12, last block of 5 rows
                (6151, 5),                          # rpb = 16, last block of 7 rows
                (9, 33))                            # a second block of one row: three idle waves
LN_HOST_CASES = ((3, 1), (7, 40), (5, 65), (9, 200), (6, 1000), (5, 1025), (4, 2047), (3, 4096), (300, 37))
#            B  C   P    groups
GN_CASES = ((9, 8, 5, 4), (17, 8, 3, 2),            # second stage with per = 2 and 3, an empty segment
            (2, 8, 257, 4), (1, 4, 1000, 2),        # ragged trips of the strided loops
            (2, 12, 33, 1),                         # one group
            (2, 40, 7, 5))                          # cpg = 8; C no multiple of 32 in the column sum
GN_NO_AFFINE = (2, 8, 257, 4)
GEGLU_ALIGN_CASES = ((3, 8), (5, 260))              # inner % 4 == 0: the vector kernel, and the scalar one when misaligned
GEGLU_CASES = GEGLU_ALIGN_CASES + ((7, 6),)         # inner % 4 != 0


def ceil_div(a, b):
    return -(-a // b)


# ---- the launch rules, restated from the comments in norm_bwd.hip ----------------------------------------------------------
def ln_nv(d):
    """columns per lane of layer_norm_bwd_kernel<NV>: the smallest power of two with 64 NV >= D"""
    nv = 1
    while 64 * nv < d:
        nv *= 2
    assert nv <= 64
    return nv


def ln_rpb(rows):
    """rows per workgroup: 8 up to 4096 rows, then as many as keep the grid at 512 blocks, a multiple of 4"""
    rpb = ceil_div(rows, 512)
    return 8 if rpb <= 8 else ceil_div(rpb, 4) * 4


def ln_blocks(rows):
    return ceil_div(rows, ln_rpb(rows))


def ln_param_depth(rows):
    return ceil_div(ln_rpb(rows), 4) + 3 + ceil_div(ln_blocks(rows), 8) + 7


def gn_depth(c, p, groups):
    return ceil_div(p, 256) + 9 + c // groups


def ln_stats_depth(d):
    return ceil_div(d, 64) + 6


def gn_stats_depth(n):
    return ceil_div(n, 256) + 9


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def ln_inputs(rows, d, offset=0.3, scale=1.5):
    """x, gamma, beta, dy (CPU float32)"""
    return (offset + scale * randn(101, rows, d), 1 + 0.1 * randn(103, d), 0.1 * randn(104, d), randn(102, rows, d))


def gn_inputs(b, c, p, affine=True):
    x, dy = 0.3 + 1.5 * randn(105, b, c, p), randn(106, b, c, p)
    return (x, 1 + 0.1 * randn(107, c), 0.1 * randn(108, c), dy) if affine else (x, None, None, dy)


def geglu_inputs(rows, inner, gelu_only):
    """u [rows, inner or 2 inner], dy [rows, inner]; the first gates (row-major) are GATES as far as they fit"""
    u, dy = 1.5 * randn(109, rows, inner if gelu_only else 2 * inner), randn(110, rows, inner)
    gate = u if gelu_only else u[:, inner:]
    for i, v in enumerate(GATES[:rows * inner]):
        gate[i // inner, i % inner] = v
    return u, dy


def geglu_tail_inputs(gelu_only):
    gate = torch.tensor(GATES).repeat(3, 1)
    u = gate if gelu_only else torch.cat([1.5 * randn(111, 3, len(GATES)), gate], dim=1)
    return u.contiguous(), randn(112, 3, len(GATES))


# ---- fp64 references with their bounds ---------------------------------------------------------------------------------------
def ln_stats_ref(x, eps=LN_EPS):
    """{"mean": (ref, bound), "rstd": (ref, bound)} of the rows of x [rows, D], absolute bounds"""
    xd = x.double()
    return _stats_ref(xd, ln_stats_depth(x.shape[-1]), eps)


def gn_stats_ref(x, groups, eps=GN_EPS):
    b, c = x.shape[:2]
    xg = x.double().reshape(b * groups, -1)
    out = _stats_ref(xg, gn_stats_depth(xg.shape[-1]), eps)
    return {k: (r.reshape(b, groups), e.reshape(b, groups)) for k, (r, e) in out.items()}


def _stats_ref(xd, depth, eps):
    eps = float(torch.tensor(eps, dtype=torch.float32))
    mean, var = xd.mean(-1), xd.var(-1, unbiased=False)
    rstd = (var + eps).rsqrt()
    dm = U * (depth + 2) * xd.abs().mean(-1)
    return {"mean": (mean, dm), "rstd": (rstd, rstd * (U * (depth + 6) + dm * dm / (2 * (var + eps))))}


def ln_ref(x, gamma, dy, mean, rstd):
    """{"dx" | "dgamma" | "dbeta": (ref, bound)} in fp64; x, dy [rows, D], gamma [D], mean, rstd [rows] float32"""
    rows, d = x.shape
    mu, rs = mean.double()[:, None], rstd.double()[:, None]
    g, xh = dy.double() * gamma.double(), (x.double() - mu) * rs
    dx = rs * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    bound = U * rs * (ln_nv(d) + 18) * (g.abs() + g.abs().mean(-1, keepdim=True) + xh.abs() * (g * xh).abs().mean(-1, keepdim=True))
    k, p = ln_param_depth(rows), dy.double() * xh
    return {"dx": (dx, bound), "dgamma": (p.sum(0), U * (k + 4) * p.abs().sum(0)),
            "dbeta": (dy.double().sum(0), U * (k + 1) * dy.double().abs().sum(0))}


def gn_ref(x, gamma, dy, mean, rstd, groups):
    """as ln_ref; x, dy [B, C, P], gamma [C] or None, mean, rstd [B, groups] float32"""
    b, c, p = x.shape
    cpg = c // groups
    gm = torch.ones(c, dtype=torch.float64) if gamma is None else gamma.double()
    mu = mean.double().repeat_interleave(cpg, 1)[:, :, None]
    rs = rstd.double().repeat_interleave(cpg, 1)[:, :, None]
    xh, t = (x.double() - mu) * rs, gm[None, :, None] * dy.double()
    grp = lambda v: v.reshape(b, groups, cpg * p).mean(-1).repeat_interleave(cpg, 1)[:, :, None]
    dx = rs * (t - grp(t) - xh * grp(t * xh))
    k = gn_depth(c, p, groups)
    bound = U * rs * (k + 12) * (t.abs() + grp(t.abs()) + xh.abs() * grp((t * xh).abs()))
    k2, pr = k + ceil_div(b, 8) + 7, dy.double() * xh
    return {"dx": (dx, bound), "dgamma": (pr.sum((0, 2)), U * (k2 + 4) * pr.abs().sum((0, 2))),
            "dbeta": (dy.double().sum((0, 2)), U * (k2 + 1) * dy.double().abs().sum((0, 2)))}


def geglu_ref(u, dy, gelu_only):
    """(du in fp64, its unit per element, the mask of the dgate half); du = [da, dgate] or dgate alone"""
    ud, d = u.double(), dy.double()
    a, t = (torch.ones_like(ud), ud) if gelu_only else ud.chunk(2, -1)
    Phi, phi = 0.5 * (1 + torch.erf(t / math.sqrt(2.0))), torch.exp(-0.5 * t * t) / math.sqrt(2 * math.pi)
    dgate, unit_g = d * a * (Phi + t * phi), U * d.abs() * a.abs() * (1 + t.abs() * phi)
    if gelu_only:
        return dgate, unit_g, torch.ones_like(dgate, dtype=torch.bool)
    da, unit_a = d * t * Phi, U * d.abs() * t.abs()
    return torch.cat([da, dgate], -1), torch.cat([unit_a, unit_g], -1), torch.cat([torch.zeros_like(da), torch.ones_like(da)], -1).bool()


def geglu_f32_cpu(u, dy, gelu_only):
    """du of torch's float32 autograd on the CPU: the yardstick GEGLU_R is 4 x of"""
    import torch.nn.functional as F
    leaf = u.clone().requires_grad_()
    out = F.gelu(leaf) if gelu_only else leaf.chunk(2, -1)[0] * F.gelu(leaf.chunk(2, -1)[1])
    out.backward(dy)
    return leaf.grad


def ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound; an element whose bound is 0 must be exact"""
    got = got.detach().cpu().double().reshape(ref.shape)
    err = (got - ref).abs()
    assert bool(torch.isfinite(err).all()), "a result is NaN or infinite"
    assert bool((err[bound == 0] == 0).all()), "an element whose bound is 0 is not exact"
    live = bound > 0
    return float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0


def over(got, ref, bound):
    """the mask of the elements outside their bound"""
    return (torch.as_tensor(got).double().reshape(ref.shape) - ref).abs() > bound


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- the kernels' arithmetic in NumPy float32 -----------------------------------------------------------------------------------
F32 = np.float32
_LANES = np.arange(64)


def _wave_sum(v):
    """tmdiff::wave_sum over the last axis (64 lanes): the xor butterfly, 32 first"""
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _LANES ^ off]
    return v[..., 0]


def _seq_sum(a, axis):
    """s = 0; s += a[i] along `axis`, in index order"""
    a = np.moveaxis(a, axis, 0)
    s = np.zeros(a.shape[1:], F32)
    for i in range(a.shape[0]):
        s = s + a[i]
    return s


def _pad_to(a, axis, n):
    pad = [(0, 0)] * a.ndim
    pad[axis] = (0, n - a.shape[axis])
    return np.pad(a, pad)


def col_sum_emulate(part, drop=None, floor_per=False):
    """col_sum_parts_kernel on part [nparts, cols]: eight contiguous segments of ceil(nparts / 8) partials, each added in
    order, then the eight results in order.  drop: that partial is lost.  floor_per: per = nparts / 8 (a defect)."""
    part = np.array(part, F32)
    n, cols = part.shape
    if drop is not None:
        part[drop] = 0
    per = n // 8 if floor_per else ceil_div(n, 8)
    seg = _seq_sum(_pad_to(part[:min(n, 8 * per)], 0, 8 * per).reshape(8, per, cols), 1)
    t = seg[0]
    for k in range(1, 8):
        t = t + seg[k]
    return t


def ln_stats_emulate(x, eps=LN_EPS, drop=None):
    """layer_norm_kernel's mean and rstd; drop = (row, col): that term is missing from the row's first sum"""
    x = np.asarray(x, F32)
    rows, d = x.shape
    w = ceil_div(d, 64) * 64
    first = x.copy()
    if drop is not None:
        first[drop] = 0
    mean = _wave_sum(_seq_sum(_pad_to(first, 1, w).reshape(rows, -1, 64), 1)) / F32(d)
    dev = x - mean[:, None]
    var = _wave_sum(_seq_sum(_pad_to(dev * dev, 1, w).reshape(rows, -1, 64), 1)) / F32(d) + F32(eps)
    return mean, (1.0 / np.sqrt(var.astype(np.float64))).astype(F32)


def _block_sum(a):
    """a [..., n] -> [...]: threads stride 256 over n, wave_sum, then ((w0 + w1) + w2) + w3"""
    n = a.shape[-1]
    w = ceil_div(n, 256) * 256
    s = _seq_sum(_pad_to(a, a.ndim - 1, w).reshape(a.shape[:-1] + (-1, 256)), a.ndim - 1)
    r = _wave_sum(s.reshape(a.shape[:-1] + (4, 64)))
    return ((r[..., 0] + r[..., 1]) + r[..., 2]) + r[..., 3]


def gn_stats_emulate(x, groups, eps=GN_EPS, drop=None):
    """group_norm_kernel's mean and rstd [B, groups]; drop = (b, group, i)"""
    x = np.asarray(x, F32)
    b = x.shape[0]
    xg = x.reshape(b, groups, -1)
    n = xg.shape[-1]
    first = xg.copy()
    if drop is not None:
        first[drop] = 0
    mean = _block_sum(first) / F32(n)
    dev = xg - mean[..., None]
    var = _block_sum(dev * dev) / F32(n) + F32(eps)
    return mean, (1.0 / np.sqrt(var.astype(np.float64))).astype(F32)


def ln_emulate(x, gamma, dy, mean, rstd, defect=None, where=0):
    """layer_norm_bwd_kernel<NV> + col_sum_parts_kernel: (dx, dgamma, dbeta).  Defects (`where` = the row or partial hit):
    "drop_term": the last column is missing from the row's sum of g; "skip_row": the row is missing from dgamma / dbeta;
    "full_width": the row means are taken over 64 NV instead of D; "no_gamma": the g of the dx expression lacks gamma;
    "drop_partial": the second stage loses that partial"""
    x, gamma, dy, mean, rstd = (np.asarray(v, F32) for v in (x, gamma, dy, mean, rstd))
    rows, d = x.shape
    nv = ln_nv(d)
    w = 64 * nv
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    gs = g.copy()
    if defect == "drop_term":
        gs[where, d - 1] = 0
    s1 = _wave_sum(_seq_sum(_pad_to(gs, 1, w).reshape(rows, nv, 64), 1))
    s2 = _wave_sum(_seq_sum(_pad_to(g * xh, 1, w).reshape(rows, nv, 64), 1))
    inv_d = F32(1) / F32(w if defect == "full_width" else d)
    c1, c2 = s1 * inv_d, s2 * inv_d
    dx = rstd[:, None] * (((dy if defect == "no_gamma" else g) - c1[:, None]) - xh * c2[:, None])
    rpb, blocks = ln_rpb(rows), ln_blocks(rows)
    outs = []
    for a in (dy * xh, dy):
        a = a.copy()
        if defect == "skip_row":
            a[where] = 0
        acc = _seq_sum(_pad_to(a, 0, blocks * rpb).reshape(blocks, rpb // 4, 4, d), 1)      # row r0 + wave + 4 trip
        part = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
        outs.append(col_sum_emulate(part, drop=where if defect == "drop_partial" else None))
    return dx, outs[0], outs[1]


def gn_emulate(x, gamma, dy, mean, rstd, groups, defect=None, where=(0, 0)):
    """group_norm_bwd_kernel + col_sum_parts_kernel: (dx, dgamma, dbeta).  Defects, `where` = (b, channel): "drop_term": the
    last element of the channel is missing from pass 1; "no_gamma": the t of the dx expression lacks gamma; "mean_over_p": the
    group means are taken over P instead of cpg P; "drop_partial": the second stage loses the partial of sample b"""
    x, dy, mean, rstd = (np.asarray(v, F32) for v in (x, dy, mean, rstd))
    b, c, p = x.shape
    cpg = c // groups
    gm = np.ones(c, F32) if gamma is None else np.asarray(gamma, F32)
    mu, rs = np.repeat(mean, cpg, 1)[:, :, None], np.repeat(rstd, cpg, 1)[:, :, None]
    xh = (x - mu) * rs
    d1 = dy.copy()
    if defect == "drop_term":
        d1[where[0], where[1], p - 1] = 0
    s1, s2 = _block_sum(d1), _block_sum(d1 * xh)                                                 # [B, C]
    g1 = _seq_sum((gm * s1).reshape(b, groups, cpg), 2)
    g2 = _seq_sum((gm * s2).reshape(b, groups, cpg), 2)
    inv_n = F32(1) / F32(p if defect == "mean_over_p" else cpg * p)
    m1, m2 = np.repeat(g1 * inv_n, cpg, 1)[:, :, None], np.repeat(g2 * inv_n, cpg, 1)[:, :, None]
    t = dy if defect == "no_gamma" else gm[None, :, None] * dy
    dx = rs * ((t - m1) - xh * m2)
    drop = where[0] if defect == "drop_partial" else None
    return dx, col_sum_emulate(s2, drop=drop), col_sum_emulate(s1, drop=drop)


# ---- guarded device buffers ------------------------------------------------------------------------------------------------------
FRONT, GUARD, SENTINEL = 4, 64, 12345.0


class G:
    """A float32 tensor of `shape` on the GPU inside one allocation: FRONT (+ off) sentinels, the tensor, GUARD sentinels.
    off = 0: 16-byte aligned; off = 1: one float past a 16-byte boundary.  Without values it is filled with NaN (an output)."""

    def __init__(self, shape, values=None, off=0):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = math.prod(shape)
        self.lo = FRONT + off
        self.buf = torch.full((self.lo + n + GUARD,), SENTINEL, device="cuda", dtype=torch.float32)
        self.t = self.buf[self.lo:self.lo + n].view(shape)
        if values is None:
            self.t.fill_(float("nan"))
        else:
            self.t.copy_(values)
        self.before = None if values is None else self.t.clone()
        assert self.t.data_ptr() % 16 == 4 * off and self.t.is_contiguous()

    @property
    def ptr(self):
        return self.t.data_ptr()

    def check(self, what=""):
        n = self.t.numel()
        assert bool((self.buf[:self.lo] == SENTINEL).all()), f"{what}: a store landed in front of the tensor"
        assert bool((self.buf[self.lo + n:] == SENTINEL).all()), f"{what}: a store landed past the end of the tensor"
        if self.before is not None:
            assert same_bits(self.t, self.before), f"{what}: an input changed"


def put(v, off=0):
    return None if v is None else G(v.shape, v, off)
