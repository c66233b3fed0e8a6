"""References and error bounds of the elementwise kernels of csrc/sampler.hip, shared by tests/test_sampler_refs_host.py (CPU)
and tests/test_gpu_sampler_edges.py (GPU).  Not a test module.

Every kernel is stated three times here.
  * `*_ref64`: the formula in fp64 on the fp32 inputs and the fp32 coefficients (cast, never re-derived in double);
  * `*_terms`: M, the fp64 sum of the absolute values of the formula's terms;
  * `*_restate`: the formula in plain torch fp32, one rounding per operation, in the order the reference evaluates it
    (axpby: one fma per term, as its kernel is written).
A kernel passes when |got - ref64| <= r * 2^-24 * M elementwise, r = the number of fp32 operations of the expression (R below)."""
import math

import torch

U = 2.0 ** -24                       # unit roundoff of fp32

# r per kernel: the fp32 operations of one output element (see each *_terms docstring)
R = {"ddpm": 8, "axpby": lambda n_in: 2 * n_in - 1, "multi_axpby": 3, "add": 1, "x0_start": 6, "x0_noise": 3, "q_sample": 3}


def f32(v):
    """v rounded to fp32, as a 0-dim CPU tensor; float(f32(v)) is that fp32 value exactly."""
    return torch.tensor(v, dtype=torch.float32)


def coefs(*vals):
    return tuple(f32(v) for v in vals)


def _on(k, like):
    return [c.to(like.device) for c in k]


def _d(k, like):
    return [c.double().to(like.device) for c in k]


# ---- inputs ------------------------------------------------------------------------------------------------------------------
PLANTED = (        # element i of vector k (k-th row, cyclically): +-0, 1e-30, +-1e30 and the pairs that put x0 at the clamp's edges
    (2.0, -2.0, 0.8, -0.8, 0.0, -0.0, 1e-30, -1e-30, 1e30, -1e30, 1e30, 1.0, -1.0, 1e-30),
    (2.0, -2.0, 0.0, -0.0, -0.0, 0.0, 1e30, 1e-30, -1e30, 1e-30, 1e30, -1.0, 1.0, -1e30),
    (1e30, -0.0, 1.0, 1e-30, 0.0, -1e30, -1.0, 1e30, 1e-30, 0.0, -1e30, 1e30, -1e-30, 2.0),
    (-1e-30, 1e30, -0.0, 1.0, 1e30, 0.0, -1e30, -2.0, 1e30, -1e30, 1e-30, 0.0, -1.0, 1e30),
)


def make_inputs(n, seed, count=1):
    """`count` CPU fp32 vectors of n elements: standard normal, with PLANTED at the front of each as far as n allows.  With
    DDPM_MID below, x = e = +-2 gives x0 = +-1 exactly and x = +-0.8, e = +-0 rounds to x0 = +-1."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(count):
        v = torch.randn(n, generator=g)
        ext = torch.tensor(PLANTED[k % len(PLANTED)], dtype=torch.float32)
        m = min(n, ext.numel())
        v[:m] = ext[:m]
        out.append(v)
    return out


# DDPM rows (c_recip, c_recipm1, coef1, coef2, sigma).  MID: exact binary c_recip / c_recipm1; LATE: alpha_cumprod = 0.01, where
# x0 = 10 x - 9.95 e lies far outside [-1, 1]; EARLY: alpha_cumprod = 0.9999; LAST: the t = 0 row of a table, sigma = 0.
DDPM_MID = coefs(1.25, 0.75, 0.3, 0.69, 0.11)
DDPM_LATE = coefs(10.0, math.sqrt(99.0), 0.02, 0.975, 0.14)
DDPM_EARLY = coefs(math.sqrt(1 / 0.9999), math.sqrt(1 / 0.9999 - 1), 0.4, 0.6, 0.007)
DDPM_LAST = coefs(math.sqrt(1 / 0.99995), math.sqrt(1 / 0.99995 - 1), 1.0, 0.0, 0.0)
DDPM_ROWS = {"mid": DDPM_MID, "late": DDPM_LATE, "early": DDPM_EARLY, "last": DDPM_LAST}
DDPM_TABLE = (DDPM_LAST, DDPM_EARLY, DDPM_MID, DDPM_MID[:4] + coefs(0.5), DDPM_LATE)       # T = 5, row 0 has sigma = 0

AXPBY_COEFS = coefs(0.5, -50.0, 1e-3, -2.25)                   # mixed signs, 1e-3 .. 50 (DPM-Solver++ 3M mixes such magnitudes)
EMA_DECAY = f32(0.9999)
EMA_COEFS = (EMA_DECAY, f32(1.0) - EMA_DECAY)                  # (decay, float32(1 - decay))
X0_COEFS = [coefs(0.8, 0.6), coefs(0.9999, 0.0141), coefs(0.02, 0.9998)]       # (alpha, sigma)
Q_A = (0.9, 0.5, 0.1, 0.99999, 1e-4, 1.0, 0.0)


# ---- the DDPM step -----------------------------------------------------------------------------------------------------------
def ddpm_restate(x, e, nz, k, clip):
    """fp32, one rounding per operation: x0 = a x - b e; clamp; mean = c1 x0 + c2 x; mean + nz sigma (nz None: + 0 sigma)."""
    a, b, c1, c2, sg = _on(k, x)
    x0 = a * x - b * e
    if clip:
        x0 = x0.clamp(-1.0, 1.0)
    mean = c1 * x0 + c2 * x
    return mean + (torch.zeros_like(x) if nz is None else nz) * sg


def ddpm_ref64(x, e, nz, k, clip):
    a, b, c1, c2, sg = _d(k, x)
    x0 = a * x.double() - b * e.double()
    if clip:
        x0 = x0.clamp(-1.0, 1.0)
    out = c1 * x0 + c2 * x.double()
    return out if nz is None else out + nz.double() * sg


def ddpm_terms(x, e, nz, k):
    """r = 8: mul, mul, sub, mul, mul, add, mul, add.  M = |c1| (|a x| + |b e|) + |c2 x| + |sigma nz|; the clamp moves x0 and
    its fp32 value towards each other or not at all (it is non-expansive), so it adds nothing."""
    a, b, c1, c2, sg = _d(k, x)
    m = c1.abs() * ((a * x.double()).abs() + (b * e.double()).abs()) + (c2 * x.double()).abs()
    return m if nz is None else m + (sg * nz.double()).abs()


# ---- axpby / multi_axpby / add -----------------------------------------------------------------------------------------------
def axpby_restate(vs, k):
    """((c0 v0 + c1 v1) + c2 v2) + c3 v3 in fp32"""
    k = _on(k, vs[0])
    acc = k[0] * vs[0]
    for c, v in zip(k[1:], vs[1:]):
        acc = acc + c * v
    return acc


def fma32(c, v, acc):
    """fma(c, v, acc) of fp32 tensors, correctly rounded, on any device.  The product of two floats is exact in fp64; the fp64
    sum s is rounded once already, and its error e = (acc + c v) - s is exact (TwoSum).  Casting s to fp32 rounds a second
    time, which is wrong only when s is exactly midway between two floats and e != 0: the true value then lies on e's side
    of the midpoint (a midpoint is an fp64 number, so |e| <= ulp64 / 2 can neither reach nor cross another one)."""
    a, p = acc.double(), c.double() * v.double()
    s = a + p
    bb = s - a
    e = (a - (s - bb)) + (p - bb)
    f = s.float()
    d = s - f.double()                                          # exact
    toward = torch.where(d > 0, torch.full_like(f, float("inf")), torch.full_like(f, float("-inf")))
    other = torch.nextafter(f, toward)                          # the float on the other side of s
    tie = (d != 0) & (d == other.double() - s) & torch.isfinite(other)
    return torch.where(tie & (e != 0) & ((e > 0) == (d > 0)), other, f)


def axpby_fused_restate(vs, k):
    """What axpby_kernel computes: acc = c0 v0, then acc = fma(c_k, v_k, acc), one rounding per term."""
    k = _on(k, vs[0])
    acc = k[0] * vs[0]
    for c, v in zip(k[1:], vs[1:]):
        acc = fma32(c, v, acc)
    return acc


def axpby_ref64(vs, k):
    return sum(c * v.double() for c, v in zip(_d(k, vs[0]), vs))


def axpby_terms(vs, k):
    """r = 2 n_in - 1 (n_in products, n_in - 1 sums); M = sum |c_k v_k|.  multi_axpby is n_in = 2: r = 3."""
    return sum((c * v.double()).abs() for c, v in zip(_d(k, vs[0]), vs))


def add_restate(a, b, sign_b):
    return a + f32(sign_b).to(a.device) * b


def add_ref64(a, b, sign_b):
    return a.double() + sign_b * b.double()


def add_terms(a, b):
    """r = 1: the product with sign_b = +-1 is exact, one sum; M = |a| + |b|."""
    return a.double().abs() + b.double().abs()


# ---- x0_from_model -----------------------------------------------------------------------------------------------------------
def x0_restate(x, m, k, is_x_start):
    al, sg = _on(k, x)
    eps = (x - al * m) / sg if is_x_start else m
    return (x - sg * eps) / al


def x0_ref64(x, m, k, is_x_start):
    al, sg = _d(k, x)
    eps = (x.double() - al * m.double()) / sg if is_x_start else m.double()
    return (x.double() - sg * eps) / al


def x0_terms(x, m, k, is_x_start):
    """x_start mode, r = 6 (mul, sub, div, mul, sub, div): the terms of (x - sigma eps) / alpha are |x| / alpha and
    |sigma eps| / alpha with |eps| <= (|x| + |alpha m|) / sigma, so M = (2 |x| + |alpha m|) / alpha.
    noise mode, r = 3 (mul, sub, div): M = (|x| + |sigma m|) / alpha."""
    al, sg = _d(k, x)
    if is_x_start:
        return (2 * x.double().abs() + (al * m.double()).abs()) / al
    return (x.double().abs() + (sg * m.double()).abs()) / al


# ---- q_sample ----------------------------------------------------------------------------------------------------------------
def q_sb(a):
    """(1 - a * a).sqrt() in fp32 (evaluated by torch on the host, where sqrt is correctly rounded): the reference's own value,
    its cancellation near a = 1 included"""
    h = a.cpu()
    return (1.0 - h * h).sqrt().to(a.device)


def q_restate(x0, nz, a):
    """x0, nz [B, n]; a [B] fp32"""
    return a[:, None] * x0 + q_sb(a)[:, None] * nz


def q_ref64(x0, nz, a):
    return a.double()[:, None] * x0.double() + q_sb(a).double()[:, None] * nz.double()


def q_terms(x0, nz, a):
    """r = 3 (mul, mul, add) with sb taken as the fp32 value above; M = |a x0| + |sb nz|."""
    return (a.double()[:, None] * x0.double()).abs() + (q_sb(a).double()[:, None] * nz.double()).abs()


# ---- the frame stack -----------------------------------------------------------------------------------------------------------
def frame_slot_ref(t, T, every):
    """Slot of the frame stack that step t fills, by walking p_sample_loop: slot 0 is x_T + MS, then one slot per kept step
    (t % every == 0) in the order t = T - 1 .. 0.  None: step t keeps no frame."""
    kept = [s for s in reversed(range(T)) if s % every == 0]
    return 1 + kept.index(t) if t in kept else None


def frame_count_ref(T, every):
    return 1 + len([s for s in range(T) if s % every == 0])


# ---- the measure ---------------------------------------------------------------------------------------------------------------
def units(got, ref, terms):
    """max over the elements of |got - ref| / (2^-24 M); an element with M = 0 must be exact"""
    err = (got.double() - ref).abs()
    assert bool(torch.isfinite(err).all()), "a result is NaN or infinite"
    assert bool((err[terms == 0] == 0).all()), "an element whose terms are all zero is not exact"
    live = terms > 0
    return float((err[live] / (U * terms[live])).max()) if bool(live.any()) else 0.0


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


SMALL = (1, 2, 3, 4, 5, 1023, 1024, 1028)
