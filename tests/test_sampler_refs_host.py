"""CPU-only companion of tests/test_gpu_sampler_edges.py: the proof that the bounds of tests/sampler_refs.py are fair.  The
restatement of every kernel stays inside |got - ref64| <= r 2^-24 M on the inputs the GPU tests use (2^20 normal samples and the
planted extremes), a formula that loses a term does not, and the fma statement that holds axpby's bits is checked against
exact arithmetic.  No kernel is launched."""
import math
from fractions import Fraction

import pytest
import torch

from sampler_refs import (AXPBY_COEFS, DDPM_MID, DDPM_ROWS, EMA_COEFS, Q_A, R, SMALL, U, X0_COEFS, add_ref64, add_restate,
                          add_terms, axpby_fused_restate, axpby_ref64, axpby_restate, axpby_terms, coefs, ddpm_ref64,
                          ddpm_restate, ddpm_terms, fma32, frame_count_ref, frame_slot_ref, make_inputs, q_ref64, q_restate,
                          q_sb, q_terms, same_bits, units, x0_ref64, x0_restate, x0_terms)

N_HOST = (1 << 20) + 13


def _report(name, worst, r):
    print(f"restatement {name}: worst {worst:.3f} units of 2^-24 M (bound r = {r})")
    assert worst <= r, (name, worst, r)


@pytest.mark.parametrize("row", sorted(DDPM_ROWS))
@pytest.mark.parametrize("clip", [True, False])
def test_ddpm_restatement_is_inside_its_bound(row, clip):
    k = DDPM_ROWS[row]
    worst = 0.0
    for n in SMALL + (N_HOST,):
        x, e, nz = make_inputs(n, 100 + n % 97, 3)
        for noise in ((nz, None) if float(k[4]) == 0.0 else (nz,)):
            got = ddpm_restate(x, e, noise, k, clip)
            worst = max(worst, units(got, ddpm_ref64(x, e, noise, k, clip), ddpm_terms(x, e, noise, k)))
    _report(f"ddpm[{row}, clip={clip}]", worst, R["ddpm"])


def test_clamp_edges_are_among_the_inputs():
    x, e = make_inputs(64, 1, 2)
    x0 = DDPM_MID[0] * x - DDPM_MID[1] * e
    assert bool((x0 == 1.0).any()) and bool((x0 == -1.0).any())
    assert bool((x0.abs() > 1e29).any()) and bool(((x0 != 0) & (x0.abs() < 1e-29)).any())


@pytest.mark.parametrize("n_in", [1, 2, 3, 4])
def test_axpby_restatement_is_inside_its_bound(n_in):
    worst = fused = 0.0
    for n in SMALL + (N_HOST,):
        vs = make_inputs(n, 200 + n_in, n_in)
        k = AXPBY_COEFS[:n_in]
        worst = max(worst, units(axpby_restate(vs, k), axpby_ref64(vs, k), axpby_terms(vs, k)))
        fused = max(fused, units(axpby_fused_restate(vs, k), axpby_ref64(vs, k), axpby_terms(vs, k)))
    _report(f"axpby[{n_in}]", worst, R["axpby"](n_in))
    _report(f"axpby[{n_in}], fused accumulation", fused, R["axpby"](n_in))


def test_ema_and_add_restatements_are_inside_their_bounds():
    a, b = make_inputs(N_HOST, 300, 2)
    _report("multi_axpby", units(axpby_restate([a, b], EMA_COEFS), axpby_ref64([a, b], EMA_COEFS), axpby_terms([a, b], EMA_COEFS)),
            R["multi_axpby"])
    for s in (1.0, -1.0):
        w = units(add_restate(a, b, s), add_ref64(a, b, s), add_terms(a, b))
        print(f"restatement add[{s:+.0f}]: worst {w:.3f} units (bound r = {R['add']})")
        assert w <= R["add"]              # (one rounding: up to 1/2 ulp of the sum, <= 1 unit of M)


@pytest.mark.parametrize("k", X0_COEFS, ids=lambda k: f"alpha{float(k[0]):.4g}")
@pytest.mark.parametrize("is_x_start", [True, False], ids=["x_start", "noise"])
def test_x0_restatement_is_inside_its_bound(k, is_x_start):
    worst = 0.0
    for n in SMALL + (N_HOST,):
        x, m = make_inputs(n, 400 + n % 89, 2)
        worst = max(worst, units(x0_restate(x, m, k, is_x_start), x0_ref64(x, m, k, is_x_start), x0_terms(x, m, k, is_x_start)))
    _report(f"x0[{'x_start' if is_x_start else 'noise'}, alpha={float(k[0]):.4g}]", worst, R["x0_start" if is_x_start else "x0_noise"])


def test_q_sample_restatement_is_inside_its_bound():
    a = torch.tensor(Q_A, dtype=torch.float32)
    n = N_HOST // 4
    x0, nz = (v.view(len(Q_A), n) for v in make_inputs(len(Q_A) * n, 500, 2))
    _report("q_sample", units(q_restate(x0, nz, a), q_ref64(x0, nz, a), q_terms(x0, nz, a)), R["q_sample"])
    sb = q_sb(a)
    assert float(sb[5]) == 0.0 and float(sb[6]) == 1.0
    # the cancellation the reference carries near a = 1 (and why sb is taken from fp32, not recomputed in double)
    exact = math.sqrt(1.0 - float(a[3]) ** 2)
    assert abs(float(sb[3]) - exact) > 4 * U * exact


def test_a_formula_that_loses_or_moves_a_term_leaves_the_bound():
    """What the bound is for: the step without its c2 x term, with eps and x swapped, an axpby that drops its last input and
    an EMA update with (decay, 1 - decay) exchanged are all far outside."""
    x, e, nz = make_inputs(4096, 7, 3)
    k = DDPM_MID
    ref, m = ddpm_ref64(x, e, nz, k, True), ddpm_terms(x, e, nz, k)
    no_c2 = ddpm_restate(x, e, nz, k[:3] + coefs(0.0) + k[4:], True)
    assert units(no_c2, ref, m) > 1e3 * R["ddpm"]
    assert units(ddpm_restate(e, x, nz, k, True), ref, m) > 1e3 * R["ddpm"]
    vs = [x, e, nz]
    kk = AXPBY_COEFS[:3]
    assert units(axpby_restate(vs[:2], kk[:2]), axpby_ref64(vs, kk), axpby_terms(vs, kk)) > 1e3 * R["axpby"](3)
    assert units(axpby_restate([x, e], EMA_COEFS[::-1]), axpby_ref64([x, e], EMA_COEFS), axpby_terms([x, e], EMA_COEFS)) > 1e3


def test_fused_products_are_inside_the_bound_but_not_the_restatements_bits():
    """A multiply-add contracted into one rounding is more accurate, hence inside the bound, and differs from the
    restatement in a large share of the elements: the bit comparison, not the bound, is what sees a contraction."""
    x, e, nz = make_inputs(1 << 16, 8, 3)
    k = DDPM_MID
    a, b, c1, c2, sg = (c.double() for c in k)
    x0 = (a * x.double() - (b * e).double()).float().clamp(-1.0, 1.0)                   # fma(a, x, -(b e))
    mean = (c1 * x0.double() + (c2 * x).double()).float()                               # fma(c1, x0, c2 x)
    fused = (mean.double() + nz.double() * sg).float()                                  # fma(nz, sigma, mean)
    assert units(fused, ddpm_ref64(x, e, nz, k, True), ddpm_terms(x, e, nz, k)) <= R["ddpm"]
    differs = (fused.view(torch.int32) != ddpm_restate(x, e, nz, k, True).view(torch.int32)).float().mean()
    assert float(differs) > 0.05, float(differs)


@pytest.mark.parametrize("T,every", [(5, 1), (5, 2), (5, 3), (1, 1), (7, 4)])
def test_frame_slot_export_follows_the_loop(T, every):
    from tmdiff_amd._lib import lib
    for t in range(-1, T + 1):
        want = frame_slot_ref(t, T, every) if 0 <= t < T and t % every == 0 else None
        got = lib.tmdiff_ddpm_frame_slot(t, T, every)
        if want is not None:
            assert got == want, (t, T, every, got, want)
            assert 1 <= got < frame_count_ref(T, every)
        elif not 0 <= t < T:
            assert got == -1
    assert lib.tmdiff_ddpm_frame_slot(0, T, 0) == -1


def test_multi_axpby_of_nothing_but_empty_tensors_is_a_no_op():
    from tmdiff_amd import ops
    empty = [tuple(torch.empty(0) for _ in range(3)) for _ in range(2)]
    m = ops.MultiAxpby(empty)
    assert m.n_chunks == 0 and not m.stale(empty)
    m.run(0.9999, 1e-4)
    assert ops.MultiAxpby([]).n_chunks == 0
    assert m.stale(empty + [tuple(torch.ones(3) for _ in range(3))])


def _fma_exact(c, v, acc):
    """fma of three Python floats holding fp32 values, by exact rational arithmetic: the nearer of the two floats around the
    true value, the even one at a true tie"""
    true = Fraction(c) * Fraction(v) + Fraction(acc)
    f = torch.tensor(float(true), dtype=torch.float32)              # a float next to the true value
    cands = [f, torch.nextafter(f, torch.tensor(float("inf"))), torch.nextafter(f, torch.tensor(float("-inf")))]
    best = min(cands, key=lambda t: (abs(Fraction(float(t)) - true), int(t.view(torch.int32)) & 1))
    return float(best)


def test_fma32_is_the_correctly_rounded_fma():
    """Crafted double-rounding cases (acc + c v within 2^-25 of the midpoint above an odd and an even float, from both sides, and
    exactly on it) and 4096 random ones against exact arithmetic."""
    one = 1.0 + 2.0 ** -23
    cases = []
    for acc in (2.0 ** 45 + 2.0 ** 22, 2.0 ** 45, -(2.0 ** 45 + 2.0 ** 22)):
        for c in (2.0 ** 21 * one, 2.0 ** 21, -(2.0 ** 21) * one, -(2.0 ** 21)):
            for v in (1.0 - 2.0 ** -23, 1.0, one):
                cases.append((c, v, acc))
    g = torch.Generator().manual_seed(3)
    r = torch.randn(3, 4096, generator=g)
    cases += [tuple(float(t) for t in r[:, i]) for i in range(4096)]
    c, v, acc = (torch.tensor([k[i] for k in cases], dtype=torch.float32) for i in range(3))
    got = fma32(c, v, acc)
    want = torch.tensor([_fma_exact(*k) for k in cases], dtype=torch.float32)
    assert same_bits(got, want), [k for k, a, b in zip(cases, got.tolist(), want.tolist()) if a != b][:4]
    naive = (acc.double() + c.double() * v.double()).float()
    assert not same_bits(naive[:36], want[:36]), "the crafted cases do not exercise the second rounding"
