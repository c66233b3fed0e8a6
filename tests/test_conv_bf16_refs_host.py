"""The helpers of conv_bf16_refs.py, proved on the CPU: the exactness of the lattice inputs, what the cases reach in the dispatch
of tmdiff_conv3d_fwd_bf16, bf16 rounding and the unit layout on the host, the fp64 reference against F.conv3d, and the power of
the two tiers of test_gpu_conv_bf16_edges.py.

Power of the checks.  One product x'[ci, pos + tap] * w[co, ci, tap] of MEDIAN magnitude among the 1728 behind a tile-corner
output of the cin_g = 64 case is removed from the reference.  The result still passes assert_close(..., 2e-3, 3e-4), the check
test_conv3d_bf16_operands_fp32_accumulate makes (max|a - b| / max|b| and a relative L2 norm: neither is elementwise); it is not
equal to the reference (exact tier: on lattice inputs the loss of a non-zero term is at least 1/2), and it misses the elementwise
bound (K + E) * 2^-24 * A of the rounding tier by a factor the test prints.
"""
import pytest
import torch
import torch.nn.functional as F

import conv_bf16_refs as R
from conftest import assert_close, rel_err

IDS = [c.name for c in R.CASES]


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_lattice_inputs_are_exact(case):
    assert R.exactness_ok(case)
    assert R.out_elements(case) <= 2 ** 19
    cin_g, cout_g = R.cin_of(case) // case.groups, case.cout // case.groups
    assert cin_g % (8 if case.k == 3 else 16) == 0 and cout_g % 32 == 0 and all(c % 8 == 0 for c in case.segs)
    assert case.groups == 1 or len(case.segs) in (1, case.groups)
    assert case.keep_y or case.emit, "a NULL y needs a second output"
    assert case.emit is None or case.k == 3


def test_cases_reach_every_configuration():
    cfg = {c.name: R.config_of(c) for c in R.CASES}
    k3 = [c for c in R.CASES if c.k == 3]
    k1 = [c for c in R.CASES if c.k == 1]
    tile = lambda c: cfg[c.name][1:5]
    # every launch configuration, with the dwordx4 epilogue on and off (fused and packed-input routes run on every case)
    for t in ((2, 2, 8, 8), (4, 1, 8, 16), (2, 1, 8, 8)):
        for v in (True, False):
            assert any(tile(c) == t and cfg[c.name].vec4 == v for c in k3), (t, v)
    assert {(cfg[c.name].NS, cfg[c.name].MSUB) for c in k1} == {(1, 4), (2, 2), (4, 1)}
    assert all((R.cin_of(c) // c.groups) % 16 == 0 for c in k1)
    # band tiles: N = 1 (three dead waves), 3, 5 (a second workgroup with one live band), 8
    assert {1, 3, 5, 8} <= {c.N for c in k3}
    assert any(c.N == 5 and cfg[c.name].tiles_n == 2 for c in k3)
    # ragged H and W against the tile; partial last column tiles at W = 10 or 20; W % 4 != 0; the W >= 16 boundary and W = 15
    assert any(c.H % cfg[c.name].TH and c.H > cfg[c.name].TH for c in k3) and any(c.H == 1 for c in k3)
    for tw, widths in ((8, (10, 12)), (16, (20,))):
        assert any(cfg[c.name].TW == tw and c.W in widths and cfg[c.name].tiles_w == 2 for c in k3), tw
    assert any(c.W in (7, 9) and not cfg[c.name].vec4 for c in k3) and any(c.W == 1 for c in k3)
    assert any(c.W == 16 and tile(c) == (4, 1, 8, 16) for c in k3) and any(c.W == 15 and tile(c) == (2, 1, 8, 8) for c in k3)
    assert any(c.W == 17 and tile(c) == (4, 1, 8, 16) for c in k3)
    # the vec4 = 0 cases at W % 4 == 0 are the misaligned twins, each beside an aligned case that differs in nothing else
    for c in k3:
        if c.misalign:
            assert c.W % 4 == 0 and not cfg[c.name].vec4 and (c.bias and c.res)
            twin = [t for t in k3 if t._replace(name="", misalign=True) == c._replace(name="")]
            assert len(twin) == 2 and sum(cfg[t.name].vec4 for t in twin) == 1, c.name
    # chunk pipeline: one chunk, two, an odd count, eight; segments on chunk borders; groups; batch; channel tiles
    assert {8, 16, 24, 64} <= {R.cin_of(c) // c.groups for c in k3}
    assert {(8, 16, 8), (8, 8)} <= {c.segs for c in k3}
    assert any(c.groups == 3 and len(c.segs) == 3 for c in k3) and any(c.groups == 3 and len(c.segs) == 1 for c in k3)
    assert any(c.B == 3 for c in k3) and any(cfg[c.name].tiles_co > 1 for c in k3)
    # epilogue: bias without residual, residual without bias, both, neither; scales different from 1
    assert {(c.bias, c.res) for c in k3} == {(False, False), (True, False), (False, True), (True, True)}
    assert {R.scales_of(c) for c in R.CASES} >= {(0.5, 2.0), (0.5, 0.5), (1.0, 2.0), (1.0, 1.0)}
    # second output: every form, with and without y, with and without a residual, both epilogues, a 3-segment input, and cases
    # that can take a producer-packed input
    em = [c for c in k3 if c.emit]
    assert {c.emit for c in em} == {"plain", "affine", "act"}
    assert {(c.keep_y, c.res) for c in em} >= {(True, True), (True, False), (False, True), (False, False)}
    assert {cfg[c.name].vec4 for c in em} == {True, False} and any(len(c.segs) == 3 for c in em)
    assert sum(R.producer_route(c) for c in k3) >= 8 and any(R.producer_route(c) and c.emit for c in k3)
    # 1x1x1: a plane of exactly one workgroup's positions and that plus 1, per configuration; one position; segments; groups
    for ns in (1, 2, 4):
        planes = {c.N * c.H * c.W for c in k1 if cfg[c.name].NS == ns}
        assert {4 * ns * 32, 4 * ns * 32 + 1} <= planes, (ns, planes)
    assert any(c.N * c.H * c.W == 1 for c in k1) and any(len(c.segs) == 3 for c in k1) and any(c.groups == 3 for c in k1)
    assert {c.act for c in k1} == {True, False}
    assert any((R.cin_of(c) // c.groups // 16) % 2 == 1 and R.cin_of(c) // c.groups > 16 for c in k1)     # an odd count of K steps
    for c in R.CASES:
        assert cfg[c.name].workspace_bytes == c.B * R.cin_of(c) * c.N * c.H * c.W * 2
        assert cfg[c.name].blocks >= 1
    for name in R.ROUNDING_CASES + R.SENSOR_CASES + R.REPEAT_CASES:
        assert name in R.CASE
    assert {tile(R.CASE[n]) for n in R.ROUNDING_CASES if R.CASE[n].k == 3} == {(2, 2, 8, 8), (4, 1, 8, 16), (2, 1, 8, 8)}
    assert {cfg[n].NS for n in R.ROUNDING_CASES if R.CASE[n].k == 1} == {1, 2, 4}
    assert all(c.name in R.ROUNDING_CASES for c in R.CASES if c.act)


def test_bf16_helpers_round_to_nearest_even_and_round_trip():
    # 1 + j * 2^-8 lies halfway between two bf16 numbers for odd j: ties go to the even significand
    f = lambda *v: torch.tensor(v, dtype=torch.float32)
    ties = f(1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 256 + 1, 256 + 3)
    want = f(1.0, 1 + 2.0 ** -6, -1.0, -(1 + 2.0 ** -6), 256.0, 260.0)
    assert torch.equal(R.bf16_rne(ties), want)
    near = f(1 + 2.0 ** -8 + 2.0 ** -23, 1 + 2.0 ** -8 - 2.0 ** -23, 0.0, -0.0, 2.0 ** -126, 3.0e38)
    assert torch.equal(R.bf16_rne(near)[:2], f(1 + 2.0 ** -7, 1.0))
    t = torch.randn(4096, generator=torch.Generator().manual_seed(3)) * 10.0 ** torch.arange(-8, 8).repeat(256)
    t = torch.cat([t, ties, near])
    assert torch.equal(R.bf16_rne(t), t.to(torch.bfloat16).float())                  # torch's own conversion (nearest even)
    assert torch.equal(R.bf16_bits(t), t.to(torch.bfloat16).view(torch.int16))
    # every bf16 pattern that is a finite number survives value -> bits
    bits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    finite = (bits.to(torch.int32) & 0x7F80) != 0x7F80
    assert torch.equal(R.bf16_bits(R.bf16_value(bits[finite])), bits[finite])
    # units: channel c of position p sits at [b, c // 8, p, c % 8]
    x = R.bf16_rne(torch.randn(2, 16, 2, 3, 5, generator=torch.Generator().manual_seed(4)))
    u = R.pack_units(x)
    assert u.shape == (2, 2, 30, 8) and u.dtype == torch.int16
    assert torch.equal(R.unpack_units(u, x.shape), x)
    assert float(R.bf16_value(u[1, 1, 1 * 15 + 0 * 5 + 4, 3])) == float(x[1, 11, 1, 0, 4])


@pytest.mark.parametrize("name", ["B-w20-n5-segments", "g3-one-tensor-cout192", "k1-g3-cin48"])
def test_reference_agrees_with_torch_conv3d(name):
    case = R.CASE[name]
    inp = R.real_inputs(case)["normal"]
    xp = R.prologue64(inp)
    got = R.reference(case, inp)
    want = F.conv3d(xp, inp["w"].double(), None, padding=case.k // 2, groups=case.groups)
    m, l2 = rel_err(R.conv64(xp, inp["w"], case.groups), want)
    assert m <= 1e-13 and l2 <= 1e-13, (m, l2)
    if inp["bias"] is not None:
        want = want + (inp["bias"].double() * inp["bias_scale"])[None, :, None, None, None]
    if inp["res"] is not None:
        want = want + inp["res"].double()
    want = want * inp["out_scale"]
    m, l2 = rel_err(got["y"], want)
    assert m <= 1e-13 and l2 <= 1e-13, (m, l2)
    # the prologue in its order: shift, act, scale
    x = torch.cat(inp["xs"], 1).double()
    if inp["shift"] is not None:
        x = x + inp["shift"].double()[:, :, None, None, None]
    if inp["act"]:
        x = F.silu(x)
    if inp["scale"] is not None:
        x = x * inp["scale"].double()[:, :, None, None, None]
    assert rel_err(xp, x)[0] <= 1e-15


def _remove_median_term(case, xq, wq, inp, ref, at):
    """ref with the product of median magnitude behind output `at` = (b, co, n, h, w) removed; the removed amount"""
    b, co, n, h, w = at
    cin_g, cout_g = wq.shape[1], case.cout // case.groups
    g = co // cout_g
    xpad = F.pad(xq.double(), (1, 1, 1, 1, 1, 1))[b, g * cin_g:(g + 1) * cin_g, n:n + 3, h:h + 3, w:w + 3]
    terms = (xpad * wq.double()[co]).reshape(-1)
    live = terms[terms != 0].abs()
    pick = live.sort().values[live.numel() // 2]
    amount = float(terms[(terms.abs() == pick).nonzero()[0, 0]]) * inp["out_scale"]
    out = ref.clone()
    out[at] -= amount
    return out, abs(amount)


def test_one_lost_term_passes_the_old_tolerance_and_fails_both_tiers():
    case = R.CASE["A-cin64-16x16"]
    assert R.cin_of(case) // case.groups == 64
    cfg = R.config_of(case)
    at = (0, 31, R.TN - 1, cfg.TH - 1, cfg.TW - 1)                    # the far corner of the first tile
    # rounding tier: real-valued data
    inp = R.real_inputs(case)["normal"]
    xq, wq = R.bf16_rne(R.prologue64(inp).float()).double(), R.bf16_rne(inp["w"]).double()
    ref = R.reference(case, inp, xq, wq)["y"]
    bnd = R.bound(case, xq, wq, inp)
    lost, amount = _remove_median_term(case, xq, wq, inp, ref, at)
    assert_close(lost.float(), ref.float(), 2e-3, 3e-4, "the check of test_conv3d_bf16_operands_fp32_accumulate")
    m, l2 = rel_err(lost.float(), ref.float())
    ratio = amount / float(bnd[at])
    print(f"one lost term of {amount:.3e}: max-rel {m:.2e} (allowed 2e-3), rel-L2 {l2:.2e} (allowed 3e-4), {ratio:.1f} bounds")
    assert ratio > 1.0 and bool(((lost - ref).abs() > bnd).any())
    assert not torch.equal(lost.float(), ref.float())
    # fp32 rounding of y itself is far inside the bound: the bound is not met by accident
    assert bool(((ref.float().double() - ref).abs() <= bnd).all())
    # exact tier: lattice inputs
    inp = R.lattice_inputs(case)
    xq = R.prologue64(inp)
    ref = R.reference(case, inp)["y"]
    assert torch.equal(ref.float().double(), ref)
    lost, amount = _remove_median_term(case, xq, inp["w"].double(), inp, ref, at)
    assert amount >= 0.5 and not torch.equal(lost.float(), ref.float())


def test_flip_flags_and_second_tolerance():
    # an fp32 number 8 ulps from a tie is flagged, 9 ulps is not; a bf16 number itself is far from every tie
    base = torch.tensor([1 + 2.0 ** -8], dtype=torch.float32).view(torch.int32)
    mk = lambda d: (base + d).view(torch.float32)
    assert bool(R.flip_flags(mk(0))) and bool(R.flip_flags(mk(8))) and bool(R.flip_flags(mk(-8)))
    assert not bool(R.flip_flags(mk(9))) and not bool(R.flip_flags(mk(-9))) and not bool(R.flip_flags(torch.tensor([1.0])))
    # the tolerance of the second output admits the correctly rounded value and refuses a neighbouring bf16 number but one
    case = R.CASE["C-w10-emit-act-scalar"]
    inp = R.real_inputs(case)["normal"]
    y = R.reference(case, inp)["y"].float()
    t = R.second64(y, inp)
    tol = R.second_tolerance(y, inp)
    good = R.bf16_rne(t.float())
    assert bool(((good.double() - t).abs() <= tol).all())
    two_off = R.bf16_value((R.bf16_bits(t.float()).to(torch.int32) + 2).to(torch.int16))
    assert bool(((two_off.double() - t).abs() > tol).all())
