"""CPU-only companion of tests/test_gpu_norm_bwd_edges.py: the proof that the bounds of tests/norm_refs.py are valid and sharp.
The float32 emulation of every kernel, in the kernel's summation order, stays below half of its bound on every case; the
same emulation with one term dropped from a sum, the last row of a ragged block skipped, the row mean taken over 64 NV, gamma
left out or one partial lost leaves the bound in the affected row, group or column.  The GEGLU budget is re-measured against
torch's float32 on the CPU, and the workspace size of the LayerNorm backward is held to its formula.  No kernel is launched."""
import numpy as np
import pytest
import torch

import norm_refs as N

ids = lambda e: "x".join(map(str, e))
CONDITIONS = ((0.3, 1.5), (100.0, 1.5))
HALF = 0.5


def _np(*ts):
    return [None if t is None else t.numpy() for t in ts]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _ln(rows, d, offset, scale):
    """inputs, the emulated float32 statistics, and the fp64 reference evaluated from them"""
    x, gamma, beta, dy = N.ln_inputs(rows, d, offset, scale)
    mean, rstd = N.ln_stats_emulate(x.numpy())
    return (x, gamma, dy, _t(mean), _t(rstd)), N.ln_ref(x, gamma, dy, _t(mean), _t(rstd))


def _gn(extents, affine=True):
    b, c, p, groups = extents
    x, gamma, beta, dy = N.gn_inputs(b, c, p, affine)
    mean, rstd = N.gn_stats_emulate(x.numpy(), groups)
    return (x, gamma, dy, _t(mean), _t(rstd)), N.gn_ref(x, gamma, dy, _t(mean), _t(rstd), groups)


LN_ALL = tuple(dict.fromkeys(N.LN_HOST_CASES + N.LN_D_CASES + N.LN_ROW_CASES))


# ---- validity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extents", LN_ALL, ids=ids)
def test_layer_norm_emulation_is_below_half_of_every_bound(extents):
    rows, d = extents
    for offset, scale in CONDITIONS + (((100.0, 0.01),) if extents == (5, 1000) else ()):
        x = N.ln_inputs(rows, d, offset, scale)[0]
        stats = N.ln_stats_ref(x)
        for name, got in zip(("mean", "rstd"), N.ln_stats_emulate(x.numpy())):
            r = N.ratio(_t(got), *stats[name])
            print(f"layer_norm {extents} offset {offset} scale {scale} {name}: {r:.3f} of the bound")
            assert r <= HALF, (name, r)
        args, ref = _ln(rows, d, offset, scale)
        for name, got in zip(("dx", "dgamma", "dbeta"), N.ln_emulate(*_np(*args))):
            r = N.ratio(_t(got), *ref[name])
            print(f"layer_norm {extents} offset {offset} scale {scale} {name}: {r:.3f} of the bound")
            assert r <= HALF, (name, r)


@pytest.mark.parametrize("extents", N.GN_CASES, ids=ids)
@pytest.mark.parametrize("affine", (True, False), ids=("affine", "plain"))
def test_group_norm_emulation_is_below_half_of_every_bound(extents, affine):
    groups = extents[3]
    args, ref = _gn(extents, affine)
    stats = N.gn_stats_ref(args[0], groups)
    for name, got in zip(("mean", "rstd"), N.gn_stats_emulate(args[0].numpy(), groups)):
        r = N.ratio(_t(got), *stats[name])
        print(f"group_norm {extents} {name}: {r:.3f} of the bound")
        assert r <= HALF, (name, r)
    for name, got in zip(("dx", "dgamma", "dbeta"), N.gn_emulate(*_np(*args), groups)):
        r = N.ratio(_t(got), *ref[name])
        print(f"group_norm {extents} affine={affine} {name}: {r:.3f} of the bound")
        assert r <= HALF, (name, r)


def test_sequential_parameter_sums_are_inside_the_bound():
    """dgamma / dbeta added row after row in float32 (depth rows, not the two-stage k): still inside the bound of depth k"""
    for rows, d in ((300, 37), (4097, 3)):
        args, ref = _ln(rows, d, 0.3, 1.5)
        x, gamma, dy, mean, rstd = _np(*args)
        xh = (x - mean[:, None]) * rstd[:, None]
        for name, terms in (("dgamma", dy * xh), ("dbeta", dy)):
            s = np.zeros(d, np.float32)
            for r in range(rows):
                s = s + terms[r]
            q = N.ratio(_t(s), *ref[name])
            print(f"layer_norm {rows}x{d} {name}, row after row: {q:.3f} of the bound")
            assert q <= 1.0, (name, q)


# ---- sharpness -----------------------------------------------------------------------------------------------------------------
def _ln_over(extents, defect, where):
    args, ref = _ln(*extents, 0.3, 1.5)
    got = N.ln_emulate(*_np(*args), defect=defect, where=where)
    return {name: N.over(g, *ref[name]) for name, g in zip(("dx", "dgamma", "dbeta"), got)}


@pytest.mark.parametrize("extents", N.LN_HOST_CASES + N.LN_D_CASES, ids=ids)
def test_layer_norm_bound_sees_a_term_dropped_from_a_row_sum(extents):
    row = extents[0] - 1
    out = _ln_over(extents, "drop_term", row)["dx"]
    print(f"layer_norm {extents}: {int(out[row].sum())} of {extents[1]} elements of the row leave the bound")
    assert bool(out[row].any()) and not bool(out[:row].any())


def test_one_dropped_term_of_4096_moves_the_whole_row():
    """the case of the issue: (3, 4096), one term of mean_D(g) lost -> every dx of that row is outside"""
    out = _ln_over((3, 4096), "drop_term", 1)["dx"]
    assert bool(out[1].all()) and not bool(out[0].any()) and not bool(out[2].any())


def _width_defect_is_visible(d):
    """1 / (64 NV) for 1 / D scales both row means by D / (64 NV).  At D = 4095 that is 1 - 2^-12, and the means of a random g
    are about D^-1/2 = 2^-6 of |g|: dx moves by 2^-18 |g|, less than the (NV + 18) u = 2^-17.6 |g| any float32 evaluation is
    allowed.  No elementwise bound can see it there (nor at D = 4096, where the two programs are the same)."""
    w = 64 * N.ln_nv(d)
    return (w - d) / w >= 2.0 ** -11


@pytest.mark.parametrize("extents", [e for e in N.LN_HOST_CASES + N.LN_D_CASES if _width_defect_is_visible(e[1])], ids=ids)
def test_layer_norm_bound_sees_a_mean_over_the_padded_width(extents):
    out = _ln_over(extents, "full_width", None)["dx"]
    assert all(bool(out[r].any()) for r in range(extents[0]))


@pytest.mark.parametrize("extents", N.LN_HOST_CASES + N.LN_D_CASES, ids=ids)
def test_layer_norm_bound_sees_gamma_left_out(extents):
    out = _ln_over(extents, "no_gamma", None)["dx"]
    assert all(bool(out[r].any()) for r in range(extents[0]))


@pytest.mark.parametrize("extents", ((9, 33), (300, 37), (4097, 3), (6151, 5)), ids=ids)
def test_parameter_bounds_see_a_skipped_row_and_a_lost_partial(extents):
    rows, d = extents
    assert rows % N.ln_rpb(rows)                               # the last block is ragged
    out = _ln_over(extents, "skip_row", rows - 1)
    assert bool(out["dgamma"].any()) and bool(out["dbeta"].any()) and not bool(out["dx"].any())
    for which in (0, N.ln_blocks(rows) - 1):
        out = _ln_over(extents, "drop_partial", which)
        assert bool(out["dgamma"].any()) and bool(out["dbeta"].any()), which


def test_column_sum_with_a_floored_segment_length_loses_partials():
    """per = nparts / 8 instead of its ceiling: the last nparts % 8 partials are never added"""
    part = np.arange(1, 9 * 3 + 1, dtype=np.float32).reshape(9, 3)
    assert np.array_equal(N.col_sum_emulate(part), part.sum(0))
    assert np.array_equal(N.col_sum_emulate(part, floor_per=True), part[:8].sum(0))
    assert not N.col_sum_emulate(np.zeros((0, 5), np.float32)).any()


@pytest.mark.parametrize("extents", N.GN_CASES, ids=ids)
def test_group_norm_bounds_see_each_defect(extents):
    b, c, p, groups = extents
    cpg = c // groups
    args, ref = _gn(extents)
    run = lambda defect, where=(0, 0): {name: N.over(g, *ref[name]) for name, g in zip(
        ("dx", "dgamma", "dbeta"), N.gn_emulate(*_np(*args), groups, defect=defect, where=where))}
    ch = c - 1                                                 # the last channel: the last group
    out = run("drop_term", (b - 1, ch))
    assert bool(out["dx"][b - 1, c - cpg:].any()) and not bool(out["dx"][:b - 1].any()) and bool(out["dbeta"][ch])
    out = run("no_gamma")
    assert all(bool(out["dx"][i, g * cpg:(g + 1) * cpg].any()) for i in range(b) for g in range(groups))
    if cpg > 1:
        out = run("mean_over_p")
        assert all(bool(out["dx"][i, g * cpg:(g + 1) * cpg].any()) for i in range(b) for g in range(groups))
    if b > 1:
        out = run("drop_partial", (b - 1, 0))
        assert bool(out["dgamma"].any()) and bool(out["dbeta"].any()) and not bool(out["dx"].any())


def test_stats_bounds_see_a_dropped_term():
    for rows, d in ((5, 65), (5, 1000), (3, 4095)):
        x = N.ln_inputs(rows, d)[0]
        ref = N.ln_stats_ref(x)
        mean, rstd = N.ln_stats_emulate(x.numpy(), drop=(rows - 1, d - 1))
        assert bool(N.over(mean, *ref["mean"])[rows - 1]) and not bool(N.over(mean, *ref["mean"])[:rows - 1].any())
    for b, c, p, groups in ((2, 8, 257, 4), (1, 4, 1000, 2)):
        x = N.gn_inputs(b, c, p)[0]
        ref = N.gn_stats_ref(x, groups)
        mean, rstd = N.gn_stats_emulate(x.numpy(), groups, drop=(b - 1, groups - 1, c // groups * p - 1))
        assert bool(N.over(mean, *ref["mean"])[b - 1, groups - 1]) and int(N.over(mean, *ref["mean"]).sum()) == 1


# ---- GEGLU / GELU --------------------------------------------------------------------------------------------------------------
def _geglu_inputs():
    for gelu_only in (False, True):
        for rows, inner in N.GEGLU_CASES:
            yield gelu_only, N.geglu_inputs(rows, inner, gelu_only)
        yield gelu_only, N.geglu_tail_inputs(gelu_only)


def test_geglu_budget_is_four_times_the_float32_cpu_ratio():
    worst = {"da": 0.0, "dgate": 0.0}
    for gelu_only, (u, dy) in _geglu_inputs():
        ref, unit, is_gate = N.geglu_ref(u, dy, gelu_only)
        got = N.geglu_f32_cpu(u, dy, gelu_only)
        worst["dgate"] = max(worst["dgate"], N.ratio(got[is_gate], ref[is_gate], unit[is_gate]))
        if not gelu_only:
            worst["da"] = max(worst["da"], N.ratio(got[~is_gate], ref[~is_gate], unit[~is_gate]))
    for name, w in worst.items():
        print(f"geglu {name}: float32 on the CPU {w:.3f} units, budget {N.GEGLU_R[name]} (recorded {N.GEGLU_CPU_MEASURED[name]})")
        # the constant is 4 x the recorded ratio; the ratio of this CPU's vector erf / exp may differ from the recorded one in
        # the last place of either function, never by a factor
        assert 0.5 * N.GEGLU_R[name] <= 4 * w <= 1.5 * N.GEGLU_R[name], (name, w)
        assert 4 * N.GEGLU_CPU_MEASURED[name] <= N.GEGLU_R[name] <= 4 * N.GEGLU_CPU_MEASURED[name] + 0.5


def test_geglu_units_see_a_wrong_derivative():
    """gelu' without its t phi(t) term, and the tanh approximation of gelu in da, are far outside the budget"""
    u, dy = N.geglu_inputs(5, 260, False)
    ref, unit, is_gate = N.geglu_ref(u, dy, False)
    a, t = u.chunk(2, -1)
    Phi = 0.5 * (1 + torch.erf(t * 0.7071067811865476))
    no_phi = torch.cat([dy * t * Phi, dy * a * Phi], -1)
    assert N.ratio(no_phi[is_gate], ref[is_gate], unit[is_gate]) > 1e3 * N.GEGLU_R["dgate"]
    tanh = torch.cat([dy * torch.nn.functional.gelu(t, approximate="tanh"), ref[:, 260:].float()], -1)
    assert N.ratio(tanh[~is_gate], ref[~is_gate], unit[~is_gate]) > 1e2 * N.GEGLU_R["da"]


def test_every_special_gate_is_among_the_inputs():
    for gelu_only in (False, True):
        for rows, inner in N.GEGLU_CASES:
            u, _ = N.geglu_inputs(rows, inner, gelu_only)
            gate = (u if gelu_only else u[:, inner:]).reshape(-1)
            assert gate[:len(N.GATES)].tolist() == [float(torch.tensor(v)) for v in N.GATES]


# ---- the launch rules and the workspace ------------------------------------------------------------------------------------------
def test_launch_rules():
    assert [N.ln_nv(d) for d in (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096)] == \
        [1, 1, 2, 2, 4, 4, 8, 8, 16, 16, 32, 32, 64, 64]
    assert [N.ln_rpb(r) for r in (1, 8, 9, 4096, 4097, 6151, 8193)] == [8, 8, 8, 8, 12, 16, 20]
    assert 4097 - (N.ln_blocks(4097) - 1) * 12 == 5 and 6151 - (N.ln_blocks(6151) - 1) * 16 == 7


@pytest.mark.parametrize("d", (1, 5, 33, 4096))
@pytest.mark.parametrize("rows", (1, 8, 9, 4096, 4097, 6151, 8193))
def test_layer_norm_workspace_is_exactly_two_rows_of_partials_per_block(rows, d):
    from tmdiff_amd._lib import lib
    assert lib.tmdiff_layer_norm_bwd_workspace_bytes(rows, d) == N.ceil_div(rows, N.ln_rpb(rows)) * 2 * d * 4


def test_layer_norm_workspace_of_no_rows_is_empty():
    from tmdiff_amd._lib import lib
    for d in (1, 40, 4096):
        assert lib.tmdiff_layer_norm_bwd_supported(0, d) == 1
        assert lib.tmdiff_layer_norm_bwd_workspace_bytes(0, d) == 0
