"""GPU tests of csrc/norm_bwd.hip (tmdiff_layer_norm_bwd, tmdiff_group_norm_bwd, tmdiff_geglu_bwd, col_sum_parts_kernel) and of
the *_stats forwards of csrc/attention.hip on the branches tests/test_gpu_norm_bwd.py never takes, with a yardstick that sees
one wrong element: every element of every gradient is held to the fp64 reference and the elementwise bound of
tests/norm_refs.py (derived there, proven valid and sharp on the CPU by tests/test_norm_refs_host.py).  The reference is
evaluated from the float32 inputs the kernel gets, the mean / rstd of the device forward included.

The entry points are called directly on views into flat buffers: inputs and NaN-filled outputs sit between sentinel runs, the
workspace is a view of exactly *_workspace_bytes bytes followed by sentinels.  After every call all sentinels are intact, no
input has changed and no NaN is left in a wanted output.

Branch -> the case that reaches it
  layer_norm_bwd_kernel<4>                   (6, 129), (5, 256)
  layer_norm_bwd_kernel<16> (row held)       (6, 513), (5, 1000), (5, 1024); (5, 1000) again with x = 100 + 0.01 randn
  layer_norm_bwd_kernel<32> (row re-read)    (5, 1025), (6, 2047)
  layer_norm_bwd_kernel<64>, ragged          (3, 4095)
  layer_norm_bwd_kernel<1>                   (4097, 3), (6151, 5), (9, 33), (0, 40)   [<2>, <8>, <64>: test_gpu_norm_bwd.py]
  ln_rows_per_block > 8                      (4097, 3): 12, last block of 5 rows; (6151, 5): 16, last block of 7 rows
  a block of one row, three idle waves       (9, 33)
  rows == 0 (NULL partials, nparts = 0)      (0, 40)
  col_sum_parts_kernel, per >= 2             (9, 8, 5, 4): per = 2, segments 5..7 empty, lo > nparts in 5..7;
                                             (17, 8, 3, 2): per = 3, lo > nparts in segment 7; (4097, 3), (6151, 5): per = 43, 49
  col_sum_parts_kernel, C % 32 != 0          (2, 40, 7, 5), and every LayerNorm D above
  group_norm_bwd_kernel, ragged strided trip (2, 8, 257, 4), (1, 4, 1000, 2)
  groups == 1                                (2, 12, 33, 1)
  gamma == NULL with dgamma / dbeta wanted   (2, 8, 257, 4) without affine
  geglu_bwd_kernel<1> with inner % 4 == 0    (3, 8), (5, 260) with u, dy or du one float off 16-byte alignment, both modes
  geglu_bwd_kernel<4>                        the same cases aligned
  geglu_bwd_kernel<1> with inner % 4 != 0    (7, 6), and the 13 tail gates
Not tested: the grid-stride trip of geglu_bwd (more than 2^20 workgroups, 2^28 vector elements: several GB per tensor)."""
import functools
import itertools

import pytest
import torch

import norm_refs as N
from norm_refs import G, put, same_bits

pytestmark = pytest.mark.gpu

ids = lambda e: "x".join(map(str, e))
ALL = (True, True, True)
NEEDS = [n for n in itertools.product((True, False), repeat=3) if any(n) and not all(n)]
WORST = {}                     # "operator gradient" -> worst error / bound seen


@pytest.fixture(scope="module")
def ops():
    from tmdiff_amd import ops
    yield ops
    torch.cuda.synchronize()
    for name in sorted(WORST):
        print(f"\nWORST {name}: {WORST[name]:.3f} of the bound")


def within(name, what, got, ref, bound, limit=1.0):
    assert not bool(torch.isnan(got).any()), f"{name} {what}: an element was never written (NaN left)"
    r = N.ratio(got, ref, bound)
    WORST[name] = max(WORST.get(name, 0.0), r)
    print(f"{name} {what}: worst error / bound {r:.3f}" + ("" if limit == 1.0 else f" (budget {limit})"))
    assert r <= limit, f"{name} {what}: {r:.3f} x the bound; {int(((got.cpu().double().reshape(ref.shape) - ref).abs() > limit * bound).sum())} elements outside"


def ptr(g):
    return None if g is None else g.ptr


def finish(ops, status, what, guards):
    ops.check(status, what)
    torch.cuda.synchronize()
    for g in guards:
        if g is not None:
            g.check(what)


# ---- direct calls on guarded buffers ---------------------------------------------------------------------------------------------
def ln_stats(ops, x, gamma, beta):
    rows, d = x.shape
    ins = [put(x), put(gamma), put(beta)]
    y, mean, rstd = G((rows, d)), G(rows), G(rows)
    st = ops.lib.tmdiff_layer_norm_stats(*map(ptr, ins), y.ptr, mean.ptr, rstd.ptr, rows, d, N.LN_EPS, ops.stream_ptr())
    finish(ops, st, "layer_norm_stats", ins + [y, mean, rstd])
    return y.t, mean.t, rstd.t


def ln_bwd(ops, x, gamma, dy, mean, rstd, need=ALL):
    """(dx, dgamma, dbeta) as device tensors, None where not wanted; mean / rstd: device tensors of the forward"""
    rows, d = x.shape
    ins = [put(x), put(gamma), put(dy), put(mean), put(rstd)]
    outs = [G((rows, d)) if need[0] else None, G(d) if need[1] else None, G(d) if need[2] else None]
    nws = ops.lib.tmdiff_layer_norm_bwd_workspace_bytes(rows, d)
    assert nws == N.ln_blocks(rows) * 2 * d * 4 if rows else nws == 0
    ws = G(nws // 4) if need[1] or need[2] else None
    st = ops.lib.tmdiff_layer_norm_bwd(*map(ptr, ins), *map(ptr, outs), ptr(ws), rows, d, ops.stream_ptr())
    finish(ops, st, f"layer_norm_bwd {rows}x{d} need={need}", ins + outs + [ws])
    return [None if o is None else o.t for o in outs]


def gn_stats(ops, x, gamma, beta, groups):
    b, c, p = x.shape
    ins = [put(x), put(gamma), put(beta)]
    y, mean, rstd = G((b, c, p)), G((b, groups)), G((b, groups))
    st = ops.lib.tmdiff_group_norm_stats(*map(ptr, ins), y.ptr, mean.ptr, rstd.ptr, b, c, p, groups, N.GN_EPS, ops.stream_ptr())
    finish(ops, st, "group_norm_stats", ins + [y, mean, rstd])
    return y.t, mean.t, rstd.t


def gn_bwd(ops, x, gamma, dy, mean, rstd, groups, need=ALL):
    b, c, p = x.shape
    ins = [put(x), put(gamma), put(dy), put(mean), put(rstd)]
    outs = [G((b, c, p)) if need[0] else None, G(c) if need[1] else None, G(c) if need[2] else None]
    nws = ops.lib.tmdiff_group_norm_bwd_workspace_bytes(b, c, p, groups)
    assert nws == 2 * b * c * 4
    ws = G(nws // 4) if need[1] or need[2] else None
    st = ops.lib.tmdiff_group_norm_bwd(*map(ptr, ins), *map(ptr, outs), ptr(ws), b, c, p, groups, ops.stream_ptr())
    finish(ops, st, f"group_norm_bwd {b}x{c}x{p}/{groups} need={need}", ins + outs + [ws])
    return [None if o is None else o.t for o in outs]


def geglu_bwd(ops, u, dy, gelu_only, offs=None):
    offs = offs or {}
    rows, inner = dy.shape
    gu, gd, du = put(u, offs.get("u", 0)), put(dy, offs.get("dy", 0)), G(u.shape, off=offs.get("du", 0))
    st = ops.lib.tmdiff_geglu_bwd(gu.ptr, gd.ptr, du.ptr, rows, inner, 1 if gelu_only else 0, ops.stream_ptr())
    finish(ops, st, f"geglu_bwd {rows}x{inner} gelu_only={gelu_only} offsets {offs}", [gu, gd, du])
    return du.t


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ln_case(extents, offset=0.3, scale=1.5):
    return N.ln_inputs(*extents, offset, scale)


def check_layer_norm(ops, extents, offset=0.3, scale=1.5):
    x, gamma, beta, dy = ln_case(extents, offset, scale)
    what = f"{extents}" + ("" if offset == 0.3 else f" x = {offset} + {scale} randn")
    y, mean, rstd = ln_stats(ops, x, gamma, beta)
    assert same_bits(y, ops.layer_norm(x.cuda(), gamma.cuda(), beta.cuda(), N.LN_EPS)), f"{what}: y of the stats form differs"
    stats = N.ln_stats_ref(x)
    within("layer_norm_stats mean", what, mean, *stats["mean"])
    within("layer_norm_stats rstd", what, rstd, *stats["rstd"])
    grads = ln_bwd(ops, x, gamma, dy, mean, rstd)
    ref = N.ln_ref(x, gamma, dy, mean.cpu(), rstd.cpu())
    for name, got in zip(("dx", "dgamma", "dbeta"), grads):
        within(f"layer_norm_bwd {name}", what, got, *ref[name])
    return (x, gamma, dy, mean, rstd), grads


@pytest.mark.parametrize("extents", N.LN_D_CASES + N.LN_ROW_CASES, ids=ids)
def test_layer_norm_backward(ops, extents):
    check_layer_norm(ops, extents)


def test_layer_norm_backward_of_a_badly_conditioned_row(ops):
    """x = 100 + 0.01 randn: rstd is about 100, and the bound scales with it"""
    (_, _, _, _, rstd), _ = check_layer_norm(ops, (5, 1000), 100.0, 0.01)
    assert float(rstd.min()) > 50.0


def test_layer_norm_backward_of_no_rows(ops):
    """dgamma and dbeta are exactly 0 (a sum over nothing), dx is empty, and nothing else is written"""
    x, gamma, beta, dy = N.ln_inputs(0, 40)
    empty = torch.empty(0)
    for need in [ALL] + NEEDS:
        dx, dgamma, dbeta = ln_bwd(ops, x, gamma, dy, empty, empty, need)
        for got in (dgamma, dbeta):
            assert got is None or (got.shape == (40,) and same_bits(got, torch.zeros(40, device="cuda")))
        assert dx is None or dx.numel() == 0
    y, mean, rstd = ln_stats(ops, x, gamma, beta)
    assert y.numel() == 0 and mean.numel() == 0


# ---- GroupNorm -------------------------------------------------------------------------------------------------------------------
def check_group_norm(ops, extents, affine=True, need=ALL):
    b, c, p, groups = extents
    x, gamma, beta, dy = N.gn_inputs(b, c, p, affine)
    what = f"{extents}" + ("" if affine else " without affine")
    y, mean, rstd = gn_stats(ops, x, gamma, beta, groups)
    plain = ops.group_norm(x.cuda(), None if gamma is None else gamma.cuda(), None if beta is None else beta.cuda(), groups, N.GN_EPS)
    assert same_bits(y, plain), f"{what}: y of the stats form differs"
    stats = N.gn_stats_ref(x, groups)
    within("group_norm_stats mean", what, mean, *stats["mean"])
    within("group_norm_stats rstd", what, rstd, *stats["rstd"])
    grads = gn_bwd(ops, x, gamma, dy, mean, rstd, groups, need)
    ref = N.gn_ref(x, gamma, dy, mean.cpu(), rstd.cpu(), groups)
    for name, got, wanted in zip(("dx", "dgamma", "dbeta"), grads, need):
        assert (got is not None) == wanted
        if wanted:
            within(f"group_norm_bwd {name}", what, got, *ref[name])
    return (x, gamma, dy, mean, rstd), grads


@pytest.mark.parametrize("extents", N.GN_CASES, ids=ids)
def test_group_norm_backward(ops, extents):
    check_group_norm(ops, extents)


def test_group_norm_backward_without_affine(ops):
    """gamma == NULL: dx alone, then all three; dgamma is then sum dy xhat (the gradient of a gamma of ones)"""
    _, only_dx = check_group_norm(ops, N.GN_NO_AFFINE, affine=False, need=(True, False, False))
    _, grads = check_group_norm(ops, N.GN_NO_AFFINE, affine=False)
    assert same_bits(only_dx[0], grads[0])


# ---- GEGLU / GELU ------------------------------------------------------------------------------------------------------------------
def check_geglu(what, du, u, dy, gelu_only):
    ref, unit, is_gate = N.geglu_ref(u, dy, gelu_only)
    got = du.cpu()
    mode = "gelu" if gelu_only else "geglu"
    within(f"{mode}_bwd dgate", what, got[is_gate], ref[is_gate], unit[is_gate], N.GEGLU_R["dgate"])
    if not gelu_only:
        within("geglu_bwd da", what, got[~is_gate], ref[~is_gate], unit[~is_gate], N.GEGLU_R["da"])


@pytest.mark.parametrize("gelu_only", (False, True), ids=("geglu", "gelu"))
@pytest.mark.parametrize("extents", N.GEGLU_ALIGN_CASES, ids=ids)
def test_geglu_backward_aligned_and_one_operand_misaligned(ops, extents, gelu_only):
    """inner % 4 == 0: aligned tensors take the float4 kernel, one misaligned operand the scalar one; the same bits"""
    u, dy = N.geglu_inputs(*extents, gelu_only)
    base = geglu_bwd(ops, u, dy, gelu_only)
    check_geglu(f"{extents} aligned", base, u, dy, gelu_only)
    for which in ("u", "dy", "du"):
        got = geglu_bwd(ops, u, dy, gelu_only, {which: 1})
        check_geglu(f"{extents} {which} misaligned", got, u, dy, gelu_only)
        differ = int((got.view(torch.int32) != base.view(torch.int32)).sum())
        assert differ == 0, f"{extents} gelu_only={gelu_only}: {which} misaligned differs from the aligned call in {differ} elements"


@pytest.mark.parametrize("gelu_only", (False, True), ids=("geglu", "gelu"))
def test_geglu_backward_odd_row_length_and_tails(ops, gelu_only):
    u, dy = N.geglu_inputs(7, 6, gelu_only)
    check_geglu("(7, 6)", geglu_bwd(ops, u, dy, gelu_only), u, dy, gelu_only)
    u, dy = N.geglu_tail_inputs(gelu_only)
    du = geglu_bwd(ops, u, dy, gelu_only)
    check_geglu("tails", du, u, dy, gelu_only)
    assert bool(torch.isfinite(du).all())


# ---- need subsets, reproducibility, the ops wrappers -----------------------------------------------------------------------------
def test_layer_norm_need_subsets_and_second_call(ops):
    (x, gamma, dy, mean, rstd), grads = check_layer_norm(ops, (6151, 5))
    for a, b in zip(ln_bwd(ops, x, gamma, dy, mean, rstd), grads):
        assert same_bits(a, b), "a second call differs"
    for need in NEEDS:
        part = ln_bwd(ops, x, gamma, dy, mean, rstd, need)
        for k in range(3):
            assert (part[k] is None) if not need[k] else same_bits(part[k], grads[k]), (need, k)


def test_group_norm_need_subsets_and_second_call(ops):
    extents = (9, 8, 5, 4)
    (x, gamma, dy, mean, rstd), grads = check_group_norm(ops, extents)
    for a, b in zip(gn_bwd(ops, x, gamma, dy, mean, rstd, 4), grads):
        assert same_bits(a, b), "a second call differs"
    for need in NEEDS:
        part = gn_bwd(ops, x, gamma, dy, mean, rstd, 4, need)
        for k in range(3):
            assert (part[k] is None) if not need[k] else same_bits(part[k], grads[k]), (need, k)


def test_ops_wrappers_return_the_bits_of_the_direct_calls(ops):
    cu = lambda t: None if t is None else t.cuda()
    x, gamma, beta, dy = ln_case((6, 2047))
    direct = ln_stats(ops, x, gamma, beta)
    for a, b in zip(ops.layer_norm_stats(cu(x), cu(gamma), cu(beta), N.LN_EPS), direct):
        assert same_bits(a, b)
    for a, b in zip(ops.layer_norm_bwd(cu(x), cu(gamma), cu(dy), direct[1], direct[2]), ln_bwd(ops, x, gamma, dy, direct[1], direct[2])):
        assert same_bits(a, b)
    for affine in (True, False):
        b_, c, p, groups = N.GN_NO_AFFINE
        x, gamma, beta, dy = N.gn_inputs(b_, c, p, affine)
        direct = gn_stats(ops, x, gamma, beta, groups)
        for a, b in zip(ops.group_norm_stats(cu(x), cu(gamma), cu(beta), groups, N.GN_EPS), direct):
            assert same_bits(a, b)
        for a, b in zip(ops.group_norm_bwd(cu(x), cu(gamma), cu(dy), direct[1], direct[2], groups),
                        gn_bwd(ops, x, gamma, dy, direct[1], direct[2], groups)):
            assert same_bits(a, b)
    for gelu_only in (False, True):
        u, dy = N.geglu_inputs(5, 260, gelu_only)
        assert same_bits(ops.geglu_bwd(cu(u), cu(dy), gelu_only=gelu_only), geglu_bwd(ops, u, dy, gelu_only))
