"""conv3d_w2_refs.py proved on the host: the restated plan is the library's, every case reaches what its comment claims, its
lattice inputs are exact under the absolute-value chain, the routing mirrors agree with the library on it, every mutation of
the reference changes the reference of every case it applies to (so the inputs can tell the mistakes apart), and the reference
itself equals an independent evaluation of the 24-plane Winograd chain."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv3d_w2_refs as R
from tmdiff_amd import _lib, ops, routing

P = 16                # a placeholder pointer (never dereferenced)
MUT_COUT = 16         # output channels the mutation checks evaluate: every mistake shows in the first 16


def _desc_fields(c):
    """the descriptor fields ops.conv3d_w2 sets for the case's epilogue, as placeholders"""
    e = c.epi
    f = {}
    if e["res"]:
        f["residual"] = P
    if e["rc"]:
        f.update(rc_x=P, rc_w=P, rc_cin=e["rc"])
    if e["dwt"]:
        f.update(y_ll=P, y_hi=(P, P, P))
    else:
        if e["keep_y"]:
            f["y"] = P
        if e["y2"] is not None:
            f["y2"] = P
        if e["ll"]:
            f["y_ll"] = P
        if e["s2d"]:
            f["y2_s2d"] = 1
    if e["pro"] is not None:
        f.update(in_shift=P, in_act=1 if e["pro"]["act"] else 0)
    return f


def test_xp_never_decides_g():
    """W2_XP = 384 staged positions hold every image count W2_NP = 256 output positions allow, for every plane the kernel takes:
    (H + 2) / H <= 3 / 2 from H = 4 on.  So G = min(256 / OP, Q) and a tile's staged positions never run short."""
    for h in range(4, 33):
        for tw in range(1, 9):
            p = R.plan(64, 128, 256, 8, h, 2 * tw)
            assert p.G_xp >= p.G_np >= 1 and p.G == p.G_np, (h, tw, p)
            assert p.G * p.IP <= R.W2_XP and p.G * p.OP <= R.W2_NP


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.name)
def test_case_reaches_what_it_claims_and_the_plan_is_the_librarys(c):
    p = R.case_plan(c)
    reaches = p.reaches(c.epi["rc"])
    assert {k: reaches[k] for k in c.claims} == c.claims, (c.name, reaches)
    assert reaches["odd_h"] == (c.H % 2 == 1) and reaches["stages"] == c.cin // 16 and reaches["cotiles"] == c.cout // 64
    fields = _desc_fields(c)
    quarter = c.epi["s2d"] or c.epi["ll"] or c.epi["dwt"]
    ext = (c.B, c.cin, c.cout, c.N, c.H, c.W, 1)
    # the two mirrors against the two entry points
    assert routing.wino2d_ok(*ext) and routing.wino2d_epilogue_ok(*ext, rc_cin=c.epi["rc"], quarter=quarter)
    assert routing.supported("tmdiff_conv3d_w2_epilogue_supported", *ext, **fields)
    assert routing.supported("tmdiff_conv3d_w2_supported", *ext, **fields) == (not quarter and not c.epi["rc"])
    # the restated workspace against the library's, for the descriptor make_conv_desc builds (placeholders for the tensors)
    d = _lib.Conv3dDesc()
    d.B, d.N, d.H, d.W, d.Cin, d.Cout, d.groups, d.ksize, d.nseg = c.B, c.N, c.H, c.W, c.cin, c.cout, 1, 3, 1
    d.seg_c[0] = c.cin
    for k, v in fields.items():
        setattr(d, k, v)
    assert _lib.lib.tmdiff_conv3d_w2_workspace_bytes(C.byref(d)) == p.workspace_bytes, (c.name, p)


def test_the_case_table_covers_the_paths():
    """Conditions on the table as a whole: every path the two older conv3d_w2 test files leave unreached is reached by some case."""
    r = {c.name: R.case_plan(c).reaches(c.epi["rc"]) for c in R.CASES}
    epi = {c.name: c.epi for c in R.CASES}
    some = lambda pred: any(pred(r[n], epi[n], R.CASE[n]) for n in r)
    assert some(lambda r_, e, c: r_["partial_last_tile"] and r_["ends_inside_block"] and not (e["rc"] or e["ll"]))
    assert some(lambda r_, e, c: r_["partial_last_tile"] and (e["s2d"] or e["ll"]))                 # a quarter output on a partial tile
    assert some(lambda r_, e, c: r_["partial_last_tile"] and c.N == 4 and R.case_plan(c).last_images == 1)
    assert some(lambda r_, e, c: r_["every_lane_live"] and not e["dwt"]) and some(lambda r_, e, c: r_["every_lane_live"] and e["dwt"])
    assert some(lambda r_, e, c: r_["odd_h"]) and some(lambda r_, e, c: r_["tw7"] == "halo") and some(lambda r_, e, c: c.W == 2)
    assert {r_["stages"] for r_ in r.values()} >= {8, 10, 16, 32} and some(lambda r_, e, c: r_["cotiles"] == 5)
    assert {c.B for c in R.CASES} >= {1, 2, 3, 5}
    assert {e["rc"] for e in epi.values()} >= {0, 32, 96, 512} and some(lambda r_, e, c: e["rc"] and c.N == 4)
    assert some(lambda r_, e, c: not e["keep_y"] and e["res"] and e["y2"] and not (e["ll"] or e["dwt"]))      # <false, true, true>
    assert some(lambda r_, e, c: e["y2"] and not e["y2"]["act"]) and some(lambda r_, e, c: e["bias_scale"] != 1.0)
    assert some(lambda r_, e, c: e["y2"] and e["y2"]["shift"] and not e["y2"]["scale"])
    assert some(lambda r_, e, c: e["y2"] and e["y2"]["scale"] and not e["y2"]["shift"])
    assert some(lambda r_, e, c: e["y2"] and e["y2"]["shift"] == "row") and some(lambda r_, e, c: e["pro"] and e["pro"]["shift"] == "row")
    assert some(lambda r_, e, c: e["pro"] and e["pro"]["act"] and c.N == 4) and some(lambda r_, e, c: e["pro"] and not e["pro"]["act"])
    assert some(lambda r_, e, c: e["ll"] and e["res"] and not e["rc"]) and some(lambda r_, e, c: not e["bias"])
    # every mutation applies somewhere, every case is told apart from at least three mistakes
    for m in R.MUTATIONS:
        assert any(R.applies(m, c) for c in R.CASES), m
    for c in R.CASES:
        assert sum(R.applies(m, c) for m in R.MUTATIONS) >= 3, c.name


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.name)
def test_lattice_inputs_are_exact_and_tell_the_mutations_apart(c):
    t = R.lattice(c)
    ok, worst = R.exactness_ok(c, t)
    print(f"conv3d_w2 lattice [{c.name}]: absolute-value chain / unit = {worst:.3e} of 2^24 = {R.TWO24:.3e}")
    assert ok, (c.name, worst)
    # the lattice itself: what the docstring says
    assert bool((t["x"] == t["x"].round()).all()) and float(t["x"].abs().max()) == 2.0
    assert set((t["w"] / 48).unique().tolist()) == {-1.0, 0.0, 1.0}
    # the reference on the first channels through F.conv3d and through the chain: both exact in fp64 on integers, so equal
    plain = R.reference(c, t, cout=MUT_COUT, chain=True)
    direct = R.reference(c, t, cout=MUT_COUT)
    assert set(plain) == set(direct) == set(R.outputs_of(c))
    exact = [k for k in plain if k not in R.silu_outputs(c)]
    for k in plain:
        if k in exact:
            assert torch.equal(plain[k], direct[k]), (c.name, k)
        else:
            assert torch.allclose(plain[k], direct[k], rtol=1e-14, atol=1e-300), (c.name, k)
    for m in R.MUTATIONS:
        if not R.applies(m, c):
            continue
        wrong = R.reference(c, t, mutation=m, cout=MUT_COUT)
        changed = {k: int((wrong[k] != plain[k]).sum()) for k in plain}
        assert any(changed.values()), f"{c.name}: mutation {m} does not change the reference on the lattice inputs"
        # ... and by far more than the SiLU outputs' tolerance, where only those are returned
        if not any(changed[k] for k in exact):
            k = max(changed, key=changed.get)
            assert float((wrong[k] - plain[k]).abs().max()) > 1e-3 * float(plain[k].abs().max()), (c.name, m)


def test_the_reference_equals_an_independent_winograd_evaluation():
    """On real-valued data (nothing exact about it): F.conv3d in double against the 24-plane chain written out in numpy, one
    tiny case with two band tiles, three column pairs and an odd number of rows."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 8, 8, 5, 6, generator=g, dtype=torch.float64)
    w = torch.randn(4, 8, 3, 3, 3, generator=g, dtype=torch.float64)
    want = F.conv3d(x, w, None, padding=1).numpy()
    got = R.wino_chain(x.numpy(), w.numpy())
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # every chain mutation is a different function on such data as well
    for m in R.CHAIN_MUTATIONS[:-1]:
        assert np.abs(R.wino_chain(x.numpy(), w.numpy(), m) - want).max() > 1e-3 * np.abs(want).max(), m
    assert np.abs(R.wino_chain(x.numpy(), w.numpy(), band_fill=np.ones((2, 8))) - want).max() > 1e-3


def test_refusals_on_the_host():
    """What test_gpu_conv3d_w2_edges.py expects ops.conv3d_w2 to refuse, asked of the mirrors and the library without a GPU."""
    ok = (2, 128, 256, 8, 8, 8)
    assert routing.wino2d_ok(*ok)
    for i, vals in ((4, (3, 33)), (5, (18, 7)), (1, (96, 144)), (2, (192, 288)), (3, (6,))):
        for v in vals:
            ext = ok[:i] + (v,) + ok[i + 1:]
            assert not routing.wino2d_ok(*ext) and not routing.supported("tmdiff_conv3d_w2_epilogue_supported", *ext), ext
    odd = (2, 128, 256, 8, 7, 8, 1)
    assert routing.wino2d_ok(*odd) and not routing.wino2d_epilogue_ok(*odd, rc_cin=32) and not routing.wino2d_epilogue_ok(*odd, quarter=True)
    for rc in (48, 544):
        assert not routing.wino2d_epilogue_ok(*ok, 1, rc_cin=rc)
    assert not routing.wino2d_epilogue_ok(2, 128, 256, 4, 8, 8, 1, quarter=True)
    for extra in (dict(in_mask=P), dict(drop_p=0.1), dict(rc_x=P, rc_w=P, rc_cin=32, residual=P, y=P)):
        assert not routing.supported("tmdiff_conv3d_w2_epilogue_supported", *ok, 1, **extra), extra
    assert hasattr(ops, "conv3d_w2")
