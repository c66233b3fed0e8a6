"""conv3d_wf_refs.py proved on the host: the restated plan is the library's (tiles, split factor, workspaces, what the entry
points accept), every listed path is reached by a named case, the lattice inputs are exact under the absolute-value chain,
the reference equals an independent evaluation of the six-plane Winograd chain, and every wrong variant of the reference
changes the reference of every case it applies to by at least one lattice step (so the exact tier can see that mistake)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv3d_wf_refs as R
from tmdiff_amd import _lib, ops, routing

P = 16                # a placeholder pointer (never dereferenced)
MUT_COUT = 16         # output channels the mutation checks evaluate (groups = 1): every mistake shows in the first 16


def _desc(c):
    """the descriptor ops.conv3d_wf builds for the case as the kernel sees it (placeholders for the tensors)"""
    o = c.opt
    B, cin, cout, N, H, W, groups = R.kernel_extents(c)
    d = _lib.Conv3dDesc()
    d.B, d.N, d.H, d.W, d.Cin, d.Cout, d.groups, d.ksize = B, N, H, W, cin, cout, groups, 3
    segs = (cin,) if o["llm"] else c.segs
    d.nseg = len(segs)
    for i, s in enumerate(segs):
        d.seg_c[i] = s
    if o["pro"] is not None:
        if o["pro"]["shift"]:
            d.in_shift = P
        if o["pro"]["scale"]:
            d.in_scale = P
        d.in_act = 1 if o["pro"]["act"] else 0
    if o["drop"]:
        d.drop_p = R.DROP[1]
    if o["rc"]:
        d.rc_x, d.rc_w, d.rc_cin = P, P, o["rc"]
    return d


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.name)
def test_the_plan_is_the_librarys(c):
    p, o = R.case_plan(c), c.opt
    B, cin, cout, N, H, W, groups = R.kernel_extents(c)
    tiles = C.c_int64(0)
    split = _lib.lib.tmdiff_conv3d_wf_plan(B, cin, cout, N, H, W, groups, 1 if o["llm"] else 0, C.byref(tiles))
    want_split = R.wf_ksplit(B, cin, cout, N, H, W, groups, pairs=o["llm"])[0]
    assert (split, tiles.value) == (want_split, p.tiles), (c.name, split, tiles.value, p)
    assert p.split == (1 if (o["ll"] or o["dwt"]) else want_split)
    if o["s2d"] or o["ll"] or o["dwt"]:
        assert want_split == 1 and routing.wf_quarter_ok(B, cin, cout, N, H, W, groups), c.name
    d = _desc(c)
    assert _lib.lib.tmdiff_conv3d_wf_supported(C.byref(d))
    assert routing.wf_route(B, cin, cout, N, H, W, groups, llm=o["llm"])[1] == want_split
    assert _lib.lib.tmdiff_conv3d_wf_workspace_bytes(C.byref(d)) == p.prologue_bytes, c.name
    if not o["llm"]:
        assert _lib.lib.tmdiff_conv3d_wf_splitk_workspace_bytes(C.byref(d)) == 4 * want_split * B * cout * N * H * W * (want_split > 1)
        assert p.splitk_bytes == (0 if (o["ll"] or o["dwt"]) else 4 * want_split * B * cout * N * H * W * (want_split > 1))
    else:
        e = _lib.Conv3dDesc()
        e.B, e.N, e.H, e.W, e.Cin, e.Cout, e.groups, e.ksize, e.nseg = c.B, c.N, c.H, c.W, sum(c.segs), c.cout, 1, 3, 1
        e.seg_c[0] = sum(c.segs)
        assert _lib.lib.tmdiff_conv3d_wfll_supported(C.byref(e))
        assert _lib.lib.tmdiff_conv3d_wfll_splitk_workspace_bytes(C.byref(e)) == p.splitk_bytes
        assert (p.chunks // p.split) % 2 == 0, "a range of the composed-LL mode holds whole chunk pairs"
    # the geometry and the loop counts as the kernel's launch() derives them
    th, tw = (8, 16) if N == 8 else (16, 16)
    assert (p.TT * 4, p.TH, p.TW) == (N, th, tw) and p.tiles_h == -(-H // th) and p.tiles_co == cout // groups // 32
    assert p.tiles_w == (1 if (N == 8 and W == 8) else -(-W // 16)) and p.chunks == cin // groups // 2
    units = (B + 1) // 2 if p.mode == "pair" else B
    assert p.tiles == units * groups * p.tiles_h * p.tiles_w * p.tiles_co


def test_every_listed_path_is_reached_by_a_named_case():
    r = {c.name: R.reaches(c) for c in R.CASES}
    o = {c.name: c.opt for c in R.CASES}
    some = lambda pred: [n for n in r if pred(r[n], o[n], R.CASE[n])]
    need = {
        "H below a tile, N = 8": lambda r_, o_, c: r_["mode"] == "n8" and r_["h_below_tile"],
        "H below a tile, N = 4": lambda r_, o_, c: r_["mode"] == "n4" and r_["h_below_tile"],
        "H below a tile, pair": lambda r_, o_, c: r_["mode"] == "pair" and r_["h_below_tile"],
        "ragged last row tile, N = 8": lambda r_, o_, c: r_["mode"] == "n8" and r_["ragged_last_row_tile"],
        "ragged last row tile, N = 4": lambda r_, o_, c: r_["mode"] == "n4" and r_["ragged_last_row_tile"],
        "ragged last row tile, pair": lambda r_, o_, c: r_["mode"] == "pair" and r_["ragged_last_row_tile"],
        "last column tile of one quad": lambda r_, o_, c: r_["last_col_quads"] == 1 and r_["col_tiles"] > 1,
        "last column tile of two quads": lambda r_, o_, c: r_["last_col_quads"] == 2,
        "last column tile of three quads": lambda r_, o_, c: r_["last_col_quads"] == 3 and r_["col_tiles"] > 1,
        "three quads in the only tile": lambda r_, o_, c: r_["last_col_quads"] == 3 and r_["col_tiles"] == 1,
        "W == 4, N = 8": lambda r_, o_, c: r_["w4"] and r_["mode"] == "n8" and not r_["llm"],
        "W == 4, N = 4": lambda r_, o_, c: r_["w4"] and r_["mode"] == "n4" and not r_["llm"],
        "pair, odd batch": lambda r_, o_, c: r_["pair_odd_batch"] and not r_["pair_single"],
        "pair, B == 1": lambda r_, o_, c: r_["pair_single"],
        "pair, grouped segments in place": lambda r_, o_, c: r_["mode"] == "pair" and r_["grouped_in_place"],
        "a single chunk": lambda r_, o_, c: r_["single_chunk"],
        "an odd chunk count": lambda r_, o_, c: r_["odd_chunks"] and r_["chunks"] > 1,
        "two chunks per range": lambda r_, o_, c: r_["split"] > 1 and r_["chunks_per_range"] == 2 and not r_["llm"],
        "the doubling branch": lambda r_, o_, c: r_["doubled"],
        "cin_g = 256 unsplit": lambda r_, o_, c: r_["chunks"] == 128 and r_["split"] == 1,
        "the fold in range 0 only": lambda r_, o_, c: r_["fold_in_range0_only"],
        "a fold on N = 4": lambda r_, o_, c: r_["fold"] and r_["mode"] == "n4",
        "a fold on a ragged plane": lambda r_, o_, c: r_["fold"] and r_["ragged_last_row_tile"] and r_["last_col_quads"] != 4,
        "the prologue pass": lambda r_, o_, c: r_["prologue_pass"],
        "a concatenation": lambda r_, o_, c: r_["prologue_pass"] and len(c.segs) == 2 and o_["pro"] is None,
        "dropout with xp_out": lambda r_, o_, c: o_["drop"],
        "s2d at H = 2, W = 4": lambda r_, o_, c: r_["quarter"] == "s2d" and (c.H, c.W) == (2, 4),
        "LL at H = 2, W = 12": lambda r_, o_, c: r_["quarter"] == "ll" and (c.H, c.W) == (2, 12),
        "Haar at H = 2, W = 12": lambda r_, o_, c: r_["quarter"] == "dwt" and (c.H, c.W) == (2, 12),
        "Haar on several tiles": lambda r_, o_, c: r_["quarter"] == "dwt" and r_["col_tiles"] > 1 and c.H > 8,
        "mode 3": lambda r_, o_, c: o_["dgrad"],
        "composed LL, N = 8": lambda r_, o_, c: r_["llm"] and r_["mode"] == "n8",
        "composed LL, N = 4": lambda r_, o_, c: r_["llm"] and r_["mode"] == "n4",
        "composed LL, pair, split": lambda r_, o_, c: r_["llm"] and r_["mode"] == "pair" and r_["split"] > 1,
        "composed LL, ll_scale != 0.5 on a split grid": lambda r_, o_, c: r_["llm"] and r_["split"] > 1 and o_["ll_scale"] != 0.5 and o_["bias"],
    }
    for what, pred in need.items():
        assert some(pred), what
    assert len(some(lambda r_, o_, c: o_["dgrad"])) >= 2
    for q in ("s2d", "ll", "dwt"):         # each quarter output with and without a residual or a fold
        assert some(lambda r_, o_, c: r_["quarter"] == q and (o_["res"] or o_["rc"])) and some(lambda r_, o_, c: r_["quarter"] == q and not (o_["res"] or o_["rc"]))
    hs = lambda mode: {c.H for c in R.CASES if R.reaches(c)["mode"] == mode and not c.opt["llm"]}
    assert hs("n8") >= {1, 2, 3, 7, 9} and hs("n4") >= {1, 5, 15, 17} and hs("pair") >= {1, 3, 8, 9}
    assert {c.W for c in R.CASES} >= {4, 12, 20, 28, 36}
    assert {c.B for c in R.CASES if R.reaches(c)["mode"] == "pair"} >= {1, 2, 3}
    assert {sum(c.segs) // c.groups for c in R.CASES} >= {2, 4, 6, 8, 128, 256}
    assert {c.opt["rc"] for c in R.CASES} >= {32, 96, 512}
    assert some(lambda r_, o_, c: o_["bias_scale"] != 1.0) and some(lambda r_, o_, c: o_["out_scale"] != 1.0)
    assert some(lambda r_, o_, c: o_["bias"] and not o_["res"]) and some(lambda r_, o_, c: o_["res"] and not o_["bias"] and not o_["dgrad"])
    pro = lambda sh, sc: some(lambda r_, o_, c: o_["pro"] is not None and (o_["pro"]["shift"], o_["pro"]["scale"]) == (sh, sc))
    assert pro(True, False) and pro(False, True)
    # the shape the doubling branch was first looked for at does not take it, and the library says the same
    assert r["long-sum-16x16"]["split"] == 32 and not r["long-sum-16x16"]["doubled"] and r["doubling"]["split"] == 4
    # every mutation applies somewhere; every case is told apart from at least four mistakes
    for m in R.MUTATIONS:
        assert any(R.applies(m, c) for c in R.CASES), m
    for c in R.CASES:
        assert sum(R.applies(m, c) for m in R.MUTATIONS) >= 4, c.name
    assert all(c.rounding for c in (R.CASE[n] for n in ("h9-w4", "h1-w12", "pair-h8-b3", "cin256-unsplit", "doubling", "fold512-split")))


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.name)
def test_lattice_inputs_are_exact_and_tell_the_mutations_apart(c):
    t = R.lattice(c)
    o = c.opt
    xp = None
    if o["drop"]:      # any keep mask serves on the host: every second element kept, scaled by 1.25
        xp = R.prologue64(t)
        xp = xp * 1.25 * (torch.arange(xp.numel()).reshape(xp.shape) % 2 == 0)
    ok, worst = R.exactness_ok(c, t, xp)
    print(f"conv3d_wf lattice [{c.name}]: absolute-value chain / unit = {worst:.3e} of 2^24 = {R.TWO24:.3e}")
    assert ok, (c.name, worst)
    assert all(bool((x == x.round()).all()) and float(x.abs().max()) == 2.0 for x in t["xs"])
    assert set((t["w"] / o["wstep"]).unique().tolist()) == {-1.0, 0.0, 1.0}
    cout = MUT_COUT if c.groups == 1 else None
    plain = R.reference(c, t, cout=cout, chain=True, xp=xp)
    direct = R.reference(c, t, cout=cout, xp=xp)
    assert tuple(plain) == tuple(direct) == R.outputs_of(c)
    exact = [k for k in plain if k not in R.silu_outputs(c)]
    for k in plain:
        if k in exact:     # both are exact in fp64 on the lattice: the restatement EQUALS F.conv3d
            assert torch.equal(plain[k], direct[k]), (c.name, k)
        else:
            assert torch.allclose(plain[k], direct[k], rtol=1e-14, atol=1e-300), (c.name, k)
    for m in R.MUTATIONS:
        if not R.applies(m, c):
            continue
        wrong = R.reference(c, t, mutation=m, cout=cout, xp=xp)
        diff = {k: float((wrong[k] - plain[k]).abs().max()) for k in plain}
        if exact:
            assert any(diff[k] >= R.step_of(c, k) for k in exact), f"{c.name}: mutation {m} moves no exact output by a lattice step: {diff}"
        else:              # (only SiLU outputs returned: far more than their tolerance)
            k = max(diff, key=diff.get)
            assert diff[k] > 1e-3 * float(plain[k].abs().max()), (c.name, m)


def test_the_reference_equals_an_independent_winograd_evaluation():
    """On real-valued data (nothing exact about it): F.conv3d in double against the six-plane chain written out in numpy --
    two band tiles, three groups, odd extents -- and the data-gradient weight against autograd."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 6, 8, 5, 7, generator=g, dtype=torch.float64)
    for groups in (1, 3):
        w = torch.randn(6, 6 // groups, 3, 3, 3, generator=g, dtype=torch.float64)
        want = F.conv3d(x, w, None, padding=1, groups=groups).numpy()
        got = R.wino_chain(x.numpy(), w.numpy(), groups)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        for m in R.CHAIN_MUTATIONS:
            assert np.abs(R.wino_chain(x.numpy(), w.numpy(), groups, m) - want).max() > 1e-3 * np.abs(want).max(), m
    for name in ("dgrad-n8", "dgrad-pair-groups3"):
        c = R.CASE[name]
        w = torch.randn(*R.weight_shape(c), generator=g, dtype=torch.float64)
        gy = torch.randn(c.B, sum(c.segs), 8, 3, 4, generator=g, dtype=torch.float64)
        xin = torch.zeros(c.B, c.cout, 8, 3, 4, dtype=torch.float64, requires_grad=True)
        F.conv3d(xin, w, None, padding=1, groups=c.groups).backward(gy)
        got = F.conv3d(gy, R.effective_weight(c, w), None, padding=1, groups=c.groups)
        assert torch.allclose(got, xin.grad, rtol=1e-12, atol=1e-12), name


def test_the_composed_ll_weights_are_the_convolution_then_the_ll_band():
    """packed_ref_wfll, applied as a stride-1 convolution with 2 x 2 taps per virtual channel of the space-to-depth tensor,
    equals F.conv3d followed by ll_scale / 2 times the 2 x 2 block sums (one 4-band tile, the inverse of G left out: the taps
    summed over the bands directly from the composed kernel)."""
    g = torch.Generator().manual_seed(9)
    w = torch.randn(32, 2, 3, 3, 3, generator=g, dtype=torch.float64)
    pk = R.packed_ref_wfll(w, 1.0).reshape(2, 2, 2, 4, 6, 32)
    # two rows of G pick single band taps: G[5] = e_2, G[0] = e_0 / 4
    w4 = torch.zeros(32, 2, 3, 4, 4, dtype=torch.float64)
    for P in range(2):
        for Q in range(2):
            w4[:, :, :, P:P + 3, Q:Q + 3] += 0.5 * w
    for ph in range(2):
        for pw in range(2):
            for i in range(2):
                for j in range(2):
                    a4, b4 = (1 + 2 * i if ph == 0 else 2 * i), (1 + 2 * j if pw == 0 else 2 * j)
                    assert torch.allclose(pk[:, ph, pw, i * 2 + j, 5].T, w4[:, :, 2, a4, b4], rtol=1e-13, atol=1e-13)
                    assert torch.allclose(4 * pk[:, ph, pw, i * 2 + j, 0].T, w4[:, :, 0, a4, b4], rtol=1e-13, atol=1e-13)
    x = torch.randn(1, 2, 4, 6, 8, generator=g, dtype=torch.float64)
    full = F.conv3d(x, w, None, padding=1)
    ll = 0.5 * (full[..., 0::2, 0::2] + full[..., 0::2, 1::2] + full[..., 1::2, 0::2] + full[..., 1::2, 1::2])
    assert torch.allclose(F.conv3d(x, w4, None, stride=(1, 2, 2), padding=1), ll, rtol=1e-12, atol=1e-12)


def test_refusals_on_the_host():
    """What test_gpu_conv3d_wf_edges.py expects ops.conv3d_wf to refuse, asked of the library's queries and the routing rules
    without a GPU."""
    ok = (2, 8, 32, 8, 8, 16)
    q = "tmdiff_conv3d_wf_supported"
    assert routing.supported(q, *ok)
    assert not routing.supported(q, 2, 8, 32, 6, 8, 16) and not routing.supported(q, 2, 8, 32, 8, 8, 6)
    assert not routing.supported(q, 2, 6, 32, 8, 8, 16, 3)                   # Cin / groups = 3
    assert not routing.supported(q, 2, 7, 32, 8, 8, 16)
    assert not routing.wf_quarter_ok(1, 8, 32, 8, 8, 16)                     # a split grid
    assert not routing.wf_quarter_ok(2, 2, 32, 8, 7, 16)                     # odd H
    assert routing.wf_quarter_ok(2, 2, 32, 8, 8, 8)                          # (pair planes: the entry point's own refusal)
    assert not routing.fold_k1(4, 32, 64, 64, 8, 8, 8)                       # a fold in pair mode is never planned
    assert hasattr(ops, "conv3d_wf") and hasattr(ops, "conv3d_wf_ll")
