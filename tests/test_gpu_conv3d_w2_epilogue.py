"""conv3d_w2's row-pair output pass (csrc/conv3d_w2.hip): the LL / Haar / space-to-depth outputs and the folded 1x1x1, against
the plain conv3d_w2 launch, the Haar kernel, fp64 convolutions on the CPU and the two-launch form; the route in conv3d_auto and
in the benchmark's network.

Shapes are the smallest at which the pass can go wrong: B = 2 (the sample stride of rc_x differs from y's), 128 -> 256 channels
(eight channel tiles), 8 bands (two band tiles), planes 16x16 (the workload's: whole 32-position blocks), 12x10 (five column
pairs: lanes past the plane in the transform, the MFMA block and the write-out; six row pairs) and 4x2 (one column pair, two
row pairs), a folded 1x1x1 of 32 (one group of K-steps) and 128 (four: both operand slots, the prefetch wrap) channels.

FOLD_BOUND: 2 x the worst error the folded launches measured on these cases (profiles/wino2d_epilogue.txt section 1), under the
2e-5 ceiling the other Winograd tests hold.  NET_BOUND: 2 x the difference the already-merged route (wino2d) makes on the same
forward (same file, section 4), under the (1e-5, 2e-6) of test_gpu_configs' fusion test."""
import collections

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close, rel_err
from oracle import unet_ref as U
from oracle.make_golden import FULL, case_inputs

pytestmark = pytest.mark.gpu

FOLD_BOUND = 7e-6           # 2 x the worst measured (3.444e-6, 8x12x10 +rc128), rounded up
assert FOLD_BOUND <= 2e-5
NET_BOUND = (4.8e-6, 2e-6)   # 2 x (2.357e-6, 1.675e-6) = (4.8e-6, 3.4e-6), the relative L2 figure cut at the ceiling
assert NET_BOUND[0] <= 1e-5 and NET_BOUND[1] <= 2e-6

B, CIN, COUT, N = 2, 128, 256, 8
PLANES = [(16, 16), (12, 10), (4, 2)]
SCALE = 0.7071


def cu(t):
    return None if t is None else t.detach().cuda().contiguous()


_CASE = {}


def _case(plane):
    """Inputs of one plane (CPU tensors) and the fp64 3x3x3 convolution without bias; computed once, never modified."""
    if plane not in _CASE:
        h, w = plane
        g = torch.Generator().manual_seed(1000 + 17 * h + w)
        t = dict(x=torch.randn(B, CIN, N, h, w, generator=g), w=torch.randn(COUT, CIN, 3, 3, 3, generator=g) / (27 * CIN) ** 0.5,
                 bias=torch.randn(COUT, generator=g) * 0.3, res=torch.randn(B, COUT, N, h, w, generator=g),
                 sh2=torch.randn(B, COUT, generator=g) * 0.3, sc2=torch.rand(B, COUT, generator=g) + 0.5)
        for cx in (32, 128):
            t[f"xr{cx}"] = torch.randn(B, cx, N, h, w, generator=g)
            t[f"w1_{cx}"] = torch.randn(COUT, cx, 1, 1, 1, generator=g) / cx ** 0.5
        t["conv64"] = F.conv3d(t["x"].double(), t["w"].double(), None, padding=1)
        _CASE[plane] = t
    return _CASE[plane]


def _gpu(plane):
    from tmdiff_amd import ops
    t = _case(plane)
    d = {k: cu(v) for k, v in t.items() if k != "conv64"}
    d["wp"] = ops.pack_conv_weight_w2(d["w"])
    d["em"] = dict(act=True, shift=d["sh2"], scale=d["sc2"])
    return d


def _err(got, want):
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


def _s2d(y2):
    """[B, C, N, H, W] -> [B, 4 C, N, H/2, W/2], channel 4 co + 2 ph + pw"""
    b, c, n, h, w = y2.shape
    return y2.reshape(b, c, n, h // 2, 2, w // 2, 2).permute(0, 1, 4, 6, 2, 3, 5).reshape(b, 4 * c, n, h // 2, w // 2)


@pytest.mark.parametrize("plane", PLANES)
def test_w2_writes_the_ll_band_and_the_space_to_depth_form(plane):
    """y_ll instead of y beside a plain or space-to-depth second output, residual and out_scale included: y2 bit-identical to
    the launch without y_ll, and (space-to-depth) to the plain launch's y2 rearranged; y_ll against the Haar kernel on the
    plain launch's y and against the definition."""
    from tmdiff_amd import ops
    d = _gpu(plane)
    kw = dict(bias=d["bias"], residual=d["res"], out_scale=SCALE)
    y_plain, y2_plain = ops.conv3d_w2(d["x"], d["wp"], COUT, emit=d["em"], **kw)      # the one-row output pass
    for s2d in (False, True):
        y, y2 = ops.conv3d_w2(d["x"], d["wp"], COUT, emit=dict(d["em"], s2d=s2d), **kw)
        y2b, yll = ops.conv3d_w2(d["x"], d["wp"], COUT, emit=dict(d["em"], s2d=s2d, ll=True), keep_y=False, **kw)
        assert torch.equal(y, y_plain)
        assert torch.equal(y2, y2b)
        assert torch.equal(y2, _s2d(y2_plain) if s2d else y2_plain)
        assert yll.shape == (B, COUT, N, plane[0] // 2, plane[1] // 2)
        want = ops.haar_dwt2d(y_plain, want_high=False, ll_scale=0.5)[0]
        assert_close(yll, want.cpu(), 1e-6, 5e-7, "LL output vs the Haar kernel on y")
        a_ = y_plain[..., 0::2, 0::2] + y_plain[..., 0::2, 1::2] + y_plain[..., 1::2, 0::2] + y_plain[..., 1::2, 1::2]
        assert_close(yll, (a_ * 0.25).cpu(), 1e-6, 5e-7, "LL output vs the definition")
    only = ops.conv3d_w2(d["x"], d["wp"], COUT, emit=dict(d["em"], s2d=True), keep_y=False, **kw)
    assert torch.equal(only, _s2d(y2_plain))


@pytest.mark.parametrize("plane", PLANES)
def test_w2_writes_the_haar_transform(plane):
    """y_ll + y_hi: LL / 2 through the emit prologue, LH, HL, HH instead of y, against the Haar kernel on the plain launch's y."""
    from tmdiff_amd import ops
    d = _gpu(plane)
    y = ops.conv3d_w2(d["x"], d["wp"], COUT, bias=d["bias"])
    got = ops.conv3d_w2(d["x"], d["wp"], COUT, bias=d["bias"], emit=dict(d["em"], dwt=True), keep_y=False)
    want = ops.haar_dwt2d(y, want_high=True, ll_scale=0.5, ll_prologue=dict(act=True, shift=d["sh2"], scale=d["sc2"]))
    assert len(got) == 4
    for nm, g_, w_ in zip(("LL'", "LH", "HL", "HH"), got, want):
        assert g_.shape == (B, COUT, N, plane[0] // 2, plane[1] // 2)
        assert_close(g_, w_.cpu(), 2e-6, 1e-6, f"Haar output {nm} vs the Haar kernel on y")


@pytest.mark.parametrize("cx", [32, 128])
@pytest.mark.parametrize("plane", PLANES)
def test_w2_folds_the_residual_convolution(plane, cx):
    """rc_x / rc_w / rc_cin: W1^T x added on the matrix pipe inside the output pass, against the fp64 convolutions (3x3x3 plus
    1x1x1 with bias, times out_scale, then the SiLU second output) and the two-launch form; with y_ll on top."""
    from tmdiff_amd import ops
    t, d = _case(plane), _gpu(plane)
    xr, w1 = d[f"xr{cx}"], d[f"w1_{cx}"]
    r64 = F.conv3d(t[f"xr{cx}"].double(), t[f"w1_{cx}"].double(), t["bias"].double())
    want = (t["conv64"] + r64) * SCALE
    v = want + t["sh2"].double()[:, :, None, None, None]
    want2 = v * torch.sigmoid(v) * t["sc2"].double()[:, :, None, None, None]
    kw = dict(bias=d["bias"], res_conv=(xr, w1, cx), out_scale=SCALE)
    y, y2 = ops.conv3d_w2(d["x"], d["wp"], COUT, emit=d["em"], **kw)
    # the same on the plain launch with an fp64-exact r (rounded once) as its residual: what the Winograd part alone costs
    yp, y2p = ops.conv3d_w2(d["x"], d["wp"], COUT, residual=cu(r64.float()), out_scale=SCALE, emit=d["em"])
    e_fold, e_plain = max(_err(y, want), _err(y2, want2)), max(_err(yp, want), _err(y2p, want2))
    print(f"wino2d epilogue error [{N}x{plane[0]}x{plane[1]} +rc{cx}]: folded {e_fold:.3e}  plain + exact r {e_plain:.3e}")
    assert e_fold <= FOLD_BOUND, (e_fold, e_plain)
    res = ops.conv3d([xr], ops.pack_conv_weight(w1), COUT, 1, bias=d["bias"])
    y_two, y2_two = ops.conv3d_w2(d["x"], d["wp"], COUT, residual=res, out_scale=SCALE, emit=d["em"])
    assert_close(y, y_two.cpu(), 5e-6, 2e-6, "folded vs two launches")           # (same products, another summation order)
    assert_close(y2, y2_two.cpu(), 5e-6, 2e-6, "folded vs two launches, second output")
    y2b, yll = ops.conv3d_w2(d["x"], d["wp"], COUT, emit=dict(d["em"], ll=True), keep_y=False, **kw)
    assert torch.equal(y2, y2b)
    assert_close(yll, ops.haar_dwt2d(y, want_high=False, ll_scale=0.5)[0].cpu(), 1e-6, 5e-7, "LL output with a folded res_conv")


def test_w2_refuses_what_it_does_not_write():
    from tmdiff_amd import ops
    d = _gpu((4, 2))
    em = d["em"]
    with pytest.raises(ValueError):
        ops.conv3d_w2(d["x"], d["wp"], COUT, emit=dict(em, ll=True))                              # the LL output replaces y
    with pytest.raises(ValueError):
        ops.conv3d_w2(d["x"], d["wp"], COUT, emit=dict(em, dwt=True, s2d=True), keep_y=False)
    with pytest.raises(ValueError):
        ops.conv3d_w2(d["x"], d["wp"], COUT, residual=d["res"], res_conv=(d["xr32"], d["w1_32"], 32))
    with pytest.raises(ValueError):                                                                # 4 bands
        ops.conv3d_w2(d["x"][:, :, :4].contiguous(), d["wp"], COUT, emit=dict(em, ll=True), keep_y=False)


def test_conv3d_auto_routes_the_three_launch_kinds_with_the_switch():
    """The launch kinds of the benchmark step that the row-pair pass adds (LL + folded 1x1x1 with a space-to-depth or a plain
    second output; the Haar transform) run on conv3d_wf with wino2d_epilogue off and on conv3d_w2 with it on: same results
    within twice the kernel bound."""
    from tmdiff_amd import ops
    d = _gpu((16, 16))
    wt = d["w"]
    weights = ops.ConvWeights(lambda: ops.pack_conv_weight(wt), lambda: ops.pack_conv_weight_wino(wt, mode=2, planes=6), None,
                              lambda: d["wp"])
    rc = dict(bias=d["bias"], res_conv=(d["xr128"], d["w1_128"], 128), out_scale=SCALE)
    kinds = [dict(emit=dict(d["em"], ll=True, s2d=True), keep_y=False, **rc), dict(emit=dict(d["em"], ll=True), keep_y=False, **rc),
             dict(emit=dict(d["em"], dwt=True), keep_y=False, bias=d["bias"])]
    outs = {}
    keep = ops.COUNTS
    try:
        for epi in (False, True):
            ops.COUNTS = collections.Counter()
            with ops.config.override(wino_min_blocks=1, wf_splitk=False, wino2d=True, wino2d_epilogue=epi):
                outs[epi] = [ops.conv3d_auto([d["x"]], weights, COUT, **kw) for kw in kinds]
            assert dict(ops.COUNTS) == {"conv3d_w2_fwd" if epi else "conv3d_wf_fwd": 3}, (epi, dict(ops.COUNTS))
    finally:
        ops.COUNTS = keep
    for off, on in zip(outs[False], outs[True]):
        assert len(off) == len(on)
        for a, b_ in zip(off, on):
            assert float((a - b_).abs().max() / a.abs().max()) <= 2 * FOLD_BOUND


def test_network_at_the_benchmark_shape_takes_the_route():
    """One forward of the benchmark workload (B = 32, widths 32-256, 64 x 64) per setting: with wino2d_epilogue on, all three
    launches (the two `256->256 8x16x16 y2 ll +rc128`, the `256->256 8x16x16 dwt`) move from conv3d_wf to conv3d_w2 -- no
    class is held back by the per-class rule -- and the output moves by no more than twice what the wino2d route itself moves it."""
    from tmdiff_amd import ops
    from tmdiff_amd.Hyper_unet_general import WavBEST
    net = U.fill_weights_(WavBEST(channels=FULL)).cuda().eval()
    d = {k: cu(v) for k, v in case_inputs(23, 32, 8, 64).items()}
    t = torch.arange(1, 33, dtype=torch.float32).reshape(32, 1).cuda() * 29

    def run(**switches):
        keep, ops.COUNTS = ops.COUNTS, collections.Counter()
        try:
            with ops.config.override(**switches), torch.no_grad():
                return net(d["x_t"], t, d["PAN"], d["MS"], "WV3"), dict(ops.COUNTS)
        finally:
            ops.COUNTS = keep

    y_none, c_none = run(wino2d=False)
    y_off, c_off = run(wino2d=True, wino2d_epilogue=False)
    y_on, c_on = run(wino2d=True, wino2d_epilogue=True)
    assert c_none.get("conv3d_w2_fwd", 0) == 0 and c_off["conv3d_w2_fwd"] == 6
    assert c_on["conv3d_w2_fwd"] == 9 and c_off["conv3d_wf_fwd"] - c_on["conv3d_wf_fwd"] == 3, (c_off, c_on)
    assert {k: v for k, v in c_on.items() if "_w" not in k} == {k: v for k, v in c_off.items() if "_w" not in k}
    base, new = rel_err(y_off, y_none), rel_err(y_on, y_off)
    print(f"wino2d epilogue network difference: wino2d off vs on max-rel {base[0]:.3e} rel-L2 {base[1]:.3e}; "
          f"wino2d_epilogue off vs on max-rel {new[0]:.3e} rel-L2 {new[1]:.3e}")
    assert_close(y_on, y_off, *NET_BOUND, "wino2d_epilogue off vs on")
