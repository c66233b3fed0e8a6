"""conv3d_w2 (csrc/conv3d_w2.hip): Winograd F(4,3) along the bands x F(2,3) along the width as transform passes plus one GEMM per
plane, against fp64 torch.nn.functional.conv3d on the CPU followed by the fp64 epilogue -- and, on the same inputs, the error of
conv3d_wf, the kernel these launches ran on before (printed; profiles/wino2d.txt holds both columns).

Shapes are small, not the workload's: B = 2, 128 -> 256 channels, planes 8x8x8 and 8x16x16, one 4-band case, one ragged plane
(8x12x10: five column pairs, a GEMM tile that ends inside a block of 32 positions -- but no last tile with fewer images than G:
Q = 4 = G there; test_gpu_conv3d_w2_edges.py has that and the other shape families).  The bound is the
one test_conv3d_winograd_in_kernel_transform and the fold tests hold, 2e-5 of the output's largest element, tightened to twice
the worst error this path measured on these cases (profiles/wino2d.txt): the nested transform adds one stage to conv3d_wf's."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = 6e-6     # 2 x the worst measured (2.9e-6, profiles/wino2d.txt); the ceiling is 2e-5
assert BOUND <= 2e-5

CASES = {      # name: (B, Cin, Cout, N, H, W, residual, keep_y, emit, prologue)
    "8x8x8 y2": (2, 128, 256, 8, 8, 8, False, False, True, False),
    "8x16x16 +res y y2": (2, 128, 256, 8, 16, 16, True, True, True, False),
    "8x16x16 y": (2, 128, 256, 8, 16, 16, False, True, False, False),
    "4x8x8 +res y": (2, 128, 256, 4, 8, 8, True, True, False, False),
    "8x12x10 +res y y2, prologue": (2, 128, 256, 8, 12, 10, True, True, True, True),
}


def _silu(t):
    return t * torch.sigmoid(t)


def _case(name):
    b, cin, cout, n, h, w, res, keep_y, emit, pro = CASES[name]
    g = torch.Generator().manual_seed(len(name) * 7 + h)
    t = dict(x=torch.randn(b, cin, n, h, w, generator=g), w=torch.randn(cout, cin, 3, 3, 3, generator=g) / (27 * cin) ** 0.5,
             bias=torch.randn(cout, generator=g) * 0.3)
    t["res"] = torch.randn(b, cout, n, h, w, generator=g) if res else None
    t["sh2"], t["sc2"] = (torch.randn(b, cout, generator=g) * 0.2, 1 + 0.1 * torch.randn(b, cout, generator=g)) if emit else (None, None)
    t["sh"], t["sc"] = (torch.randn(b, cin, generator=g) * 0.2, 1 + 0.1 * torch.randn(b, cin, generator=g)) if pro else (None, None)
    return t


_REF = {}


def _reference(name):
    """fp64: the prologue, the convolution, the epilogue y = (conv + bias + res) * out_scale, y2 = silu(y + sh2) * sc2"""
    if name not in _REF:
        t = _case(name)
        x = t["x"].double()
        if t["sh"] is not None:
            x = _silu(x + t["sh"].double()[:, :, None, None, None]) * t["sc"].double()[:, :, None, None, None]
        y = torch.nn.functional.conv3d(x, t["w"].double(), t["bias"].double(), padding=1)
        if t["res"] is not None:
            y = y + t["res"].double()
        y = y * 0.5
        y2 = None if t["sh2"] is None else _silu(y + t["sh2"].double()[:, :, None, None, None]) * t["sc2"].double()[:, :, None, None, None]
        _REF[name] = (y, y2)
    return _REF[name]


def _run(name, path):
    from tmdiff_amd import ops
    b, cin, cout, n, h, w, res, keep_y, emit, pro = CASES[name]
    t = _case(name)
    cu = lambda v: None if v is None else v.cuda().contiguous()
    kw = dict(bias=cu(t["bias"]), residual=cu(t["res"]), out_scale=0.5)
    if pro:
        kw.update(in_shift=cu(t["sh"]), in_scale=cu(t["sc"]), in_act=True)
    em = dict(act=True, shift=cu(t["sh2"]), scale=cu(t["sc2"])) if emit else None
    if path == "w2":
        out = ops.conv3d_w2(cu(t["x"]), ops.pack_conv_weight_w2(cu(t["w"])), cout, emit=em, keep_y=keep_y, **kw)
    elif w % 4 == 0:
        out = ops.conv3d_wf([cu(t["x"])], ops.pack_conv_weight_wino(cu(t["w"]), mode=2, planes=6), cout, emit=em, keep_y=keep_y, **kw)
    else:       # (conv3d_wf takes W % 4 == 0 only: such a plane ran on the direct kernel before)
        out = ops.conv3d([cu(t["x"])], ops.pack_conv_weight(cu(t["w"])), cout, 3, emit=em, keep_y=keep_y, **kw)
    torch.cuda.synchronize()
    y, y2 = (out if keep_y else None, None) if not emit else (out if keep_y else (None, out))
    return y, y2


def _err(got, want):
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("name", list(CASES))
def test_conv3d_w2_against_fp64(name):
    ry, ry2 = _reference(name)
    errs = {}
    for path in ("wf", "w2"):
        y, y2 = _run(name, path)
        errs[path] = max(_err(y, ry) if y is not None else 0.0, _err(y2, ry2) if y2 is not None else 0.0)
    was = "conv3d_wf" if CASES[name][5] % 4 == 0 else "conv3d (direct)"
    print(f"wino2d error [{name}]: {was} {errs['wf']:.3e}  conv3d_w2 {errs['w2']:.3e}")
    assert errs["w2"] <= BOUND, errs


def test_w2_weight_pack_is_the_kron_of_the_two_g_matrices():
    """Small-integer weights (multiples of 48: every entry of G_band (x) G_w times one is an integer) pack exactly."""
    from tmdiff_amd import ops
    cout, cin = 64, 8
    g = torch.Generator().manual_seed(3)
    w = 48.0 * torch.randint(-3, 4, (cout, cin, 3, 3, 3), generator=g).float()
    u = ops.pack_conv_weight_w2(w.cuda()).cpu().numpy().reshape(24, 3, cin // 4, cout, 4)
    gb = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
                   [0, 0, 1]])
    gw = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]])
    kr = np.kron(gb, gw)                                            # [kb * 4 + kw][dn * 3 + dw]
    wn = w.numpy().astype(np.float64)                               # [co][ci][dn][dh][dw]
    want = np.einsum("knw,oinhw->khoi", kr.reshape(24, 3, 3), wn)   # [k][dh][co][ci]
    assert np.abs(want - np.rint(want)).max() < 1e-9
    want = np.rint(want)
    got = u.transpose(0, 1, 3, 2, 4).reshape(24, 3, cout, cin)      # [k][dh][co][cq * 4 + e]
    assert np.array_equal(got, want.astype(np.float32))


def test_w2_transforms_with_identity_taps_reproduce_the_input():
    """A centre tap of one on the channel diagonal: the input pass and the output pass alone decide the result (the GEMM
    multiplies by the transformed unit taps), which is the input."""
    from tmdiff_amd import ops
    b, c, n, h, w = 1, 256, 8, 12, 10
    g = torch.Generator().manual_seed(11)
    x = torch.randn(b, c, n, h, w, generator=g)
    wt = torch.zeros(c, c, 3, 3, 3)
    wt[torch.arange(c), torch.arange(c), 1, 1, 1] = 1.0
    y = ops.conv3d_w2(x.cuda(), ops.pack_conv_weight_w2(wt.cuda()), c).cpu()
    err = float((y - x).abs().max() / x.abs().max())
    print(f"wino2d error [identity taps]: conv3d_w2 {err:.3e}")
    assert err <= BOUND, err


def test_conv3d_auto_routes_the_deep_layers_with_the_switch():
    """ops.config.wino2d sends a conv3d_wf launch of a routed shape to conv3d_w2 (same result within the bound); a launch off
    the shape rule (64 input channels) stays where it was."""
    import collections
    from tmdiff_amd import ops
    name = "8x8x8 y2"
    b, cin, cout, n, h, w, *_ = CASES[name]
    t = _case(name)
    x, wt = t["x"].cuda(), t["w"].cuda()
    weights = ops.ConvWeights(lambda: ops.pack_conv_weight(wt), lambda: ops.pack_conv_weight_wino(wt, mode=2, planes=6), None,
                              lambda: ops.pack_conv_weight_w2(wt))
    keep, ops.COUNTS = ops.COUNTS, collections.Counter()
    try:
        with ops.config.override(wino_min_blocks=1, wino2d=False):
            y0 = ops.conv3d_auto([x], weights, cout)
        with ops.config.override(wino_min_blocks=1, wino2d=True):
            y1 = ops.conv3d_auto([x], weights, cout)
            ops.conv3d_auto([x[:, :64].contiguous()], ops.ConvWeights(
                lambda: ops.pack_conv_weight(wt[:, :64].contiguous()),
                lambda: ops.pack_conv_weight_wino(wt[:, :64].contiguous(), mode=2, planes=6), None,
                lambda: ops.pack_conv_weight_w2(wt[:, :64].contiguous())), cout)     # Cin = 64: stays on conv3d_wf
        counts = dict(ops.COUNTS)
    finally:
        ops.COUNTS = keep
    assert counts == {"conv3d_wf_fwd": 2, "conv3d_w2_fwd": 1}, counts
    assert float((y1 - y0).abs().max() / y0.abs().max()) <= 2 * BOUND
