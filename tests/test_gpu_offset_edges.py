"""GPU tests of the convolution families at the edges of their 32-bit offset limits (tests/test_host_logic.py checks that the
entry points, support queries and routing agree on where those limits are).  Every family runs at the largest extents it
accepts -- where a descriptor span or a byte offset comes closest to 2^32 / 2^31 -- and, where the path changes, just past
the edge.  The reference is an fp64 convolution on the GPU (27 shifted fp64 matrix products, prologue and epilogue in fp64),
compared chunk by chunk over every element.  Every output is filled with NaN before the launch and followed by a guard of
sentinels: a dropped or misplaced store fails even where the kernel would have written zeros."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GIB = 1 << 30
BUDGET = 40 * GIB             # peak device memory of one test
GUARD = 4096                  # sentinel floats after every output
SENTINEL = 12345.0
MAX_REL, L2_REL = 2e-5, 2e-6  # fp32 tolerances of the existing tests


@pytest.fixture
def ops():
    from tmdiff_amd import ops
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()        # (what other tests' fixtures hold is not this test's)
    yield ops
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"\nPEAK {peak / GIB:.2f} GiB")
    torch.cuda.empty_cache()
    assert peak <= BUDGET, f"peak device memory {peak / GIB:.2f} GiB"


def guarded(shape, dtype=torch.float32):
    """(tensor of `shape` filled with NaN, the whole buffer): GUARD sentinels follow the tensor in the same allocation."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.empty(n + GUARD, device="cuda", dtype=dtype)
    if dtype == torch.int16:
        buf[:n].fill_(0x7FC0)           # bf16 NaN
        buf[n:].fill_(0x1234)
    else:
        buf[:n].fill_(float("nan"))
        buf[n:].fill_(SENTINEL)
    return buf[:n].view(shape), buf


def assert_guard(buf, n_guard=GUARD):
    tail = buf[-n_guard:]
    want = 0x1234 if buf.dtype == torch.int16 else SENTINEL
    assert bool((tail == want).all()), "a store landed past the end of an output"


class Err:
    """max-rel and rel-L2 of a tensor compared in chunks against an fp64 reference; NaN anywhere fails."""

    def __init__(self, what):
        self.what, self.max_err, self.max_ref, self.sq_err, self.sq_ref = what, 0.0, 0.0, 0.0, 0.0

    def add(self, got, ref):
        assert not bool(torch.isnan(got).any()), f"{self.what}: an element was never written (NaN left)"
        e = got.double() - ref
        self.max_err = max(self.max_err, float(e.abs().max()))
        self.max_ref = max(self.max_ref, float(ref.abs().max()))
        self.sq_err += float((e * e).sum())
        self.sq_ref += float((ref * ref).sum())

    def check(self, max_rel=MAX_REL, l2_rel=L2_REL):
        m, l2 = self.max_err / max(self.max_ref, 1e-30), (self.sq_err / max(self.sq_ref, 1e-300)) ** 0.5
        assert m <= max_rel and l2 <= l2_rel, f"{self.what}: max-rel {m:.3e} (<= {max_rel}), rel-L2 {l2:.3e} (<= {l2_rel})"


def conv_rows(x, w64, h0, h1):
    """fp64 3x3x3 convolution (padding 1) of x [Cin, N, H, W] (fp32, GPU) at the rows h0:h1: [Cout, N, h1 - h0, W]."""
    _, N, H, W = x.shape
    lo, hi = max(h0 - 1, 0), min(h1 + 1, H)
    xc = F.pad(x[:, :, lo:hi].double(), (1, 1, 1 if h0 == 0 else 0, 1 if h1 == H else 0, 1, 1))
    out = torch.zeros(w64.shape[0], N, h1 - h0, W, device=x.device, dtype=torch.float64)
    for dn in range(3):
        for dh in range(3):
            for dw in range(3):
                out += torch.einsum("oc,cnhw->onhw", w64[:, :, dn, dh, dw], xc[:, dn:dn + N, dh:dh + h1 - h0, dw:dw + W])
    return out


def row_chunks(N, H, W, positions=1 << 20, step=2):
    rows = max(step, positions // (N * W) // step * step)
    return [(h0, min(h0 + rows, H)) for h0 in range(0, H, rows)]


def launch(ops, fn, d, *args):
    ops.check(fn(C.byref(d), *args, ops.stream_ptr()), fn.__name__)
    torch.cuda.synchronize()


def rand(*shape, scale=1.0):
    return torch.randn(*shape, device="cuda") * scale


# ---- conv3d_wf at a plane of exactly 2^24 positions --------------------------------------------------------------------------
WF_PLANES = [(4, 2048, 2048), (8, 1024, 2048)]       # 16 x 16 tiles / 8 x 16 tiles


@pytest.mark.parametrize("nhw", WF_PLANES, ids=["4x2048x2048", "8x1024x2048"])
def test_offset_edge_wf_plane_2p24_outputs(ops, nhw):
    """conv3d_wf at plane = 2^24 (its limit), B = 2, 4 -> 64 channels: y and the second output with a residual, bias and
    out_scale -- sample 1 starts 4 GiB into each output."""
    torch.manual_seed(1)
    B, cin, cout, (N, H, W) = 2, 4, 64, nhw
    assert N * H * W == 1 << 24
    x, w = rand(B, cin, N, H, W), rand(cout, cin, 3, 3, 3, scale=(cin * 27) ** -0.5)
    bias, res = rand(cout), rand(B, cout, N, H, W)
    sh2, sc2 = rand(B, cout, scale=0.3), torch.rand(B, cout, device="cuda") + 0.5
    assert ops.routing.wf_route(B, cin, cout, N, H, W)[0]
    wp = ops.pack_conv_weight_wino(w, mode=2, planes=6)
    y, ybuf = guarded((B, cout, N, H, W))
    y2, y2buf = guarded((B, cout, N, H, W))
    d = ops.make_conv_desc([x], wp, cout, 3, y, y2=y2, bias=bias, residual=res, out_scale=0.75, y2_act=True, y2_shift=sh2,
                           y2_scale=sc2)
    assert ops.lib.tmdiff_conv3d_wf_supported(C.byref(d))
    launch(ops, ops.lib.tmdiff_conv3d_wf_fwd, d, None)
    assert_guard(ybuf)
    assert_guard(y2buf)
    e, e2, w64 = Err("y"), Err("y2"), w.double()
    for b in range(B):
        for h0, h1 in row_chunks(N, H, W):
            r = (conv_rows(x[b], w64, h0, h1) + bias.double()[:, None, None, None] + res[b, :, :, h0:h1].double()) * 0.75
            e.add(y[b, :, :, h0:h1], r)
            t = r + sh2[b].double()[:, None, None, None]
            e2.add(y2[b, :, :, h0:h1], t * torch.sigmoid(t) * sc2[b].double()[:, None, None, None])
    e.check()
    e2.check()


def test_offset_edge_wf_plane_2p24_ll_band(ops):
    """conv3d_wf at plane 2^24 writing the halved LL band of y (y_ll) beside the second output, no y."""
    torch.manual_seed(2)
    B, cin, cout, (N, H, W) = 2, 4, 64, (8, 1024, 2048)
    x, w = rand(B, cin, N, H, W), rand(cout, cin, 3, 3, 3, scale=(cin * 27) ** -0.5)
    bias = rand(cout)
    assert ops.routing.wf_route(B, cin, cout, N, H, W) == (True, 1)
    wp = ops.pack_conv_weight_wino(w, mode=2, planes=6)
    y2, y2buf = guarded((B, cout, N, H, W))
    yll, llbuf = guarded((B, cout, N, H // 2, W // 2))
    d = ops.make_conv_desc([x], wp, cout, 3, None, y2=y2, bias=bias, y_ll=yll)
    launch(ops, ops.lib.tmdiff_conv3d_wf_fwd, d, None)
    assert_guard(y2buf)
    assert_guard(llbuf)
    e2, el, w64 = Err("y2"), Err("y_ll"), w.double()
    for b in range(B):
        for h0, h1 in row_chunks(N, H, W):
            r = conv_rows(x[b], w64, h0, h1) + bias.double()[:, None, None, None]
            e2.add(y2[b, :, :, h0:h1], r)
            q = (r[..., 0::2, 0::2] + r[..., 0::2, 1::2] + r[..., 1::2, 0::2] + r[..., 1::2, 1::2]) * 0.25
            el.add(yll[b, :, :, h0 // 2:h1 // 2], q)
    e2.check()
    el.check()


def test_offset_edge_wf_plane_2p24_folded_res_conv(ops):
    """conv3d_wf at plane 2^24 with a folded 1x1x1 residual convolution of rc_cin = 32 channels (rc_x: 2 GiB per sample)."""
    torch.manual_seed(3)
    B, cin, cout, rc, (N, H, W) = 2, 4, 64, 32, (4, 2048, 2048)
    x, w = rand(B, cin, N, H, W), rand(cout, cin, 3, 3, 3, scale=(cin * 27) ** -0.5)
    xr, w1, bias = rand(B, rc, N, H, W), rand(cout, rc, 1, 1, 1, scale=rc ** -0.5), rand(cout)
    assert ops.routing.wf_fold_fits(B, cin, cout, N, H, W, rc)
    wp = ops.pack_conv_weight_wino(w, mode=2, planes=6)
    y, ybuf = guarded((B, cout, N, H, W))
    d = ops.make_conv_desc([x], wp, cout, 3, y, bias=bias, res_conv=(xr, w1, rc))
    launch(ops, ops.lib.tmdiff_conv3d_wf_fwd, d, None)
    assert_guard(ybuf)
    e, w64, w1d = Err("y"), w.double(), w1.double().view(cout, rc)
    for b in range(B):
        for h0, h1 in row_chunks(N, H, W):
            r = conv_rows(x[b], w64, h0, h1) + bias.double()[:, None, None, None]
            r += torch.einsum("oc,cnhw->onhw", w1d, xr[b, :, :, h0:h1].double())
            e.add(y[b, :, :, h0:h1], r)
    e.check()


def test_offset_edge_past_wf_plane_runs_elsewhere(ops):
    """One plane past 2^24: conv3d_wf refuses it, and conv3d_auto runs it on a family that takes it (the staged kernel)."""
    torch.manual_seed(4)
    B, cin, cout, (N, H, W) = 1, 4, 64, (4, 2048, 2052)
    assert not ops.routing.wf_route(B, cin, cout, N, H, W)[0]
    assert ops.routing.conv3_family(B, cin, cout, N, H, W) == "staged"
    x, w, bias = rand(B, cin, N, H, W), rand(cout, cin, 3, 3, 3, scale=(cin * 27) ** -0.5), rand(cout)
    y, ybuf = guarded((B, cout, N, H, W))
    ops.conv3d_auto([x], ops.ConvWeights(lambda: ops.pack_conv_weight(w), lambda: ops.pack_conv_weight_wino(w, mode=2, planes=6)),
                    cout, bias=bias, out=y)
    torch.cuda.synchronize()
    assert_guard(ybuf)
    e, w64 = Err("y"), w.double()
    for h0, h1 in row_chunks(N, H, W):
        e.add(y[0, :, :, h0:h1], conv_rows(x[0], w64, h0, h1) + bias.double()[:, None, None, None])
    e.check()


# ---- bf16: the dwordx4 epilogue just below 2^24 positions, the dword one at 2^24 ---------------------------------------------
def _bf16_round(t):
    return t.to(torch.bfloat16).float()


@pytest.mark.parametrize("nhw", [(8, 1024, 2044), (8, 1024, 2048)], ids=["below-2p24-dwordx4", "2p24-dword"])
def test_offset_edge_bf16_epilogues(ops, nhw):
    """bf16 operands / fp32 accumulation, Cout = 64 (64-channel tiles), residual and the packed bf16 second output, B = 2:
    against an fp64 convolution of the bf16-rounded operands."""
    torch.manual_seed(5)
    B, cin, cout, (N, H, W) = 2, 8, 64, nhw
    x, w = rand(B, cin, N, H, W), rand(cout, cin, 3, 3, 3, scale=(cin * 27) ** -0.5)
    bias, res = rand(cout), rand(B, cout, N, H, W)
    wp = ops.pack_conv_weight_bf16(w)
    y, ybuf = guarded((B, cout, N, H, W))
    y2, y2buf = guarded((B, cout // 8, N * H * W, 8), torch.int16)
    d = ops.make_conv_desc([x], wp, cout, 3, y, y2=y2, bias=bias, residual=res, out_scale=0.5)
    nb = ops.lib.tmdiff_conv3d_bf16_workspace_bytes(C.byref(d))
    assert nb
    ws = torch.empty(nb // 2, device="cuda", dtype=torch.int16)
    launch(ops, ops.lib.tmdiff_conv3d_fwd_bf16, d, ws.data_ptr())
    del ws
    assert_guard(ybuf)
    assert_guard(y2buf)
    e, e2, w64 = Err("y"), Err("y2 (bf16)"), _bf16_round(w).double()
    for b in range(B):
        xb = _bf16_round(x[b])
        for h0, h1 in row_chunks(N, H, W):
            r = (conv_rows(xb, w64, h0, h1) + bias.double()[:, None, None, None] + res[b, :, :, h0:h1].double()) * 0.5
            e.add(y[b, :, :, h0:h1], r)
            # (y2: bf16 units [Cout / 8, plane, 8]; channel = unit * 8 + k)
            g = y2[b].view(cout // 8, N, H, W, 8)[:, :, h0:h1].permute(0, 4, 1, 2, 3).reshape(cout, N, h1 - h0, W)
            e2.add(g.view(torch.bfloat16).float(), r)
    e.check(2e-3, 3e-4)                  # (tests/test_gpu_kernels.py::test_conv3d_bf16_operands_fp32_accumulate)
    e2.check(2 ** -7, 2 ** -8)           # (and bf16 rounding of the second output)


# ---- the direct kernels: vector epilogue at 2^23, dword past it; staged and fused at their plane limits -------------------------
@pytest.mark.parametrize("staged", [True, False], ids=["staged", "fused"])
@pytest.mark.parametrize("nhw", [(8, 1024, 1024), (8, 1024, 1032)], ids=["2p23-vector", "2p23+-dword"])
def test_offset_edge_direct_epilogues(ops, nhw, staged):
    """The direct kernels at plane 2^23 (the dwordx4 epilogue's last plane) and past it (the dword epilogue), Cout = 64, B = 2,
    with a residual and the second output."""
    torch.manual_seed(6)
    B, cin, cout, (N, H, W) = 2, 4, 64, nhw
    x, w = rand(B, cin, N, H, W), rand(cout, cin, 3, 3, 3, scale=(cin * 27) ** -0.5)
    bias, res, sh2 = rand(cout), rand(B, cout, N, H, W), rand(B, cout, scale=0.3)
    y, ybuf = guarded((B, cout, N, H, W))
    y2, y2buf = guarded((B, cout, N, H, W))
    d = ops.make_conv_desc([x], ops.pack_conv_weight(w), cout, 3, y, y2=y2, bias=bias, residual=res, out_scale=0.5, y2_act=True,
                           y2_shift=sh2)
    if staged:
        assert ops.lib.tmdiff_conv3d_fwd_staged_supported(C.byref(d))
        launch(ops, ops.lib.tmdiff_conv3d_fwd_staged, d, None)
    else:
        launch(ops, ops.lib.tmdiff_conv3d_fwd, d)
    assert_guard(ybuf)
    assert_guard(y2buf)
    e, e2, w64 = Err("y"), Err("y2"), w.double()
    for b in range(B):
        for h0, h1 in row_chunks(N, H, W):
            r = (conv_rows(x[b], w64, h0, h1) + bias.double()[:, None, None, None] + res[b, :, :, h0:h1].double()) * 0.5
            e.add(y[b, :, :, h0:h1], r)
            t = r + sh2[b].double()[:, None, None, None]
            e2.add(y2[b, :, :, h0:h1], t * torch.sigmoid(t))
    e.check()
    e2.check()


def test_offset_edge_staged_largest_plane(ops):
    """The staged kernel at the largest plane below 2^28 positions (plane * 8 < 2^31), 4 -> 32 channels, B = 1."""
    torch.manual_seed(7)
    B, cin, cout, (N, H, W) = 1, 4, 32, (8, 4096, 8188)
    assert ops.routing.direct_family(cin, cout, extents=(B, N, H, W)) == "staged"
    x, w = rand(B, cin, N, H, W), rand(cout, cin, 3, 3, 3, scale=(cin * 27) ** -0.5)
    y, ybuf = guarded((B, cout, N, H, W))
    ops.conv3d([x], ops.pack_conv_weight(w), cout, 3, out=y, staged=True)
    torch.cuda.synchronize()
    assert_guard(ybuf)
    e, w64 = Err("y"), w.double()
    for h0, h1 in row_chunks(N, H, W, 1 << 21):
        e.add(y[0, :, :, h0:h1], conv_rows(x[0], w64, h0, h1))
    e.check()


@pytest.mark.parametrize("cout", [1, 3])
def test_offset_edge_fused_largest_plane(ops, cout):
    """The fused kernel at the largest plane below 2^31 positions, 1 -> cout channels, B = 1 (8 GiB per channel)."""
    torch.manual_seed(8)
    B, cin, (N, H, W) = 1, 1, (8, 16384, 16382)
    x, w = rand(B, cin, N, H, W), rand(cout, cin, 3, 3, 3, scale=27 ** -0.5)
    y, ybuf = guarded((B, cout, N, H, W))
    ops.conv3d([x], ops.pack_conv_weight(w), cout, 3, out=y, staged=False)
    torch.cuda.synchronize()
    assert_guard(ybuf)
    e, w64 = Err("y"), w.double()
    for h0, h1 in row_chunks(N, H, W, 1 << 24):
        e.add(y[0, :, :, h0:h1], conv_rows(x[0], w64, h0, h1))
    e.check()


def test_offset_edge_fused_past_plane_raises(ops):
    """A plane of 2^31 positions is past every direct kernel: the public op raises instead of launching."""
    x = torch.empty(1, 1, 8, 16384, 16384, device="cuda")
    w = torch.zeros(1, 1, 3, 3, 3, device="cuda")
    from tmdiff_amd._lib import TmdiffError
    with pytest.raises(TmdiffError, match="plane too large"):
        ops.conv3d_auto([x], ops.ConvWeights(lambda: ops.pack_conv_weight(w)), 1)


# ---- conv3d_ll: Cin x plane just below 2^30 -------------------------------------------------------------------------------------
def test_offset_edge_ll_largest_input(ops):
    """Conv_0 + halved LL band as one strided convolution, 64 -> 64 channels at 8 x 1024 x 2046 (Cin x plane just below
    2^30), B = 2 (sample 1 starts 4 GiB into the input): against the fp64 convolution's 2 x 2 means."""
    torch.manual_seed(9)
    B, cin, cout, (N, H, W) = 2, 64, 64, (8, 1024, 2046)
    assert cin * N * H * W < (1 << 30) <= cin * N * H * (W + 2)
    assert ops.routing.ll_fits(B, cin, cout, N, H, W)
    x, w, bias = rand(B, cin, N, H, W), rand(cout, cin, 3, 3, 3, scale=(cin * 27) ** -0.5), rand(cout)
    y, ybuf = guarded((B, cout, N, H // 2, W // 2))
    d = ops.make_conv_desc([x], ops.pack_conv_weight_ll(w, 0.5), cout, 3, y, bias=bias, out_div=2)
    assert ops.lib.tmdiff_conv3d_ll_supported(C.byref(d))
    ops.check(ops.lib.tmdiff_conv3d_ll_fwd(C.byref(d), 0.5, ops.stream_ptr()), "conv3d_ll_fwd")
    torch.cuda.synchronize()
    assert_guard(ybuf)
    e, w64 = Err("y"), w.double()
    for b in range(B):
        for h0, h1 in row_chunks(N, H, W, 1 << 19):
            r = conv_rows(x[b], w64, h0, h1) + bias.double()[:, None, None, None]
            e.add(y[b, :, :, h0 // 2:h1 // 2], (r[..., 0::2, 0::2] + r[..., 0::2, 1::2] + r[..., 1::2, 0::2] + r[..., 1::2, 1::2]) * 0.25)
    e.check()


def test_offset_edge_wf_plane_2p24_haar_transform(ops):
    """conv3d_wf at plane 2^24 writing the whole Haar transform of y instead of y (y_hi): LL / 2 through the emit prologue, LH,
    HL, HH, B = 2 (8 bands: the only band count with a Haar output)."""
    torch.manual_seed(10)
    B, cin, cout, (N, H, W) = 2, 4, 64, (8, 1024, 2048)
    x, w = rand(B, cin, N, H, W), rand(cout, cin, 3, 3, 3, scale=(cin * 27) ** -0.5)
    bias, sh2, sc2 = rand(cout), rand(B, cout, scale=0.3), torch.rand(B, cout, device="cuda") + 0.5
    wp = ops.pack_conv_weight_wino(w, mode=2, planes=6)
    bands = [guarded((B, cout, N, H // 2, W // 2)) for _ in range(4)]
    d = ops.make_conv_desc([x], wp, cout, 3, None, bias=bias, y_ll=bands[0][0], y_hi=[t for t, _ in bands[1:]], y2_act=True,
                           y2_shift=sh2, y2_scale=sc2)
    launch(ops, ops.lib.tmdiff_conv3d_wf_fwd, d, None)
    for _, buf in bands:
        assert_guard(buf)
    errs, w64 = [Err(n) for n in ("LL'", "LH", "HL", "HH")], w.double()
    for b in range(B):
        for h0, h1 in row_chunks(N, H, W):
            r = conv_rows(x[b], w64, h0, h1) + bias.double()[:, None, None, None]
            a_, b_, c_, d_ = r[..., 0::2, 0::2], r[..., 0::2, 1::2], r[..., 1::2, 0::2], r[..., 1::2, 1::2]
            t = (a_ + b_ + c_ + d_) * 0.25 + sh2[b].double()[:, None, None, None]
            want = (t * torch.sigmoid(t) * sc2[b].double()[:, None, None, None], (a_ - b_ + c_ - d_) * 0.5,
                    (a_ + b_ - c_ - d_) * 0.5, (a_ - b_ - c_ + d_) * 0.5)
            for e, (got, _), ref in zip(errs, bands, want):
                e.add(got[b, :, :, h0 // 2:h1 // 2], ref)
    for e in errs:
        e.check()


# ---- the 1x1x1 bandwidth kernel ------------------------------------------------------------------------------------------------
def test_offset_edge_conv1_largest_plane(ops):
    """The 16-byte 1x1x1 bandwidth kernel at the largest plane below its limit (plane * 16 < 2^31), 16 -> 32 channels, B = 1."""
    torch.manual_seed(11)
    B, cin, cout, (N, H, W) = 1, 16, 32, (8, 4096, 4092)
    assert N * H * W * 16 < (1 << 31) <= N * H * (W + 4) * 16
    x, w, bias = rand(B, cin, N, H, W), rand(cout, cin, 1, 1, 1, scale=cin ** -0.5), rand(cout)
    y, ybuf = guarded((B, cout, N, H, W))
    ops.conv3d([x], ops.pack_conv_weight(w), cout, 1, out=y, bias=bias)
    torch.cuda.synchronize()
    assert_guard(ybuf)
    e, w2 = Err("y"), w.double().view(cout, cin)
    for h0, h1 in row_chunks(N, H, W, 1 << 23):
        e.add(y[0, :, :, h0:h1], torch.einsum("oc,cnhw->onhw", w2, x[0, :, :, h0:h1].double()) + bias.double()[:, None, None, None])
    e.check()


def test_offset_edge_conv1_side_xp_largest_sample(ops):
    """The bandwidth kernel writing the prologue output x' = SiLU(x + shift) of its input on the side, Cin x plane just below
    2^30 (64 channels at 4 x 2048 x 2044), B = 2: x' and y against fp64."""
    torch.manual_seed(12)
    B, cin, cout, (N, H, W) = 2, 64, 32, (4, 2048, 2044)
    assert cin * N * H * W < (1 << 30) <= cin * N * H * (W + 4)
    assert ops.routing.k1_side_xp(B, (cin,), cout, N, H, W)
    x, w, shift = rand(B, cin, N, H, W), rand(cout, cin, 1, 1, 1, scale=cin ** -0.5), rand(B, cin, scale=0.3)
    y, ybuf = guarded((B, cout, N, H, W))
    xp, xpbuf = guarded((B, cin, N, H, W))
    ops.conv3d([x], ops.pack_conv_weight(w), cout, 1, out=y, side_xp=dict(out=xp, shift=shift, act=True))
    torch.cuda.synchronize()
    assert_guard(ybuf)
    assert_guard(xpbuf)
    e, ex, w2 = Err("y"), Err("x'"), w.double().view(cout, cin)
    for b in range(B):
        for h0, h1 in row_chunks(N, H, W, 1 << 21):
            t = x[b, :, :, h0:h1].double() + shift[b].double()[:, None, None, None]
            ex.add(xp[b, :, :, h0:h1], t * torch.sigmoid(t))
            e.add(y[b, :, :, h0:h1], torch.einsum("oc,cnhw->onhw", w2, x[b, :, :, h0:h1].double()))
    ex.check()
    e.check()


# ---- weight gradients ------------------------------------------------------------------------------------------------------------
def _tap_sum(ga, xs):
    """sum over samples and positions of ga [S, o, W] (rows of g, see wgrad_reference) times xs [bs, c, N, R, W]: [o, c] -- one
    batched product per (sample, band, row), so that every product is short (fp64 GEMMs with one long inner dimension and a
    tiny output run on very few workgroups)."""
    return torch.bmm(ga, xs.permute(0, 2, 3, 4, 1).reshape(-1, xs.shape[-1], xs.shape[1])).sum(0)


def wgrad_reference(x, g, cout, cin, positions=1 << 20):
    """fp64 dL/dw [Cout, Cin, 3, 3, 3] and dL/dbias of a 3x3x3 convolution (padding 1) of x [B, Cin, N, H, W] given g."""
    B, _, N, H, W = x.shape
    dw = torch.zeros(cout, cin, 3, 3, 3, device=x.device, dtype=torch.float64)
    db = torch.zeros(cout, device=x.device, dtype=torch.float64)
    if N * H * W <= positions:             # small planes: whole samples, several at a time
        bs = positions // (N * H * W)
        chunks = [(b0, min(b0 + bs, B), 0, H) for b0 in range(0, B, bs)]
    else:
        chunks = [(b, b + 1, h0, h1) for b in range(B) for h0, h1 in row_chunks(N, H, W, positions, 1)]
    for b0, b1, h0, h1 in chunks:
        lo, hi = max(h0 - 1, 0), min(h1 + 1, H)
        xc = F.pad(x[b0:b1, :, :, lo:hi].double(), (1, 1, 1 if h0 == 0 else 0, 1 if h1 == H else 0, 1, 1))
        gc = g[b0:b1, :, :, h0:h1].double()
        db += gc.sum(dim=(0, 2, 3, 4))
        ga = gc.permute(0, 2, 3, 1, 4).reshape(-1, cout, W)
        for dn in range(3):
            for dh in range(3):
                for dwi in range(3):
                    dw[:, :, dn, dh, dwi] += _tap_sum(ga, xc[:, :, dn:dn + N, dh:dh + h1 - h0, dwi:dwi + W])
    return dw, db


def _run_wgrad(ops, fn, ws_fn, x, g, cout, cin):
    d = ops.make_conv_desc([x], 0, cout, 3, g)
    dw, dwbuf = guarded((cout, cin, 3, 3, 3))
    db, dbbuf = guarded((cout,))
    nb = ws_fn(C.byref(d))
    ws = torch.empty(max(16, nb) // 4, device="cuda", dtype=torch.float32)
    ops.check(fn(C.byref(d), g.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), ops.stream_ptr()), fn.__name__)
    torch.cuda.synchronize()
    del ws
    assert_guard(dwbuf)
    assert_guard(dbbuf)
    return d, dw, db


def _check_wgrad(dw, db, ref, max_rel=1e-5, l2_rel=1e-5):
    e, eb = Err("dw"), Err("dbias")
    e.add(dw, ref[0])
    eb.add(db, ref[1])
    e.check(max_rel, l2_rel)
    eb.check(1e-5, 1e-5)


def test_offset_edge_wgrad_direct_largest_plane(ops):
    """The direct weight gradient just below its plane limit (plane * 32 < 2^31: 6 x 4096 x 2730), 4 -> 32 channels, with the
    bias gradient (6 bands: the Winograd weight gradient does not take it)."""
    torch.manual_seed(13)
    B, cin, cout, (N, H, W) = 1, 4, 32, (6, 4096, 2730)
    assert N * H * W * 32 < (1 << 31) <= N * H * (W + 1) * 32
    x, g = rand(B, cin, N, H, W), rand(B, cout, N, H, W)
    d = ops.make_conv_desc([x], 0, cout, 3, g)
    assert not ops.wgrad_wino_takes(d)
    _, dw, db = _run_wgrad(ops, ops.lib.tmdiff_conv3d_wgrad_bias, ops.lib.tmdiff_conv3d_wgrad_workspace_bytes, x, g, cout, cin)
    _check_wgrad(dw, db, wgrad_reference(x, g, cout, cin))


@pytest.mark.parametrize("shape", [(1, 4, 4088, 4096), (8191, 16, 8, 8)], ids=["plane-4x4088x4096", "grid-B8191x16"])
def test_offset_edge_wgrad_wino_largest_shape(ops, shape):
    """The Winograd-domain weight gradient at the largest shapes ww_fits accepts along two axes: the 32-bit offsets of its
    transformed planes (one more row of tiles is refused) and the transform pass's grid (2 B T <= 65535), 4 -> 32 channels."""
    torch.manual_seed(14)
    B, N, H, W = shape
    cin, cout = 4, 32
    x, g = rand(B, cin, N, H, W), rand(B, cout, N, H, W)
    d = ops.make_conv_desc([x], 0, cout, 3, g)
    assert ops.lib.tmdiff_conv3d_wgrad_wino_supported(C.byref(d))
    e = ops.make_conv_desc([x[:1]], 0, cout, 3, g[:1])
    e.B, e.H = (B + 1, H) if B > 1 else (B, H + 8)
    assert not ops.lib.tmdiff_conv3d_wgrad_wino_supported(C.byref(e))          # (the edge: one more sample / row of tiles)
    _, dw, db = _run_wgrad(ops, ops.lib.tmdiff_conv3d_wgrad_wino_bias, ops.lib.tmdiff_conv3d_wgrad_wino_workspace_bytes, x, g,
                           cout, cin)
    # (each weight sums 2^26 products through the F(3,4) transforms in fp32: 1.1e-5 max-rel / 8e-6 rel-L2 measured at the plane
    #  edge; a misplaced offset or a dropped store is off by O(1))
    _check_wgrad(dw, db, wgrad_reference(x, g, cout, cin, 1 << 20), 2e-5, 1e-5)


# ---- abs_quantile_clamp --------------------------------------------------------------------------------------------------------
def quantile_reference(x, q, max_val):
    """(s [B], clamped x): torch.quantile's arithmetic -- rank q * (n - 1) in fp32, lerp weight rank - floor(rank), at::lerp in
    fp32 -- on an fp64 sort of |x| (torch.quantile refuses more than 2^24 elements); clamp(x, -s, s) / s rounded once."""
    B, n = x.shape
    a = x.abs().double().sort(dim=1).values
    rank = torch.tensor(q, dtype=torch.float32) * torch.tensor(float(n - 1), dtype=torch.float32)
    k = min(int(torch.floor(rank)), n - 1)
    frac = rank - torch.tensor(float(k), dtype=torch.float32)
    lo, hi = a[:, k].float(), a[:, min(k + 1, n - 1)].float()
    diff = hi - lo
    qv = lo + frac * diff if float(frac) < 0.5 else hi - diff * (1.0 - frac)
    s = torch.maximum(qv, torch.tensor(max_val, dtype=torch.float32, device=x.device))
    sd = s.double()[:, None]
    return s, (torch.minimum(torch.maximum(x.double(), -sd), sd) / sd).float()


def _quantile_case(ops, x, q, max_val):
    B, n = x.shape
    buf = torch.empty(B * n + GUARD, device="cuda", dtype=torch.float32)
    buf[B * n:].fill_(SENTINEL)
    t = buf[:B * n].view(B, n)
    t.copy_(x)
    s = ops.abs_quantile_clamp_(t, q, max_val)
    torch.cuda.synchronize()
    assert_guard(buf)
    want_s, want = quantile_reference(x, q, max_val)
    assert torch.equal(s, want_s), (s[:8], want_s[:8])
    assert torch.equal(t.view(torch.int32), want.view(torch.int32)), "clamped values differ (bits, the sign of zero included)"


def test_offset_edge_quantile_large_sample(ops):
    """n = 2^25 + 3 per sample (past torch.quantile's 2^24), B = 2."""
    torch.manual_seed(15)
    x = rand(2, (1 << 25) + 3)
    for q in (0.995, 0.5):
        _quantile_case(ops, x, q, 0.0)


def test_offset_edge_quantile_ties_equal_zeros_and_batch_caps(ops):
    """Heavy ties at ranks k and k + 1 (and a step between them), an all-equal sample, zeros with -0.0, B = 256 and 300 (the
    per-sample workgroup cap changes at 256) and n = 1."""
    torch.manual_seed(16)
    n = 4001                                              # rank q (n - 1) = 3980 at q = 0.995
    ties = torch.randint(0, 3, (4, n), device="cuda").float() * 0.5 - 0.5     # {-0.5, 0, 0.5}: ties everywhere
    step = torch.cat([torch.full((1, 3981), 0.25, device="cuda"), torch.full((1, n - 3981), 2.0, device="cuda")], 1)
    equal = torch.full((1, n), -0.7, device="cuda")
    zeros = torch.zeros(1, n, device="cuda")
    zeros[0, 0::2] = -0.0
    zeros[0, :7] = torch.tensor([3.0, -0.0, 0.0, -2.0, 0.0, -0.0, 1e-3])
    for q, max_val in ((0.995, 0.0), (0.5, 0.0), (0.99515, 0.1)):      # (0.99515: k = 3980, k + 1 = 3981 in `step`)
        _quantile_case(ops, torch.cat([ties, step, equal]), q, max_val)
    _quantile_case(ops, zeros, 0.5, 1.0)                  # quantile 0: s = max_val; -0.0 / 1 keeps its sign
    for B in (256, 300):
        _quantile_case(ops, rand(B, 70001), 0.995, 0.0)
    _quantile_case(ops, rand(3, 1), 0.995, 0.0)
    _quantile_case(ops, rand(3, 1), 0.0, 0.5)
