"""The 23-tap polynomial interpolator on the GPU (csrc/resample.hip, ``ops.upsample_poly23``) and ``fuse_scene(interp="poly23")``.

Inputs: 2 x 3 planes of randn (tests/test_poly23_host.py, ``poly23_input``) at (1, 1), (2, 3), (5, 7) -- the extent is below the
filter's reach of 6, so coordinates wrap more than once --, (16, 16) -- exactly one 64 x 64 tile at x4 --, (17, 33) -- tile
remainders on both axes, two and three tiles at x4 --, (40, 24).  An odd w at x2 takes the scalar store path, an ``out=`` view
one element off 16-byte alignment takes it at every shape.

Tolerance against the float64 definition ``metrics.upsample_poly23``, with eps = 2^-24 and m = max|x|: a float32 restatement of
the kernel's arithmetic on the CPU (pair sums, then six fused multiply-adds from j = 5 down to 0, H then W, stage by stage;
``poly23_float32``) measured at most 1.725 eps m at x2 and 2.071 eps m at x4 over these inputs.  The device is held to 4 x that,
rounded up: 7 eps m at x2, 9 eps m at x4 (the margin covers the restatement's emulated fused multiply-add).  The worst-case bounds
-- 40 eps m at x2, 200 eps m at x4: four passes, an L1 gain of 1.6236 per pass -- are far above either.

Everything else is bit for bit: the copied samples, fused x4 against the two x2 stages, a rolled input against a rolled output
(circular borders; the shift carries content across tile edges), ``out=`` against the allocating call, the scalar against the
vector path."""
import numpy as np
import pytest
import torch

from test_poly23_host import EPS, GPU_TOL_EPS, POLY23_GPU_SHAPES, WORST_CASE_EPS, poly23_input

pytestmark = pytest.mark.gpu

CASES = [(2, 1), (2, 0), (4, 1)]          # (ratio, phase)


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _off_by_one(shape):
    """A contiguous float32 view of ``shape`` whose first element sits 4 bytes past a 16-byte boundary."""
    buf = torch.full((int(np.prod(shape)) + 1,), float("nan"), device="cuda")
    view = buf[1:].view(shape)
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4
    return view


@pytest.mark.parametrize("h,w", POLY23_GPU_SHAPES)
@pytest.mark.parametrize("ratio,phase", CASES)
def test_poly23_against_the_definition(h, w, ratio, phase):
    from tmdiff_amd import metrics, ops
    x = poly23_input(h, w)
    xd = x.cuda()
    m = float(x.abs().max())
    got = ops.upsample_poly23(xd, ratio, phase=phase)
    assert got.shape == (2, 3, ratio * h, ratio * w) and got.dtype == torch.float32
    want = metrics.upsample_poly23(x, ratio, phase)
    err = np.abs(got.cpu().double().numpy() - want).max() / (EPS * m)
    print(f"poly23 x{ratio} phase {phase} {h} x {w}: max error {err:.3f} eps m (tolerance {GPU_TOL_EPS[ratio]})")
    assert GPU_TOL_EPS[ratio] <= WORST_CASE_EPS[ratio]
    assert err <= GPU_TOL_EPS[ratio]
    # the samples are moved, not computed
    if ratio == 4:
        assert _same(got[..., 2::4, 2::4], xd)
    else:
        assert _same(got[..., phase::2, phase::2], xd)
    # out=: the same object, the same bits; one element off alignment: the scalar path, the same bits again
    out = torch.full_like(got, float("nan"))
    assert ops.upsample_poly23(xd, ratio, out=out, phase=phase) is out and _same(out, got)
    off = _off_by_one(got.shape)
    assert ops.upsample_poly23(xd, ratio, out=off, phase=phase) is off and _same(off, got)


@pytest.mark.parametrize("h,w", POLY23_GPU_SHAPES)
def test_poly23_fused_x4_is_the_two_stages(h, w):
    from tmdiff_amd import ops
    xd = poly23_input(h, w).cuda()
    fused = ops.upsample_poly23(xd, 4)
    half = ops.upsample_poly23(xd, 2, phase=1)
    assert _same(fused, ops.upsample_poly23(half, 2, phase=0))
    # the x2 image it never writes: the fused result's own samples at the even coordinates
    assert _same(fused[..., ::2, ::2], half)
    # ... and through the scalar path of either stage
    staged = ops.upsample_poly23(ops.upsample_poly23(xd, 2, out=_off_by_one(half.shape)), 2, out=_off_by_one(fused.shape), phase=0)
    assert _same(fused, staged)


@pytest.mark.parametrize("h,w,shift", [(17, 33, (3, 5)), (40, 24, (-9, 7)), (5, 7, (2, 3)), (1, 1, (1, 1))])
@pytest.mark.parametrize("ratio,phase", CASES)
def test_poly23_roll_equivariance(h, w, shift, ratio, phase):
    """Circular borders: a pixel's bits do not depend on the tile that makes it, nor on where the image wraps."""
    from tmdiff_amd import ops
    xd = poly23_input(h, w).cuda()
    got = ops.upsample_poly23(torch.roll(xd, shift, dims=(-2, -1)).contiguous(), ratio, phase=phase)
    want = torch.roll(ops.upsample_poly23(xd, ratio, phase=phase), (ratio * shift[0], ratio * shift[1]), dims=(-2, -1))
    assert _same(got, want)


def test_poly23_constant_and_limits():
    from tmdiff_amd import ops
    c = ops.upsample_poly23(torch.full((1, 2, 17, 33), 3.25, device="cuda"), 4)
    assert float((c / 3.25 - 1.0).abs().max()) <= 9 * EPS
    x = torch.zeros(1, 1, 8, 8, device="cuda")
    for bad in (dict(ratio=3), dict(ratio=4, phase=0), dict(ratio=2, phase=2), dict(out=torch.empty(1, 1, 32, 16, device="cuda"))):
        with pytest.raises(ValueError):
            ops.upsample_poly23(x, **bad)
    with pytest.raises(ValueError):
        ops.upsample_poly23(x.double())
    assert ops.upsample_poly23(torch.zeros(0, 3, 8, 8, device="cuda")).shape == (0, 3, 32, 32)


def test_poly23_captures_into_a_graph():
    """With out= nothing is allocated or synchronised."""
    from tmdiff_amd import ops
    xd = poly23_input(17, 33).cuda()
    want = ops.upsample_poly23(xd, 4)
    src, out = torch.zeros_like(xd), torch.zeros_like(want)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.upsample_poly23(src, 4, out=out)               # warm-up on the capture stream
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        ops.upsample_poly23(src, 4, out=out)
    src.copy_(xd)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _same(out, want)


def test_fuse_scene_poly23():
    """The set-up of tests/test_gpu_resample.py::test_fuse_scene: the tiny network, 8 bands, 32 x 48, tile 32, overlap 16."""
    from oracle import unet_ref as U
    from oracle.make_golden import TINY
    from tmdiff_amd import ops
    from tmdiff_amd.Hyper_unet_general import WavBEST
    from tmdiff_amd.diffusion_general import GeneralDiffusion
    from tmdiff_amd.tiling import fuse_scene, sample_tiled
    ref = U.fill_weights_(U.WavBESTRef(channels=TINY)).eval()
    net = WavBEST(channels=TINY)
    net.load_state_dict(ref.state_dict())
    net = net.cuda().eval()
    diff = GeneralDiffusion(net, "l1", noise_fn=lambda like: torch.randn(like.shape, dtype=torch.float32)).cuda()
    diff.set_new_noise_schedule({"schedule": "cosine", "n_timestep": 1000}, "cuda")
    g = torch.Generator().manual_seed(70)
    lr_ms, pan = torch.rand(1, 8, 8, 12, generator=g).cuda(), torch.rand(1, 1, 32, 48, generator=g).cuda()
    kw = dict(tile=32, method="dpmsolver", steps=3, overlap=16)

    def run(fn):
        torch.manual_seed(11)
        return fn()

    got = run(lambda: fuse_scene(diff, lr_ms, pan, "WV3", interp="poly23", **kw))
    ms = ops.upsample_poly23(lr_ms, 4)
    want = run(lambda: sample_tiled(diff, {"MS": ms, "PAN": pan}, "WV3", **kw))
    assert got.shape == (1, 8, 32, 48) and _same(got, want)
    default = run(lambda: fuse_scene(diff, lr_ms, pan, "WV3", **kw))
    assert _same(run(lambda: fuse_scene(diff, lr_ms, pan, "WV3", interp="bilinear", **kw)), default)
    assert _same(default, run(lambda: sample_tiled(diff, {"MS": ops.upsample_bilinear(lr_ms, 4), "PAN": pan}, "WV3", **kw)))
    assert not _same(got, default)
    with pytest.raises(ValueError, match="interp"):
        fuse_scene(diff, lr_ms, pan, "WV3", interp="cubic", **kw)
