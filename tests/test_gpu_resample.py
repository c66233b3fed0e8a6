"""The resampling kernels (csrc/resample.hip) and the full-resolution loop built on them, on the GPU.

Bounds, with eps = 2^-24 and m = max|x|:
  pyr_down, two levels: 40 eps m.  Two levels x two passes x at most 9 roundings of values no larger than m are 36 roundings (the
    kernel's 5-tap sum has 5); a float32 restatement on the CPU measured 1.7 eps m.
  upsample_bilinear: 8 eps m.  Two lerps of at most 4 roundings each with exact weights (the kernel's lerp has 2: b - a, which
    may reach 2 m, and the fused multiply-add); a float32 restatement on the CPU measured 1.6 eps m.
  quality_fullres / val_dataset(full_resolution=True): 1e-9, the rule of tests/test_gpu_metrics.py -- the host functions are fed
    the device-made low-resolution PAN, so the two sides differ by the order of summation only."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_resample_host import pyr_down_statement

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
TOL = 1e-9

# (70, 132): the level-2 image is 18 x 33, two and three workgroup tiles of edge 16 with a ragged last one on either axis (the
# one-level kernel's tiles of edge 32 split its 35 x 66 image the same way); (6, 260): one ragged tile row, five tile columns
PYR_SHAPES = [(5, 5), (7, 9), (28, 28), (29, 31), (64, 64), (70, 132), (6, 260)]
UP_SHAPES = [(1, 1), (2, 3), (7, 9), (16, 16), (17, 65)]


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


def _rand(seed, *shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- pyr_down ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", PYR_SHAPES)
def test_pyr_down_against_the_statement(h, w):
    from tmdiff_amd import ops
    x = _rand(h * 1000 + w, 2, 3, h, w)
    xd = x.cuda()
    m = float(x.max())
    two = ops.pyr_down(xd)
    assert two.shape == (2, 3, *ops.pyr_down_shape(h, w)) and two.dtype == torch.float32
    for levels, got in ((2, two), (1, ops.pyr_down(xd, 1))):
        want = pyr_down_statement(x.numpy(), levels)
        assert tuple(got.shape) == want.shape
        err = np.abs(got.cpu().double().numpy() - want).max() / (EPS * m)
        print(f"pyr_down {h} x {w}, {levels} level(s): max error {err:.2f} eps m")
        assert err <= 40.0
    assert torch.equal(_bits(two), _bits(ops.pyr_down(ops.pyr_down(xd, 1), 1)))
    half = ops.pyr_down(torch.full_like(xd, 0.5))
    assert bool((half == 0.5).all())


def test_pyr_down_out_and_argument_checks():
    from tmdiff_amd import ops
    x = _rand(1, 2, 3, 29, 31).cuda()
    want = ops.pyr_down(x)
    out = torch.full((2, 3, 8, 8), -1.0, device="cuda")
    assert ops.pyr_down(x, out=out) is out and torch.equal(out, want)
    out.fill_(-1.0)
    ops.pyr_down(x, 2, out)                               # reuse
    assert torch.equal(out, want)
    one = torch.empty(2, 3, 15, 16, device="cuda")
    assert torch.equal(ops.pyr_down(ops.pyr_down(x, 1, out=one), 1), want)
    with pytest.raises(ValueError):
        ops.pyr_down(x, out=torch.empty(2, 3, 8, 9, device="cuda"))
    with pytest.raises(ValueError):
        ops.pyr_down(x, out=one)                          # the one-level shape
    with pytest.raises(ValueError):
        ops.pyr_down(torch.zeros(1, 1, 4, 4, device="cuda"), 2)
    assert ops.pyr_down(torch.zeros(1, 1, 4, 4, device="cuda"), 1).shape == (1, 1, 2, 2)
    with pytest.raises(ValueError):
        ops.pyr_down(x.transpose(2, 3))                   # not contiguous
    with pytest.raises(ValueError):
        ops.pyr_down(x.double())
    with pytest.raises(ValueError):
        ops.pyr_down(x, 3)
    with pytest.raises(ValueError):
        ops.pyr_down(x[0])


# ---- upsample_bilinear ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", UP_SHAPES)
@pytest.mark.parametrize("ratio", [2, 4])
def test_upsample_against_interpolate(h, w, ratio):
    from tmdiff_amd import ops
    x = _rand(h * 1000 + w + ratio, 2, 3, h, w)
    want = F.interpolate(x.double(), scale_factor=ratio, mode="bilinear", align_corners=False)
    got = ops.upsample_bilinear(x.cuda(), ratio)
    assert got.shape == want.shape == (2, 3, ratio * h, ratio * w) and got.dtype == torch.float32
    err = float((got.cpu().double() - want).abs().max()) / (EPS * float(x.max()))
    print(f"upsample x{ratio} {h} x {w}: max error {err:.2f} eps m")
    assert err <= 8.0
    half = ops.upsample_bilinear(torch.full((2, 3, h, w), 0.5, device="cuda"), ratio)
    assert bool((half == 0.5).all())
    # the 16-byte and the 4-byte store forms hold the same values: an output 4 bytes off a 16-byte boundary takes the second
    buf = torch.empty(got.numel() + 1, device="cuda")
    off = ops.upsample_bilinear(x.cuda(), ratio, out=buf[1:].view(got.shape))
    assert off.data_ptr() % 16 == 4 and torch.equal(_bits(off), _bits(got))


def test_upsample_argument_checks():
    from tmdiff_amd import ops
    x = _rand(2, 1, 2, 7, 9).cuda()
    with pytest.raises(ValueError):
        ops.upsample_bilinear(x, 3)
    with pytest.raises(ValueError):
        ops.upsample_bilinear(x, 4, out=torch.empty(1, 2, 28, 35, device="cuda"))
    with pytest.raises(ValueError):
        ops.upsample_bilinear(x.double(), 4)
    with pytest.raises(ValueError):
        ops.upsample_bilinear(x[:, :, ::2], 4)


# ---- quality_fullres -----------------------------------------------------------------------------------------------------------
def _fullres_case(seed, c, b=1):
    """(l_ms [b, c, 7, 7], pan [b, 1, 28, 28], ps [b, c, 28, 28]) in [0, 1], correlated as a fused product is."""
    g = torch.Generator().manual_seed(seed)
    pan = torch.rand(b, 1, 28, 28, generator=g)
    ps = (0.6 * pan + 0.4 * torch.rand(b, c, 28, 28, generator=g)).clamp(0, 1)
    l_ms = (F.avg_pool2d(ps, 4) + 0.02 * torch.randn(b, c, 7, 7, generator=g)).clamp(0, 1)
    return l_ms, pan, ps


def _host_noref(l_ms, pan, l_pan, ps):
    """NOREF_FIELDS of one image from the host definitions ([C, H, W] float32 CPU tensors)."""
    from tmdiff_amd import metrics as M
    a = [t.double().numpy() for t in (l_ms, pan, l_pan, ps)]
    return [M.d_lambda(a[0], a[3], hwc=False), M.d_s(*a, hwc=False), M.qnr(*a, hwc=False)]


def _close(got, want):
    return abs(got - want) <= TOL * max(1.0, abs(want))


@pytest.mark.parametrize("c", [4, 8])
def test_quality_fullres_against_the_host(c):
    from tmdiff_amd import metrics as M, ops
    l_ms, pan, ps = _fullres_case(40 + c, c, b=2)
    d = [t.cuda() for t in (l_ms, pan, ps)]
    got = M.quality_fullres(*d)
    assert tuple(got) == M.NOREF_FIELDS
    l_pan = ops.pyr_down(d[1], 2)
    assert l_pan.shape == (2, 1, 7, 7)
    same = M.quality_noref(d[0], d[1], l_pan, d[2])
    for i in range(2):
        want = _host_noref(l_ms[i], pan[i], l_pan[i].cpu(), ps[i])
        for k, w in zip(M.NOREF_FIELDS, want):
            g = float(got[k][i])
            print(f"quality_fullres C={c} [{i}] {k}: device {g!r} host {w!r} |diff| {abs(g - w):.2e}")
            assert _close(g, w), (k, g, w)
            assert float(same[k][i]) == g
    with pytest.raises(ValueError):
        M.quality_fullres(d[0][:, :, :6].contiguous(), d[1], d[2])
    with pytest.raises(ValueError):
        M.quality_fullres(torch.rand(2, c, 8, 8, device="cuda"), d[1], d[2])


def test_pyramid_and_metrics_in_one_captured_graph():
    """pyr_down(out=) then metrics_noref(out=, workspace=) captured on one stream as one chain; the inputs are overwritten in
    place and the replay equals the eager call on the new contents."""
    from tmdiff_amd import ops
    l_ms, pan, ps = (t.cuda() for t in _fullres_case(50, 4))
    l_pan = torch.empty(1, 1, 7, 7, device="cuda")
    out = torch.zeros(1, 3, device="cuda", dtype=torch.float64)
    ws = ops.metrics_workspace(*ps.shape, ps.device)

    def chain():
        ops.metrics_noref(l_ms, pan, ops.pyr_down(pan, 2, out=l_pan), ps, out=out, workspace=ws)

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        chain()                                           # warm-up on the capture stream
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        chain()
    first = out.clone()
    new = [t.cuda() for t in _fullres_case(51, 4)]
    for dst, src in zip((l_ms, pan, ps), new):
        dst.copy_(src)
    out.zero_()
    l_pan.zero_()
    graph.replay()
    torch.cuda.synchronize()
    want_pan = ops.pyr_down(new[1], 2)
    want = ops.metrics_noref(new[0], new[1], want_pan, new[2])
    assert torch.equal(_bits(l_pan), _bits(want_pan))
    assert torch.equal(out.view(torch.int64), want.view(torch.int64))
    assert not torch.equal(out, first)


# ---- val_dataset(full_resolution=True) -----------------------------------------------------------------------------------------
class _Trainer:
    """Stand-in for model.DDPM, as in tests/test_gpu_metrics.py: SR is a stack whose last image is the result."""

    def feed_data(self, d):
        self.d = d

    def test(self, continous=False, prompt="QB"):
        self.SR = torch.cat([torch.zeros_like(self.d["PS"]), self.d["PS"] * 1.25 - 0.1])     # leaves [0, 1]: the clamp acts

    def get_current_visuals(self):
        return {"SR": self.SR, "HR": self.d["HR"], "LR": self.d["LR"], "PAN": self.d["PAN"]}


def test_val_dataset_full_resolution(tmp_path):
    import scipy.io as scio
    from tmdiff_amd import evaluate, metrics as M, ops
    loader = []
    for seed in (60, 61):
        l_ms, pan, ps = _fullres_case(seed, 4)
        loader.append({"LR": l_ms.cuda(), "PAN": pan.cuda(), "PS": ps.cuda(), "HR": ps.cuda()})
    score = evaluate.val_dataset(_Trainer(), "GF2", loader, str(tmp_path / "full"), log=lambda *a: None, full_resolution=True)
    assert set(score) == {"d_lambda_GF2", "d_s_GF2", "qnr_GF2", "sec_per_item"}
    rows = []
    for item in loader:
        sr = (item["PS"] * 1.25 - 0.1).clamp(0, 1)
        l_pan = ops.pyr_down(item["PAN"], 2)
        rows.append(_host_noref(item["LR"][0].cpu(), item["PAN"][0].cpu(), l_pan[0].cpu(), sr[0].cpu()))
    for k, want in zip(M.NOREF_FIELDS, np.mean(rows, axis=0)):
        print(f"val_dataset full resolution {k}: device {score[f'{k}_GF2']!r} host {want!r}")
        assert _close(score[f"{k}_GF2"], float(want)), k
    for i, item in enumerate(loader):
        m = scio.loadmat(os.path.join(str(tmp_path / "full"), "GF2", f"output_mulExm_{i}.mat"))
        assert np.array_equal(m["sr"], evaluate.to_hwc01(item["PS"] * 1.25 - 0.1) * 1023.0)
    # the default is the host path against HR, as before: the same keys and the same numbers as a by-hand evaluation
    host = evaluate.val_dataset(_Trainer(), "GF2", loader, str(tmp_path / "host"), log=lambda *a: None)
    assert set(host) == {"ssim_GF2", "sam_GF2", "sec_per_item"}
    pairs = [(evaluate.to_hwc01(item["HR"]), evaluate.to_hwc01(item["PS"] * 1.25 - 0.1)) for item in loader]
    assert host["ssim_GF2"] == (0.0 + M.ssim(*pairs[0], 1) + M.ssim(*pairs[1], 1)) / 2
    assert host["sam_GF2"] == (0.0 + M.sam(*pairs[0]) + M.sam(*pairs[1])) / 2
    for i in range(2):
        a = scio.loadmat(os.path.join(str(tmp_path / "host"), "GF2", f"output_mulExm_{i}.mat"))["sr"]
        b = scio.loadmat(os.path.join(str(tmp_path / "full"), "GF2", f"output_mulExm_{i}.mat"))["sr"]
        assert a.dtype == b.dtype and np.array_equal(a, b)


# ---- fuse_scene ----------------------------------------------------------------------------------------------------------------
def test_fuse_scene():
    """The diffusion object of tests/test_gpu_tiled_fused.py at its smallest scene and tile: the tiny network, 8 bands, 32 x 48,
    tile 32, overlap 16."""
    from oracle import unet_ref as U
    from oracle.make_golden import TINY
    from tmdiff_amd import metrics as M, ops
    from tmdiff_amd.Hyper_unet_general import WavBEST
    from tmdiff_amd.diffusion_general import GeneralDiffusion
    from tmdiff_amd.tiling import fuse_scene, sample_tiled
    ref = U.fill_weights_(U.WavBESTRef(channels=TINY)).eval()
    net = WavBEST(channels=TINY)
    net.load_state_dict(ref.state_dict())
    net = net.cuda().eval()
    diff = GeneralDiffusion(net, "l1", noise_fn=lambda like: torch.randn(like.shape, dtype=torch.float32)).cuda()
    diff.set_new_noise_schedule({"schedule": "cosine", "n_timestep": 1000}, "cuda")
    lr_ms, pan = _rand(70, 1, 8, 8, 12).cuda(), _rand(71, 1, 1, 32, 48).cuda()
    kw = dict(tile=32, method="dpmsolver", steps=3, overlap=16)
    torch.manual_seed(11)
    got, scores = fuse_scene(diff, lr_ms, pan, "WV3", score=True, **kw)
    ms = ops.upsample_bilinear(lr_ms, 4)
    torch.manual_seed(11)
    want = sample_tiled(diff, {"MS": ms, "PAN": pan}, "WV3", **kw)
    assert got.shape == (1, 8, 32, 48) and torch.equal(got, want)
    torch.manual_seed(11)
    assert torch.equal(fuse_scene(diff, lr_ms, pan, "WV3", **kw), want)
    again = M.quality_fullres(lr_ms, pan, got)
    assert tuple(scores) == M.NOREF_FIELDS
    for k in M.NOREF_FIELDS:
        assert torch.equal(scores[k].view(torch.int64), again[k].view(torch.int64)), k
    with pytest.raises(ValueError):
        fuse_scene(diff, lr_ms, pan[:, :, :, :44].contiguous(), "WV3", **kw)
    with pytest.raises(ValueError):
        fuse_scene(diff, lr_ms, pan, "WV3", ratio=2, **kw)
    assert diff.denoise_fn is net
