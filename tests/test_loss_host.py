"""Host side of the composite finetune loss (no GPU): the C ABI of csrc/loss.hip as far as it can be checked without
launching, the float64 definition tmdiff_amd.losses.spectral_spatial_loss_host against independent statements of its three
terms, and the `loss_terms` option of GeneralDiffusion / define_General."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

SYMBOLS = ("tmdiff_loss_supported", "tmdiff_loss_workspace_bytes", "tmdiff_spectral_spatial_loss")
I31 = 2 ** 31 - 1


def rand(seed, *shape, lo=0.0, hi=1.0):
    return lo + (hi - lo) * torch.rand(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported():
    from tmdiff_amd import _lib
    header = open(os.path.join(ROOT, "include", "tmdiff_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b(int|size_t)\s+%s\(" % name, header), f"{name} is not declared in include/tmdiff_hip.h"
        assert name in _lib.SIGNATURES, name
        assert getattr(raw, name) is not None
    for limit in ("1 <= C <= 16", "H, W >= 3", "2^31 - 1", "TMDIFF_E_UNSUPPORTED"):       # the limits are documented with them
        section = header[header.index("csrc/loss.hip"):header.index("int tmdiff_loss_supported")]
        assert limit in section, limit


def expected_bytes(b, h, w):
    return 24 * b * (-(-h // 16)) * (-(-w // 32))


@pytest.mark.parametrize("b,c,h,w,lap,ok", [
    (1, 16, 3, 3, 1, True), (1, 17, 3, 3, 1, False), (1, 16, 5, 5, 0, True), (1, 17, 5, 5, 0, False), (1, 0, 5, 5, 0, False),
    (2, 4, 2, 9, 1, False), (2, 4, 9, 2, 1, False), (2, 4, 2, 9, 0, True), (2, 4, 9, 2, 0, True), (2, 4, 1, 1, 0, True),
    (2, 4, 3, 9, 1, True), (2, 4, 9, 3, 1, True), (2, 4, 3, 3, 0, True), (2, 4, 0, 3, 0, False), (0, 4, 8, 8, 0, False),
    (1, 1, 1, I31, 0, True), (2, 1, 1, 2 ** 30, 0, False), (1, 1, 3, I31 // 3, 1, True), (1, 1, 3, I31 // 3 + 1, 1, False),
    (1, 16, 11585, 11585, 1, True), (1, 16, 11586, 11585, 1, False), (3, 8, 17, 33, 1, True),
])
def test_supported_and_workspace_at_the_documented_limits(b, c, h, w, lap, ok):
    from tmdiff_amd._lib import lib
    assert (b * c * h * w <= I31) or not ok
    assert bool(lib.tmdiff_loss_supported(b, c, h, w, lap)) is ok
    assert lib.tmdiff_loss_workspace_bytes(b, c, h, w, lap) == (expected_bytes(b, h, w) if ok else 0)


def test_ops_wrapper_names_the_limits_without_a_gpu():
    from tmdiff_amd import ops
    assert ops.loss_supported(1, 16, 3, 3) and not ops.loss_supported(1, 17, 3, 3) and not ops.loss_supported(1, 4, 2, 8, lap=True)
    x = torch.zeros(1, 17, 4, 4)
    with pytest.raises(ValueError, match="1 <= C <= 16"):
        ops.spectral_spatial_loss(x, x, x, "l1", 0.1, 0.5)
    x = torch.zeros(1, 4, 2, 8)
    with pytest.raises(ValueError, match="H, W >= 3"):
        ops.spectral_spatial_loss(x, x, x, "l1", 0.0, 0.5)
    x = torch.zeros(1, 4, 8, 8)
    with pytest.raises(ValueError, match="ms is needed"):
        ops.spectral_spatial_loss(x, x, None, "l1", 0.1, 0.0)
    with pytest.raises(ValueError, match="not negative"):
        ops.spectral_spatial_loss(x, x, x, "l1", -0.1, 0.0)
    with pytest.raises(ValueError, match="base"):
        ops.spectral_spatial_loss(x, x, x, "huber", 0.1, 0.0)
    with pytest.raises(ValueError, match="contiguous float32 tensor on the GPU"):
        ops.spectral_spatial_loss(x, x, x, "l1", 0.1, 0.5)


# ---- the definition against independent statements ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", [2, 4, 8])
def test_sam_term_is_the_mean_of_metrics_sam(c):
    """u = x0 + MS and v = xhat + MS are the images: the term in degrees is the batch mean of metrics.sam (pinned to the
    reference's SAM_numpy), which forms acos(dot / |v| / |u|), on random positive images.  There the angles are 0.01 .. 1 rad,
    where acos of a float64 cosine carries a few ulp / sin(angle) <= 1e-13: 1e-12 relative on the mean."""
    from tmdiff_amd import metrics as M
    from tmdiff_amd.losses import spectral_spatial_loss_host
    hr, sr, ms = rand(1, 3, c, 9, 11, lo=0.05), rand(2, 3, c, 9, 11, lo=0.05), rand(3, 3, c, 9, 11)
    total, base, sam, lap = spectral_spatial_loss_host(hr - ms, sr - ms, ms, "l1", 0.25, 0.0)
    want = np.mean([M.sam((hr[i] - ms[i] + ms[i]).numpy(), (sr[i] - ms[i] + ms[i]).numpy(), hwc=False) for i in range(3)])
    got = float(sam) * 180.0 / math.pi
    print(f"C={c}: sam {got!r} deg, metrics.sam {want!r}")
    assert abs(got - want) <= 1e-12 * abs(want) and want > 1.0
    assert float(lap) == 0.0 and float(total) == float(base) + 0.25 * float(sam)
    # the angle is taken on the images: the residuals alone give another number
    other = spectral_spatial_loss_host(hr - ms, sr - ms, torch.zeros_like(ms), "l1", 0.25, 0.0)[2]
    assert abs(float(other) - float(sam)) > 1e-3


def test_sam_term_with_one_band_is_zero_or_pi():
    from tmdiff_amd.losses import spectral_spatial_loss_host
    hr, sr, ms = rand(1, 2, 1, 5, 6, lo=0.05), rand(2, 2, 1, 5, 6, lo=0.05), rand(3, 2, 1, 5, 6)
    sr[0, 0, 0, :3] *= -1.0
    sam = spectral_spatial_loss_host(hr, sr, torch.zeros_like(ms), "l1", 1.0, 0.0)[2]
    assert abs(float(sam) - 3 * math.pi / 60) <= 1e-15


def test_lap_term_is_conv2d_with_the_stated_kernel():
    from tmdiff_amd.losses import spectral_spatial_loss_host
    x0, xh = rand(4, 2, 3, 7, 10, lo=-1.0), rand(5, 2, 3, 7, 10, lo=-1.0)
    k = torch.tensor([[1.0, 1.0, 1.0], [1.0, -8.0, 1.0], [1.0, 1.0, 1.0]], dtype=torch.float64).view(1, 1, 3, 3)
    d = (xh - x0).reshape(6, 1, 7, 10)
    want = F.conv2d(d, k).abs()
    assert tuple(want.shape) == (6, 1, 5, 8)
    total, base, sam, lap = spectral_spatial_loss_host(x0, xh, None, "l2", 0.0, 0.5)
    assert abs(float(lap) - float(want.mean())) <= 1e-13 * float(want.mean())
    assert float(sam) == 0.0 and float(total) == float(base) + 0.5 * float(lap)
    one = spectral_spatial_loss_host(x0[..., :3, :3], xh[..., :3, :3], None, "l1", 0.0, 1.0)[3]     # one interior pixel
    assert abs(float(one) - float(F.conv2d((xh - x0)[..., :3, :3].reshape(6, 1, 3, 3), k).abs().mean())) <= 1e-14
    with pytest.raises(ValueError):
        spectral_spatial_loss_host(x0[..., :2, :], xh[..., :2, :], None, "l1", 0.0, 1.0)


@pytest.mark.parametrize("base,ref", [("l1", torch.nn.L1Loss), ("l2", torch.nn.MSELoss), ("smooth_l1", torch.nn.SmoothL1Loss)])
def test_base_term_is_torchs_loss_in_float64(base, ref):
    from tmdiff_amd.losses import spectral_spatial_loss_host
    x0 = rand(6, 2, 4, 6, 6, lo=-2.0, hi=2.0)
    xh = rand(7, 2, 4, 6, 6, lo=-2.0, hi=2.0).requires_grad_(True)
    assert bool(((xh - x0).abs() > 1.0).any()) and bool(((xh - x0).abs() < 1.0).any())      # both branches of smooth l1
    total, b, sam, lap = spectral_spatial_loss_host(x0.float(), xh, None, base)
    want = ref()(xh, x0.float().double())
    assert abs(float(b) - float(want)) <= 1e-15 * float(want) and float(total) == float(b)
    g, = torch.autograd.grad(total, xh)
    gw, = torch.autograd.grad(want, xh)
    assert float((g - gw).abs().max()) <= 1e-16


def test_degenerate_pixels_contribute_their_angle_and_no_gradient():
    """Integer data: parallel and antiparallel spectra (|cross|^2 is exactly 0), a zero u, a zero v; nothing non-finite."""
    from tmdiff_amd.losses import spectral_spatial_loss_host
    u = torch.tensor([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [0.0, 0.0, 0.0], [1.0, 2.0, 3.0], [1.0, 0.0, 0.0]])
    v = torch.tensor([[3.0, 6.0, 9.0], [-2.0, -4.0, -6.0], [1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    ms = torch.tensor([0.0, 1.0, -2.0]).view(1, 3, 1, 1)
    x0 = (u.t().reshape(1, 3, 1, 6) - ms).double()
    xh = (v.t().reshape(1, 3, 1, 6) - ms).double().requires_grad_(True)
    total, _, sam, _ = spectral_spatial_loss_host(x0, xh, ms.expand(1, 3, 1, 6), "l1", 1.0, 0.0)
    assert abs(float(sam) - (math.pi + math.pi / 2) / 6) <= 1e-15
    g, = torch.autograd.grad(sam, xh)
    assert bool(torch.isfinite(g).all())
    assert float(g[..., :5].abs().max()) == 0.0
    # the last pixel: u = e0, v = e1; the gradient is -u_perp / |u_perp| / |v| / (number of pixels) = -e0 / 6
    assert torch.allclose(g[0, :, 0, 5], torch.tensor([-1.0 / 6, 0.0, 0.0], dtype=torch.float64), atol=1e-16)


def test_sam_gradient_is_minus_the_unit_perpendicular_over_v():
    from tmdiff_amd.losses import spectral_spatial_loss_host
    x0, ms = rand(8, 2, 5, 4, 4, lo=-0.5), rand(9, 2, 5, 4, 4)
    xh = rand(10, 2, 5, 4, 4, lo=-0.5).requires_grad_(True)
    sam = spectral_spatial_loss_host(x0, xh, ms, "l1", 1.0, 0.0)[2]
    g, = torch.autograd.grad(sam, xh)
    u, v = x0 + ms, xh.detach() + ms
    perp = u - (u * v).sum(1, keepdim=True) / (v * v).sum(1, keepdim=True) * v
    want = -perp / perp.norm(dim=1, keepdim=True) / v.norm(dim=1, keepdim=True) / 32.0
    assert float((g - want).abs().max()) <= 1e-13 * float(want.abs().max())
    assert float(((g * 32.0).norm(dim=1) * v.norm(dim=1) - 1.0).abs().max()) <= 1e-12


# ---- the option ---------------------------------------------------------------------------------------------------------------
def test_general_diffusion_loss_terms_option():
    from tmdiff_amd.diffusion_general import GeneralDiffusion
    from tmdiff_amd.losses import SpectralSpatialLoss
    net = torch.nn.Identity()
    for terms in (None, {}):
        for kind, cls in (("l1", torch.nn.L1Loss), ("l2", torch.nn.MSELoss), ("smooth_l1", torch.nn.SmoothL1Loss)):
            d = GeneralDiffusion(net, kind, loss_terms=terms)
            d.set_loss("cpu")
            assert type(d.loss_func) is cls and d.loss_terms is None
    assert GeneralDiffusion(net).loss_terms is None
    for terms, want in (({"sam": 0.1, "lap": 0.5}, (0.1, 0.5)), ({"sam": 0.2}, (0.2, 0.0)), ({"lap": 2}, (0.0, 2.0)),
                        ({"sam": 0.0, "lap": 0.0}, (0.0, 0.0))):
        d = GeneralDiffusion(net, "smooth_l1", loss_terms=terms)
        d.set_loss("cpu")
        assert isinstance(d.loss_func, SpectralSpatialLoss)
        assert (d.loss_func.base, d.loss_func.w_sam, d.loss_func.w_lap) == ("smooth_l1",) + want
        assert d.loss_func.last_terms is None
    for bad in ({"tv": 1.0}, {"sam": 0.1, "ssim": 1.0}, {"sam": -0.1}, {"lap": -1}, {"lap": float("nan")}, {"sam": "much"}):
        with pytest.raises(ValueError):
            GeneralDiffusion(net, "l1", loss_terms=bad)
    for terms in (None, {"sam": 0.1}):
        d = GeneralDiffusion(net, "huber", loss_terms=terms)
        with pytest.raises(NotImplementedError):
            d.set_loss("cpu")


def test_define_general_and_the_option_file_read_loss_terms(tmp_path):
    from oracle.make_golden import TINY
    from tmdiff_amd import config, networks
    from tmdiff_amd.losses import SpectralSpatialLoss
    opt = {"phase": "val", "model": {"unet": {"channel_multiplier": TINY}, "diffusion": {"loss_type": "l2"}}}
    plain = networks.define_General(opt)
    plain.set_loss("cpu")
    assert plain.loss_terms is None and type(plain.loss_func) is torch.nn.MSELoss
    opt["model"]["diffusion"]["loss_terms"] = {"sam": 0.1, "lap": 0.5}
    net = networks.define_General(config.dict_to_nonedict(opt))
    net.set_loss("cpu")
    assert isinstance(net.loss_func, SpectralSpatialLoss) and (net.loss_func.base, net.loss_func.w_sam, net.loss_func.w_lap) == ("l2", 0.1, 0.5)
    opt["model"]["diffusion"]["loss_terms"] = {"edge": 1.0}
    with pytest.raises(ValueError):
        networks.define_General(opt)
    # the option file: the key passes through parse() and is checked there
    body = ('{"name": "t", "gpu_ids": [0], "path": {"log": "logs", "resume_state": null}, "datasets": {}, "train": {},\n'
            ' "model": {"beta_schedule": {}, "diffusion": {"loss_type": "l1", "loss_terms": %s}}} // comment\n')
    path = tmp_path / "opt.json"
    path.write_text(body % '{"sam": 0.1, "lap": 0.5}')
    parsed = config.parse(str(path), "train", root=str(tmp_path), make_dirs=False)
    assert dict(parsed["model"]["diffusion"]["loss_terms"]) == {"sam": 0.1, "lap": 0.5}
    path.write_text(body % '{"sam": -1}')
    with pytest.raises(ValueError):
        config.parse(str(path), "train", root=str(tmp_path), make_dirs=False)
