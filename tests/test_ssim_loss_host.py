"""Host side of the SSIM loss term (no GPU): the C ABI of csrc/ssim_loss.hip as far as it can be checked without launching,
the float64 definition tmdiff_amd.losses.ssim_loss_host against metrics.ssim, the closed-form gradient the kernel implements
against autograd of the definition, and the `dssim` key of the `loss_terms` option."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

SYMBOLS = ("tmdiff_ssim_loss_supported", "tmdiff_ssim_loss_workspace_bytes", "tmdiff_ssim_loss")
I31 = 2 ** 31 - 1


def rand(seed, *shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported():
    from tmdiff_amd import _lib
    C = ctypes
    header = open(os.path.join(ROOT, "include", "tmdiff_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b(int|size_t)\s+%s\(" % name, header), f"{name} is not declared in include/tmdiff_hip.h"
        assert name in _lib.SIGNATURES, name
        assert getattr(raw, name) is not None
    vp = C.c_void_p
    assert _lib.SIGNATURES["tmdiff_ssim_loss_supported"] == (C.c_int, [C.c_int32] * 5)
    assert _lib.SIGNATURES["tmdiff_ssim_loss_workspace_bytes"] == (C.c_size_t, [C.c_int32] * 5)
    assert _lib.SIGNATURES["tmdiff_ssim_loss"] == (C.c_int, [vp] * 4 + [C.c_int32, C.c_double, C.c_double, C.c_int32] + [vp] * 4 +
                                                   [C.c_size_t] + [C.c_int32] * 4 + [vp])
    assert _lib.ABI_VERSION == 6
    # the new section follows the composite loss's, which stays as it was; the workspace formula and the limits are documented
    assert header.index("csrc/ssim_loss.hip") > header.index("int tmdiff_spectral_spatial_loss(")
    section = header[header.index("csrc/ssim_loss.hip"):header.index("int tmdiff_ssim_loss_supported")]
    for text in ("8 * B * C * ceil(H / 16) * ceil(W / 32)", "3 <= win <= 11", "H, W >= win", "2^31 - 1", "TMDIFF_E_UNSUPPORTED"):
        assert text in section, text


def expected_bytes(b, c, h, w):
    return 8 * b * c * (-(-h // 16)) * (-(-w // 32))


@pytest.mark.parametrize("b,c,h,w,win,ok", [
    (1, 1, 7, 7, 7, True), (2, 4, 9, 12, 7, True), (3, 17, 17, 33, 7, True), (1, 64, 64, 64, 7, True),
    (1, 1, 6, 9, 7, False), (1, 1, 9, 6, 7, False),                       # H = win - 1, W = win - 1
    (1, 1, 3, 3, 3, True), (1, 1, 2, 3, 3, False), (1, 1, 11, 11, 11, True), (1, 1, 10, 11, 11, False),
    (2, 4, 16, 16, 4, False), (2, 4, 16, 16, 6, False), (2, 4, 16, 16, 8, False), (2, 4, 16, 16, 10, False),      # even win
    (2, 4, 16, 16, 13, False), (2, 4, 16, 16, 1, False), (2, 4, 16, 16, 0, False), (2, 4, 16, 16, -7, False),
    (2, 0, 16, 16, 7, False), (0, 4, 16, 16, 7, False), (2, 4, 0, 16, 7, False),
    (2, 4, 16, 16, 5, True), (2, 4, 16, 16, 9, True),
    (1, 1, 7, I31 // 7, 7, True), (1, 1, 7, I31 // 7 + 1, 7, False), (1, 16, 11585, 11585, 7, True), (1, 16, 11586, 11585, 7, False),
])
def test_supported_and_workspace_at_the_documented_limits(b, c, h, w, win, ok):
    from tmdiff_amd import ops
    from tmdiff_amd._lib import lib
    assert (b * c * h * w <= I31) or not ok
    assert bool(lib.tmdiff_ssim_loss_supported(b, c, h, w, win)) is ok
    assert ops.ssim_loss_supported(b, c, h, w, win) is ok
    assert lib.tmdiff_ssim_loss_workspace_bytes(b, c, h, w, win) == (expected_bytes(b, c, h, w) if ok else 0)


def test_entry_point_refuses_without_launching():
    """Unsupported extents, window, data range or weight: TMDIFF_E_UNSUPPORTED before any pointer is looked at (all are NULL)."""
    from tmdiff_amd import _lib
    call = _lib.lib.tmdiff_ssim_loss
    unsupported, invalid = -2, -1            # TMDIFF_E_UNSUPPORTED, TMDIFF_E_INVALID (include/tmdiff_hip.h)
    for win, rng, wt, dims in ((8, 1.0, 1.0, (1, 1, 16, 16)), (7, 1.0, 1.0, (1, 1, 6, 16)), (13, 1.0, 1.0, (1, 1, 16, 16)), (7, 0.0, 1.0, (1, 1, 16, 16)),
                               (7, float("nan"), 1.0, (1, 1, 16, 16)), (7, float("inf"), 1.0, (1, 1, 16, 16)),
                               (7, 1.0, -1.0, (1, 1, 16, 16)), (7, 1.0, float("nan"), (1, 1, 16, 16)),
                               (7, 1.0, float("inf"), (1, 1, 16, 16)), (7, 1.0, 1.0, (1, 0, 16, 16))):
        assert call(None, None, None, None, win, rng, wt, 0, None, None, None, None, 0, *dims, None) == unsupported, (win, rng, wt)
    # supported extents with null tensors: another status (invalid), still no launch
    assert call(None, None, None, None, 7, 1.0, 1.0, 0, None, None, None, None, 0, 1, 1, 16, 16, None) == invalid


def test_ops_wrapper_checks_its_arguments_without_a_gpu():
    from tmdiff_amd import ops
    x = torch.zeros(1, 4, 6, 16)
    with pytest.raises(ValueError, match="H, W >= win"):
        ops.ssim_loss(x, x)
    x = torch.zeros(1, 4, 16, 16)
    with pytest.raises(ValueError, match="3 <= win <= 11"):
        ops.ssim_loss(x, x, win=8)
    with pytest.raises(ValueError, match="data_range"):
        ops.ssim_loss(x, x, data_range=0.0)
    with pytest.raises(ValueError, match="not negative"):
        ops.ssim_loss(x, x, weight=-1.0)
    with pytest.raises(ValueError, match="one shape"):
        ops.ssim_loss(x, x[:, :2])
    with pytest.raises(ValueError, match="accumulate"):
        ops.ssim_loss(x, x, accumulate=True)
    with pytest.raises(ValueError, match="contiguous float32 tensor on the GPU"):
        ops.ssim_loss(x, x)


# ---- the definition -------------------------------------------------------------------------------------------------------------
def test_host_definition_equals_metrics_ssim():
    """All planes have one shape, so the mean over images of metrics.ssim's per-plane means is the mean over all windows."""
    from tmdiff_amd import metrics as M
    from tmdiff_amd.losses import ssim_loss_host
    a, b = rand(1, 2, 4, 9, 12), rand(2, 2, 4, 9, 12)
    dssim, ssim = ssim_loss_host(a, b, win=7)
    want = sum(M.ssim(a[i], b[i], hwc=False) for i in range(2)) / 2
    assert ssim.dtype == torch.float64 and ssim.dim() == 0
    assert abs(float(ssim) - want) <= 1e-14 and -1.0 < want < 1.0 and want != 0.0
    assert float(dssim) == 1.0 - float(ssim)
    # float32 inputs are scored in float64, and another data range changes the constants alone
    d32, s32 = ssim_loss_host(a.float(), b.float())
    want32 = sum(M.ssim(a[i].float().double(), b[i].float().double(), hwc=False) for i in range(2)) / 2
    assert s32.dtype == torch.float64 and abs(float(s32) - want32) <= 1e-14
    want_r = sum(M.ssim(a[i], b[i], data_range=2.0, hwc=False) for i in range(2)) / 2
    assert abs(float(ssim_loss_host(a, b, data_range=2.0)[1]) - want_r) <= 1e-14 and abs(want_r - want) > 1e-4
    with pytest.raises(ValueError):
        ssim_loss_host(a[..., :6, :], b[..., :6, :])


@pytest.mark.parametrize("win", [3, 7, 11])
def test_identical_inputs_have_zero_dssim_exactly(win):
    from tmdiff_amd.losses import ssim_loss_host
    a = rand(3, 2, 3, 13, 14).float()
    dssim, ssim = ssim_loss_host(a, a.clone(), win=win)
    assert float(dssim) == 0.0 and float(ssim) == 1.0


@pytest.mark.parametrize("win,shape", [(7, (2, 4, 9, 12)), (3, (1, 2, 5, 6)), (11, (1, 3, 19, 14)), (7, (1, 1, 7, 7))])
def test_closed_form_gradient_equals_autograd_of_the_definition(win, shape):
    """The three per-window maps and the adjoint box filter of csrc/ssim_loss.hip, stated in torch operations
    (losses.ssim_grad_closed_form), against autograd of ssim_loss_host."""
    from tmdiff_amd.losses import ssim_grad_closed_form, ssim_loss_host
    a = rand(4, *shape)
    b = (a + 0.1 * torch.randn(*shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)).requires_grad_(True)
    dssim, _ = ssim_loss_host(a, b, win=win)
    want, = torch.autograd.grad(dssim, b)
    got = ssim_grad_closed_form(a, b, win=win)
    err = float((got - want).abs().max())
    print(f"win={win} {shape}: closed form against autograd, largest difference {err:.3e} (max |g| {float(want.abs().max()):.3e})")
    assert got.shape == want.shape and err <= 1e-14 and float(want.abs().max()) > 1e-4


# ---- the option -------------------------------------------------------------------------------------------------------------------
def test_loss_terms_accepts_dssim_and_builds_the_composite_module():
    from tmdiff_amd import losses
    from tmdiff_amd.diffusion_general import GeneralDiffusion
    net = torch.nn.Identity()
    d = GeneralDiffusion(net, "l1", loss_terms={"dssim": 0.2})
    d.set_loss("cpu")
    assert isinstance(d.loss_func, losses.SpectralSpatialLoss)
    assert (d.loss_func.base, d.loss_func.w_sam, d.loss_func.w_lap, d.loss_func.w_dssim) == ("l1", 0.0, 0.0, 0.2)
    d = GeneralDiffusion(net, "l2", loss_terms={"sam": 0.1, "lap": 0.5, "dssim": 2})
    d.set_loss("cpu")
    assert (d.loss_func.base, d.loss_func.w_sam, d.loss_func.w_lap, d.loss_func.w_dssim) == ("l2", 0.1, 0.5, 2.0)
    d = GeneralDiffusion(net, "l1", loss_terms={"sam": 0.1})
    d.set_loss("cpu")
    assert d.loss_func.w_dssim == 0.0 and losses.SpectralSpatialLoss("l1", 0.1, 0.5).w_dssim == 0.0
    assert losses.parse_loss_terms({"sam": 0.1, "lap": 0.5, "dssim": 0.2}) == (0.1, 0.5)
    assert losses.dssim_weight({"sam": 0.1, "dssim": 0.2}) == 0.2 and losses.dssim_weight({}) == 0.0
    assert losses.TERM_FIELDS5 == losses.TERM_FIELDS + ("dssim",)
    for bad in ({"dssim": -1}, {"dssim": float("nan")}, {"dssim": float("inf")}, {"dssim": "much"}, {"ssim": 1.0},
                {"dssim": 0.2, "ssim": 1.0}, {"dssim": 0.2, "tv": 1.0}):
        with pytest.raises(ValueError):
            GeneralDiffusion(net, "l1", loss_terms=bad)
    with pytest.raises(ValueError):
        losses.SpectralSpatialLoss("l1", 0.0, 0.0, w_dssim=-0.5)
    for bad in ({"win": 8}, {"win": 13}, {"win": 1}, {"data_range": 0.0}, {"data_range": float("inf")}):
        with pytest.raises(ValueError):
            losses.SSIMLoss(**bad)
    mod = losses.SSIMLoss()
    assert (mod.win, mod.data_range, mod.last_terms) == (7, 1.0, None)


def test_define_general_and_the_option_file_read_the_dssim_key(tmp_path):
    from oracle.make_golden import TINY
    from tmdiff_amd import config, networks
    from tmdiff_amd.losses import SpectralSpatialLoss
    opt = {"phase": "val", "model": {"unet": {"channel_multiplier": TINY},
                                     "diffusion": {"loss_type": "l1", "loss_terms": {"lap": 0.5, "dssim": 0.2}}}}
    net = networks.define_General(config.dict_to_nonedict(opt))
    net.set_loss("cpu")
    assert isinstance(net.loss_func, SpectralSpatialLoss)
    assert (net.loss_func.w_sam, net.loss_func.w_lap, net.loss_func.w_dssim) == (0.0, 0.5, 0.2)
    body = ('{"name": "t", "gpu_ids": [0], "path": {"log": "logs", "resume_state": null}, "datasets": {}, "train": {},\n'
            ' "model": {"beta_schedule": {}, "diffusion": {"loss_type": "l1", "loss_terms": %s}}} // comment\n')
    path = tmp_path / "opt.json"
    path.write_text(body % '{"sam": 0.1, "dssim": 0.2}')
    parsed = config.parse(str(path), "train", root=str(tmp_path), make_dirs=False)
    assert dict(parsed["model"]["diffusion"]["loss_terms"]) == {"sam": 0.1, "dssim": 0.2}
    for bad in ('{"dssim": -1}', '{"ssim": 1.0}'):
        path.write_text(body % bad)
        with pytest.raises(ValueError):
            config.parse(str(path), "train", root=str(tmp_path), make_dirs=False)
