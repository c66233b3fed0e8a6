"""CPU-only tests of the full-resolution loop's host side: the float64 definitions of the pyramid step and the bilinear
upsampling (tmdiff_amd/metrics.py) against independent statements of the same rules, the two new entry points in the header, the
library and the binding, and the argument checks of ``val_dataset(full_resolution=True)`` and ``LRHRDataset.has_gt``.

Neither definition is pinned to OpenCV itself: cv2 is not in this image.  ``pyr_down`` is held to scipy's correlation with
``mode="mirror"`` (which is reflect-101: d c b | a b c d | c b a), ``upsample_bilinear`` to torch's F.interpolate."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from scipy.ndimage import correlate1d

from conftest import ROOT

TAPS = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
PYR_SHAPES = [(5, 5), (7, 9), (28, 28), (29, 31), (12, 20)]


def pyr_down_statement(x, levels=2):
    """float64: per level the 5-tap correlation along both of the last two axes with a mirrored border, then every second pixel."""
    y = np.asarray(x, dtype=np.float64)
    for _ in range(levels):
        y = correlate1d(correlate1d(y, TAPS, axis=-1, mode="mirror"), TAPS, axis=-2, mode="mirror")[..., ::2, ::2]
    return y


def test_scipy_mirror_is_reflect_101():
    got = correlate1d(np.arange(5.0), np.array([1.0, 0, 0, 0, 0]), mode="mirror")       # picks x[i - 2]
    assert got.tolist() == [2.0, 1.0, 0.0, 1.0, 2.0]
    got = correlate1d(np.arange(5.0), np.array([0, 0, 0, 0, 1.0]), mode="mirror")       # picks x[i + 2]
    assert got.tolist() == [2.0, 3.0, 4.0, 3.0, 2.0]


@pytest.mark.parametrize("h,w", PYR_SHAPES)
def test_host_pyr_down_against_the_statement(h, w):
    from tmdiff_amd import metrics
    x = np.random.default_rng(h * 100 + w).random((2, 3, h, w))
    for levels in (1, 2):
        got, want = metrics.pyr_down(x, levels), pyr_down_statement(x, levels)
        eh, ew = h, w
        for _ in range(levels):
            eh, ew = (eh + 1) // 2, (ew + 1) // 2
        assert got.shape == want.shape == (2, 3, eh, ew) and got.dtype == np.float64
        err = np.abs(got - want).max()
        print(f"pyr_down {h} x {w}, {levels} level(s): max error {err:.3e}")
        assert err <= 1e-15
    assert np.array_equal(metrics.pyr_down(x, 2), metrics.pyr_down(metrics.pyr_down(x, 1), 1))
    assert np.array_equal(metrics.pyr_down(torch.from_numpy(x[0, 0]).float()), metrics.pyr_down(x[0, 0].astype(np.float32)))


def test_host_pyr_down_edges():
    from tmdiff_amd import metrics
    assert np.array_equal(metrics.pyr_down(np.full((9, 6), 0.5)), np.full((3, 2), 0.5))
    # one row of a known image: [1 4 6 4 1] / 16 around 0 with -1 -> 1, -2 -> 2
    x = np.tile(np.array([16.0, 0.0, 32.0, 0.0, 0.0]), (5, 1))
    assert metrics.pyr_down(x, 1)[0].tolist() == [(6 * 16 + 2 * 32) / 16, (16 + 6 * 32) / 16, (2 * 32) / 16]
    with pytest.raises(ValueError):
        metrics.pyr_down(np.zeros((4, 8)), 2)            # level 2 would see an extent of 2


@pytest.mark.parametrize("h,w", [(1, 1), (2, 3), (7, 9), (16, 16), (17, 65)])
@pytest.mark.parametrize("ratio", [2, 4])
def test_host_upsample_against_interpolate(h, w, ratio):
    from tmdiff_amd import metrics
    x = torch.rand(2, 3, h, w, generator=torch.Generator().manual_seed(h * 100 + w), dtype=torch.float64)
    want = F.interpolate(x, scale_factor=ratio, mode="bilinear", align_corners=False).numpy()
    got = metrics.upsample_bilinear(x, ratio)
    assert got.shape == want.shape == (2, 3, ratio * h, ratio * w) and got.dtype == np.float64
    err = np.abs(got - want).max()
    print(f"upsample x{ratio} {h} x {w}: max error {err:.3e}")
    assert err <= 1e-15
    assert np.array_equal(metrics.upsample_bilinear(np.full((h, w), 0.5), ratio), np.full((ratio * h, ratio * w), 0.5))


def test_entry_points_are_declared_exported_and_bound():
    from tmdiff_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmdiff_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("tmdiff_pyr_down", "tmdiff_upsample_bilinear"):
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in include/tmdiff_hip.h"
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == 7
    assert _lib.ABI_VERSION == 6


def test_entry_points_refuse_what_they_do_not_take():
    """Argument checks come before any launch, so they run without a GPU."""
    from tmdiff_amd import _lib
    lib = _lib.lib
    msg = lambda: lib.tmdiff_last_error_string().decode()
    assert lib.tmdiff_pyr_down(None, None, 1, 4, 8, 2, None) == -2 and ">= 5" in msg()
    assert lib.tmdiff_pyr_down(None, None, 1, 8, 2, 1, None) == -2
    assert lib.tmdiff_pyr_down(None, None, 1, 8, 8, 3, None) == -2
    assert lib.tmdiff_pyr_down(None, None, 2, 32768, 32768, 2, None) == -2 and "2^31" in msg()
    assert lib.tmdiff_upsample_bilinear(None, None, 1, 8, 8, 3, None) == -2 and "2 or 4" in msg()
    assert lib.tmdiff_upsample_bilinear(None, None, 8, 8192, 8192, 2, None) == -2 and "2^31" in msg()
    assert lib.tmdiff_pyr_down(None, None, -1, 8, 8, 2, None) == -1
    assert lib.tmdiff_pyr_down(None, None, 1, 8, 8, 2, None) == -1 and "null" in msg()
    assert lib.tmdiff_pyr_down(None, None, 0, 8, 8, 2, None) == 0
    assert lib.tmdiff_upsample_bilinear(None, None, 0, 8, 8, 4, None) == 0


def test_ops_refuse_host_tensors():
    from tmdiff_amd import metrics, ops
    with pytest.raises(ValueError):
        ops.pyr_down(torch.zeros(1, 1, 8, 8))
    with pytest.raises(ValueError):
        ops.upsample_bilinear(torch.zeros(1, 1, 8, 8))
    with pytest.raises(TypeError):
        metrics.quality_fullres(torch.zeros(1, 4, 7, 7), torch.zeros(1, 1, 28, 28), torch.zeros(1, 4, 28, 28))
    assert ops.pyr_down_shape(29, 31) == (8, 8) and ops.pyr_down_shape(29, 31, 1) == (15, 16)


class _Trainer:
    """Stand-in for model.DDPM: SR is a stack whose last image is the result; the visuals are what ``keys`` names."""

    def __init__(self, keys):
        self.keys = keys

    def feed_data(self, d):
        self.d = d

    def test(self, continous=False, prompt="QB"):
        self.SR = torch.cat([torch.zeros_like(self.d["MS"]), self.d["MS"]])

    def get_current_visuals(self):
        return {"SR": self.SR, **{k: self.d[k] for k in self.keys}}


@pytest.mark.parametrize("keys", [("HR",), ("HR", "LR"), ("HR", "PAN", "MS")])
def test_full_resolution_needs_lr_and_pan(tmp_path, keys):
    from tmdiff_amd import evaluate
    item = {"MS": torch.rand(1, 4, 28, 28), "HR": torch.rand(1, 4, 28, 28), "LR": torch.rand(1, 4, 7, 7), "PAN": torch.rand(1, 1, 28, 28)}
    with pytest.raises(ValueError, match="LR"):
        evaluate.val_dataset(_Trainer(keys), "GF2", [item], str(tmp_path), log=lambda *a: None, full_resolution=True)
    # without the switch the same visuals are scored as before
    score = evaluate.val_dataset(_Trainer(keys), "GF2", [item], str(tmp_path), log=lambda *a: None)
    assert set(score) == {"ssim_GF2", "sam_GF2", "sec_per_item"}


def test_dataset_says_whether_it_has_ground_truth():
    from tmdiff_amd.data import LRHRDataset
    g = np.random.default_rng(0)
    arrays = {"ms": g.random((2, 4, 4, 4)), "lms": g.random((2, 4, 16, 16)), "pan": g.random((2, 1, 16, 16))}
    full = LRHRDataset(arrays)
    assert full.has_gt is False and torch.equal(full[0]["HR"], full[0]["MS"])
    reduced = LRHRDataset({**arrays, "gt": g.random((2, 4, 16, 16))})
    assert reduced.has_gt is True and not torch.equal(reduced[0]["HR"], reduced[0]["MS"])
