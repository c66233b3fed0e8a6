"""Host side of the quality-metric suite (no GPU): the float64 definitions of tmdiff_amd/metrics.py against the reference's own
functions (tests/golden/metrics_suite.npz, tools/make_metrics_golden.py), their non-finite conventions, and the C ABI of the
device path as far as it can be checked without launching."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

CASES = ("wv3_f32", "gf2_f32", "wv3_f64")
RTOL = 1e-12          # both sides are fp64 evaluations of the same formula on the same float64 inputs


def _inputs(golden, tag):
    src, g = golden("metrics"), golden("metrics_suite")
    hr, sr = src[f"{tag}_hr"].astype(np.float64), src[f"{tag}_sr"].astype(np.float64)
    return hr, sr, g[f"{tag}_pan"], g[f"{tag}_l_pan"], g[f"{tag}_l_ms"]


@pytest.mark.parametrize("tag", CASES)
def test_host_functions_reproduce_the_reference(golden, tag):
    from tmdiff_amd import metrics as M
    g = golden("metrics_suite")
    hr, sr, pan, l_pan, l_ms = _inputs(golden, tag)
    got = {"rmse": M.rmse(hr, sr), "ergas": M.ergas(hr, sr), "ergas_swapped": M.ergas(sr, hr, ratio=0.5), "cc": M.cc(hr, sr),
           "scc": M.scc(hr, sr), "q": M.q_index(hr, sr), "d_lambda": M.d_lambda(l_ms, sr), "d_s": M.d_s(l_ms, pan, l_pan, sr),
           "qnr": M.qnr(l_ms, pan, l_pan, sr), "q_pop01": float(M._q_pop(sr[..., 0], sr[..., 1]))}
    if hr.shape[-1] == 4:
        got["q4"] = M.q4(hr, sr)
    assert ("q4" in got) == (f"{tag}_q4" in g.files)
    for k, v in got.items():
        want = float(g[f"{tag}_{k}"])
        print(f"{tag} {k}: {v!r} want {want!r} rel {abs(v - want) / abs(want):.2e}")
        assert abs(v - want) <= RTOL * abs(want), (tag, k, v, want)
    # ERGAS divides by the mean of its SECOND argument: swapping the arguments changes it
    assert abs(M.ergas(hr, sr) - M.ergas(sr, hr)) > 1e-6


def test_layouts_and_dtypes_agree(golden):
    """[C, H, W] tensors with hwc=False and float32 inputs (cast to float64 inside) give the [H, W, C] float64 value, up to the
    order in which NumPy adds the elements of differently laid out arrays (a few ulp)."""
    from tmdiff_amd import metrics as M
    hr, sr, pan, l_pan, l_ms = _inputs(golden, "gf2_f32")
    chw = lambda x: torch.from_numpy(np.ascontiguousarray(np.moveaxis(x, -1, 0)).astype(np.float32))
    same = lambda u, v: abs(u - v) <= 1e-14 * abs(v)
    for f in (M.rmse, M.ergas, M.cc, M.scc, M.q_index, M.q4):
        assert same(f(chw(hr), chw(sr), hwc=False), f(hr, sr)), f.__name__
    assert same(M.d_lambda(chw(l_ms), chw(sr), hwc=False), M.d_lambda(l_ms, sr))
    args = (chw(l_ms), torch.from_numpy(pan.astype(np.float32))[None], torch.from_numpy(l_pan.astype(np.float32))[None], chw(sr))
    assert same(M.d_s(*args, hwc=False), M.d_s(l_ms, pan, l_pan, sr))
    assert same(M.qnr(*args, hwc=False), M.qnr(l_ms, pan, l_pan, sr))
    assert M.PAIR_FIELDS == ("psnr", "sam", "ssim", "ergas", "rmse", "cc", "scc", "q", "q4")
    assert M.NOREF_FIELDS == ("d_lambda", "d_s", "qnr")


def test_non_finite_conventions():
    """Plain IEEE: a band that is constant in both images makes cc, scc and q_index NaN; identical images make mpsnr inf and
    leave rmse / ergas 0; only SAM replaces a non-finite per-pixel angle by 0."""
    from tmdiff_amd import metrics as M
    rng = np.random.default_rng(5)
    a = rng.random((12, 10, 3))
    b = np.clip(a + 0.05 * rng.standard_normal(a.shape), 0, 1)
    assert all(np.isfinite(f(a, b)) for f in (M.cc, M.scc, M.q_index, M.rmse, M.ergas))
    a[..., 1] = b[..., 1] = 0.5
    assert np.isnan(M.cc(a, b)) and np.isnan(M.scc(a, b)) and np.isnan(M.q_index(a, b))
    assert np.isfinite(M.rmse(a, b)) and np.isfinite(M.ergas(a, b)) and np.isfinite(M.ssim(a, b))
    assert M.mpsnr(a, a) == float("inf") and M.rmse(a, a) == 0.0 and M.ergas(a, a) == 0.0
    a[0, 0] = 0                                     # a zero spectrum: the angle is 0 / 0 -> counted as 0
    assert np.isfinite(M.sam(a, b))


def test_q4_needs_four_bands():
    from tmdiff_amd import metrics as M
    x = np.random.default_rng(1).random((8, 8, 8))
    for c in (1, 3, 5, 8):
        with pytest.raises(ValueError):
            M.q4(x[..., :c], x[..., :c])
    assert abs(M.q4(x[..., :4], x[..., :4]) - 1.0) < 1e-12


def test_quality_takes_device_tensors_only():
    from tmdiff_amd import metrics as M
    x = torch.rand(1, 4, 8, 8)
    with pytest.raises(TypeError):
        M.quality(x, x)
    with pytest.raises(TypeError):
        M.quality_noref(x[:, :, :2, :2], x[:, :1], x[:, :1, :2, :2], x)


def test_abi_declares_and_exports_the_metric_symbols():
    from tmdiff_amd import _lib
    names = ("tmdiff_metrics_supported", "tmdiff_metrics_workspace_bytes", "tmdiff_metrics_pair", "tmdiff_metrics_noref")
    header = open(os.path.join(ROOT, "include", "tmdiff_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/tmdiff_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 6


def test_metrics_supported_at_its_edges():
    """Predicate only: nothing is launched."""
    from tmdiff_amd import _lib, ops
    ok = ops.metrics_supported
    assert not ok(1, 0, 64, 64) and ok(1, 1, 64, 64) and ok(1, 16, 64, 64) and not ok(1, 17, 64, 64)
    assert not ok(1, 4, 6, 64) and ok(1, 4, 7, 64) and not ok(1, 4, 64, 6) and ok(1, 4, 64, 7) and ok(1, 1, 7, 7)
    assert ok(0, 4, 64, 64) and not ok(-1, 4, 64, 64)
    # 32-bit element offsets: 2^31 - 8 elements are taken, 2^31 are not (2^31 - 1 is prime: no extents reach it exactly)
    assert ok(1, 1, 8, 268435455) and not ok(1, 1, 8, 268435456)
    assert ok(1, 8, 16384, 16383) and not ok(1, 8, 16384, 16384) and not ok(2, 16, 8192, 8192) and ok(2, 16, 8192, 8191)
    wb = _lib.lib.tmdiff_metrics_workspace_bytes
    assert wb(1, 17, 64, 64) == 0 and wb(1, 4, 6, 64) == 0
    # one row of partials per 16 x 64 tile: 12 sums + 4 extremes per band, the angle sum, 16 cross products; fp64
    assert wb(3, 8, 1024, 1024) == 3 * (1024 // 16) * (1024 // 64) * (16 * 8 + 17) * 8
    assert wb(1, 4, 16, 16) >= 2 * 64 * (5 + 15) * 8                # small images: the two grams of the full-resolution set
