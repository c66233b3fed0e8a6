"""metrics.q2n, the float64 host definition of Q2n (Q4 / Q8 on blocks), which is unpinned: nothing outside this project is
available to compare it with.  It is held to independent statements of the published algorithm instead: the algebra of the
product, the one- and two-band cases written with real and complex arithmetic, explicit against implicit padding, and the
degenerate branches written out.  Then the C ABI's declarations and its limits, which need no GPU."""
import math

import numpy as np
import pytest

RAGGED = [(40, 72), (33, 32), (35, 70)]


def _pair(seed, c, h, w, noise=0.05):
    rng = np.random.default_rng(seed)
    t = rng.random((c, h, w))
    return t, t + noise * rng.standard_normal((c, h, w))


def _blocks(x, block=32, shift=32):
    """The windows of an image whose extents need no padding: {(j, i): [C, block * block]}."""
    c, h, w = x.shape
    return {(j, i): x[:, j * shift:j * shift + block, i * shift:i * shift + block].reshape(c, -1)
            for j in range((h - block) // shift + 1) for i in range((w - block) // shift + 1)}


def _normalised(g, f):
    """x, y of one block before the conjugation, for bands that are neither constant nor of mean zero."""
    a, s = g.mean(1, keepdims=True), g.std(1, ddof=1, keepdims=True)
    return (g - a) / s + 1.0, (f - a) / s + 1.0


# ---- 1. the product -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 2, 4, 8])
def test_product_norm_is_multiplicative(c):
    from tmdiff_amd.metrics import cd_mul
    rng = np.random.default_rng(c)
    for _ in range(20):
        p, r = rng.standard_normal(c), rng.standard_normal(c)
        got, want = np.linalg.norm(cd_mul(p, r)), np.linalg.norm(p) * np.linalg.norm(r)
        assert abs(got - want) <= 1e-12 * max(1.0, want), (c, got, want)


def test_product_of_two_components_is_complex():
    from tmdiff_amd.metrics import cd_mul
    rng = np.random.default_rng(7)
    for _ in range(20):
        p, r = rng.standard_normal(2), rng.standard_normal(2)
        z = complex(*p) * complex(*r)
        assert np.allclose(cd_mul(p, r), [z.real, z.imag], rtol=0, atol=1e-15)


@pytest.mark.parametrize("c", [8, 16])
def test_basis_vectors_multiply_to_signed_basis_vectors(c):
    from tmdiff_amd.metrics import cd_mul, cd_sign_table
    eye = np.eye(c)
    table = cd_sign_table(c)
    for i in range(c):
        for j in range(c):
            v = cd_mul(eye[i], eye[j])
            want = np.zeros(c)
            want[i ^ j] = v[i ^ j]
            assert abs(v[i ^ j]) == 1.0 and np.array_equal(v, want) and table[i, j] == v[i ^ j], (i, j, v)
    assert np.array_equal(table[0], np.ones(c)) and np.array_equal(table[:, 0], np.ones(c))      # e_0 is the unit
    assert np.array_equal(np.diag(table)[1:], -np.ones(c - 1))                                   # e_i^2 = -1
    assert np.array_equal(cd_sign_table(16)[:c, :c], table)                                      # the algebras are nested


def test_sixteen_components_have_no_multiplicative_norm():
    """Sedenions have zero divisors: what holds up to eight bands must not be assumed of sixteen."""
    from tmdiff_amd.metrics import cd_mul
    e = np.eye(16)
    assert np.array_equal(cd_mul(e[3] + e[10], e[6] - e[15]), np.zeros(16))


# ---- 2. identity --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", RAGGED)
@pytest.mark.parametrize("c", [1, 2, 3, 4, 6, 8, 16])
def test_identical_images_score_one(c, h, w):
    from tmdiff_amd.metrics import q2n
    x, _ = _pair(c, c, h, w)
    value, vals = q2n(x, x, hwc=False, return_map=True)
    assert abs(value - 1.0) <= 1e-12 and np.abs(vals - 1.0).max() <= 1e-12
    assert isinstance(value, float)


def test_layouts_agree():
    from tmdiff_amd.metrics import q2n
    t, p = _pair(3, 4, 64, 32)
    assert q2n(np.moveaxis(t, 0, -1), np.moveaxis(p, 0, -1)) == q2n(t, p, hwc=False)


# ---- 3. independent statements -------------------------------------------------------------------------------------------------
def test_one_band_is_the_universal_quality_index_of_the_normalised_block():
    from tmdiff_amd.metrics import q2n
    t, p = _pair(11, 1, 64, 96)
    _, vals = q2n(t, p, hwc=False, return_map=True)
    assert vals.shape == (2, 3)
    for (j, i), g in _blocks(t).items():
        x, y = _normalised(g, _blocks(p)[j, i])
        x, y = x[0], y[0]
        m1, m2 = x.mean(), y.mean()
        cov = np.sum((x - m1) * (y - m2)) / (x.size - 1.0)
        want = abs(4.0 * cov * m1 * m2 / ((x.var(ddof=1) + y.var(ddof=1)) * (m1 * m1 + m2 * m2)))
        assert abs(vals[j, i] - want) <= 1e-12, (j, i, vals[j, i], want)


def test_two_bands_are_the_complex_quality_index():
    """z1 = x_0 + i x_1, z2 = conj(y_0 + i y_1): |2 cov(z1, z2)| |2 m1 m2| / ((var z1 + var z2) (|m1|^2 + |m2|^2)), the
    covariance WITHOUT a conjugate on its second argument (the algebra's product, not the Hermitian one)."""
    from tmdiff_amd.metrics import q2n
    t, p = _pair(12, 2, 64, 96)
    _, vals = q2n(t, p, hwc=False, return_map=True)
    for (j, i), g in _blocks(t).items():
        x, y = _normalised(g, _blocks(p)[j, i])
        z1, z2 = x[0] + 1j * x[1], y[0] - 1j * y[1]
        n = z1.size
        m1, m2 = z1.mean(), z2.mean()
        cov = np.sum((z1 - m1) * (z2 - m2)) / (n - 1.0)
        var = (np.sum(np.abs(z1 - m1) ** 2) + np.sum(np.abs(z2 - m2) ** 2)) / (n - 1.0)
        want = abs(2.0 * cov) * 2.0 * abs(m1) * abs(m2) / (var * (abs(m1) ** 2 + abs(m2) ** 2))
        assert abs(vals[j, i] - want) <= 1e-12, (j, i, vals[j, i], want)


# ---- 4. padding ---------------------------------------------------------------------------------------------------------------
def test_mirror_padding_is_symmetric_padding():
    from tmdiff_amd.metrics import q2n
    t, p = _pair(13, 4, 40, 72)
    pad = ((0, 0), (0, 24), (0, 24))
    got, got_map = q2n(t, p, hwc=False, return_map=True)
    want, want_map = q2n(np.pad(t, pad, mode="symmetric"), np.pad(p, pad, mode="symmetric"), hwc=False, return_map=True)
    assert got_map.shape == (2, 3) and got == want and np.array_equal(got_map, want_map)
    assert np.array_equal(np.pad(t, pad, mode="symmetric")[:, 40 + 5, :72], t[:, 40 - 1 - 5])      # row H + k is row H - 1 - k


def test_band_padding_is_a_zero_band():
    from tmdiff_amd.metrics import q2n
    t, p = _pair(14, 3, 33, 32)
    zero = np.zeros((1, 33, 32))
    assert q2n(t, p, hwc=False) == q2n(np.concatenate([t, zero]), np.concatenate([p, zero]), hwc=False)
    t, p = _pair(15, 5, 32, 32)
    zero = np.zeros((3, 32, 32))
    assert q2n(t, p, hwc=False) == q2n(np.concatenate([t, zero]), np.concatenate([p, zero]), hwc=False)


@pytest.mark.parametrize("h,w,block,shift", [(40, 72, 32, 32), (33, 32, 32, 32), (20, 28, 8, 4), (12, 20, 16, 16), (64, 64, 32, 16)])
def test_map_shape(h, w, block, shift):
    from tmdiff_amd.metrics import q2n
    t, p = _pair(16, 2, h, w)
    value, vals = q2n(t, p, block, shift, hwc=False, return_map=True)
    assert vals.shape == (math.ceil(h / shift), math.ceil(w / shift)) and value == float(vals.mean())


def test_overlapping_blocks():
    from tmdiff_amd.metrics import q2n
    t, p = _pair(17, 4, 64, 64)
    _, fine = q2n(t, p, 32, 16, hwc=False, return_map=True)
    _, coarse = q2n(t, p, 32, 32, hwc=False, return_map=True)
    assert fine.shape == (4, 4) and coarse.shape == (2, 2)
    assert np.array_equal(fine[::2, ::2], coarse)
    # the blocks of row 3 start at row 48: rows 64 .. 79 are the mirror of rows 63 .. 48
    _, want = q2n(np.pad(t, ((0, 0), (0, 16), (0, 16)), mode="symmetric"), np.pad(p, ((0, 0), (0, 16), (0, 16)), mode="symmetric"),
                  32, 16, hwc=False, return_map=True)
    assert np.array_equal(fine, want[:4, :4])


# ---- 5. degenerate conventions --------------------------------------------------------------------------------------------------
def test_constant_ground_truth_band_stays_finite():
    from tmdiff_amd.metrics import q2n
    t, p = _pair(18, 4, 32, 64)
    t[2] = 0.5
    value, vals = q2n(t, p, hwc=False, return_map=True)
    assert np.isfinite(vals).all() and 0.0 <= value < 1e-20, value


def test_all_zero_ground_truth_band_is_shifted_only():
    """mean == 0 exactly: y = f + 1 without a division, x = 0 / 2^-52 + 1 = 1."""
    from tmdiff_amd.metrics import cd_mul, q2n
    t, p = _pair(19, 4, 32, 32)
    t[1] = 0.0
    g, f = t.reshape(4, -1), p.reshape(4, -1)
    x, y = _normalised(g[[0, 2, 3]], f[[0, 2, 3]])
    x = np.stack([x[0], np.ones(1024), x[1], x[2]])
    y = np.stack([y[0], -(f[1] + 1.0), -y[1], -y[2]])
    m1, m2 = x.mean(1), y.mean(1)
    e1, e2, k = np.sum(m1 * m1), np.sum(m2 * m2), 1024.0 / 1023.0
    t3 = k * np.mean(np.sum(x * x, 0)) + k * np.mean(np.sum(y * y, 0)) - k * (e1 + e2)
    q = (k * cd_mul(x, y).mean(1) - k * cd_mul(m1, m2)) * (2.0 * np.sqrt(e1 * e2) / (e1 + e2)) * 2.0 / t3
    want = float(np.sqrt(np.sum(q * q)))
    got = q2n(t, p, hwc=False)
    assert abs(got - want) <= 1e-12 and 0.5 < got < 1.0, (got, want)


def constant_pair(h=32, w=64):
    """Both images constant in every band, and the bias they score: bands 0 and 1 of the ground truth are zero (y = f + 1 = 1.25
    and -2), bands 2 and 3 agree in the two images (y = -1); x = 1 everywhere.  Every sum over such a block is exact, and the
    values are chosen so that k (4 + 7.5625) rounds to the sum of the rounded k 4 and k 7.5625 for k = n / (n - 1) of 8 x 8, 16 x 16
    and 32 x 32 blocks: t3 == 0 is an exact test (the original's), which other constants can miss by one rounding."""
    t, p = np.zeros((4, h, w)), np.zeros((4, h, w))
    p[0], p[1] = 0.25, 1.0
    t[2] = p[2] = 0.75
    t[3] = p[3] = 1.0
    e1, e2 = 4.0, 1.25 ** 2 + 2.0 ** 2 + 2.0
    return t, p, 2.0 * math.sqrt(e1 * e2) / (e1 + e2)


@pytest.mark.parametrize("block", [8, 16, 32])
def test_all_constant_images_give_the_bias(block):
    from tmdiff_amd.metrics import q2n
    t, p, want = constant_pair()
    value, vals = q2n(t, p, block, block, hwc=False, return_map=True)
    assert want < 0.96 and value == want and np.array_equal(vals, np.full((32 // block, 64 // block), want))
    assert q2n(t, t, block, block, hwc=False) == 1.0


# ---- 6. error cases -----------------------------------------------------------------------------------------------------------
def test_value_errors():
    from tmdiff_amd.metrics import q2n
    t, p = _pair(20, 2, 40, 40)
    for block, shift in ((1, 1), (0, 0), (32, 0), (32, 33), (8, -1)):
        with pytest.raises(ValueError):
            q2n(t, p, block, shift, hwc=False)
    q2n(t[:, :16, :16], p[:, :16, :16], 32, 32, hwc=False)                  # 16 mirrored rows of 16: the most
    with pytest.raises(ValueError):
        q2n(t[:, :15], p[:, :15], 32, 32, hwc=False)                        # 17 mirrored rows of 15
    with pytest.raises(ValueError):
        q2n(t[:, :, :15], p[:, :, :15], 32, 32, hwc=False)


def test_quality_is_for_device_tensors():
    import torch
    from tmdiff_amd import metrics
    t = torch.rand(1, 4, 32, 32)
    with pytest.raises(TypeError) as plain:
        metrics.quality(t, t)
    with pytest.raises(TypeError) as with_q2n:
        metrics.quality(t, t, q2n=True)
    assert str(plain.value) == str(with_q2n.value)


def test_val_dataset_refuses_q2n_without_the_device_path(tmp_path):
    from tmdiff_amd import evaluate
    with pytest.raises(ValueError):
        evaluate.val_dataset(None, "WV3", [], str(tmp_path), q2n=True)
    with pytest.raises(ValueError):
        evaluate.val_dataset(None, "WV3", [], str(tmp_path), device_metrics=True, full_resolution=True, q2n=True)
    assert not list(tmp_path.iterdir())


# ---- 7. ABI -------------------------------------------------------------------------------------------------------------------
NAMES = ("tmdiff_metrics_q2n", "tmdiff_metrics_q2n_workspace_bytes", "tmdiff_metrics_q2n_supported")


def test_entry_points_are_declared_exported_and_bound():
    import ctypes
    import os
    import re
    from conftest import ROOT
    from tmdiff_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmdiff_hip.h")).read(), flags=re.S)
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in include/tmdiff_hip.h"
        assert hasattr(dll, name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["tmdiff_metrics_q2n"][1]) == 17
    assert _lib.ABI_VERSION == 6


def test_supported_on_each_side_of_each_limit():
    from tmdiff_amd import ops
    ok = ops.metrics_q2n_supported
    assert ok(1, 16, 32, 32) and not ok(1, 17, 32, 32) and not ok(1, 0, 32, 32)
    assert ok(1, 4, 32, 32, 8, 8) and ok(1, 4, 32, 32, 16, 16) and not ok(1, 4, 32, 32, 12, 12) and not ok(1, 4, 64, 64, 64, 64)
    assert ok(1, 4, 32, 32, 16, 16) and not ok(1, 4, 32, 32, 16, 17)
    assert ok(1, 4, 32, 32, 16, 1) and not ok(1, 4, 32, 32, 16, 0)
    assert ok(1, 4, 16, 40, 32, 32) and not ok(1, 4, 15, 40, 32, 32)          # 16 mirrored rows of 16 / 17 of 15
    assert ok(1, 4, 40, 16, 32, 32) and not ok(1, 4, 40, 15, 32, 32)
    assert ok(1, 4, 16384, 32767, 32, 32) and not ok(1, 4, 16384, 32768, 32, 32)   # fewer than 2^31 elements
    assert ops.q2n_grid(40, 72, 32, 32) == (2, 3) and ops.q2n_grid(264, 264, 8, 4) == (66, 66)
    from tmdiff_amd import _lib
    assert _lib.lib.tmdiff_metrics_q2n_workspace_bytes(3, 8, 40, 72, 32, 32) == 3 * 6 * 8
    assert _lib.lib.tmdiff_metrics_q2n_workspace_bytes(3, 17, 40, 72, 32, 32) == 0


def test_entry_point_refuses_what_it_does_not_take():
    """The argument checks come before any launch and before the null-pointer check, so they run without a GPU."""
    from tmdiff_amd import _lib
    call = lambda c, h, w, block, shift: _lib.lib.tmdiff_metrics_q2n(None, 0, 0, None, 0, 0, 1, c, h, w, block, shift, None, None,
                                                                     None, 0, None)
    for args in ((17, 32, 32, 32, 32), (4, 32, 32, 12, 12), (4, 32, 32, 32, 0), (4, 15, 32, 32, 32)):
        assert call(*args) == -2, args
        assert b"metrics_q2n" in _lib.lib.tmdiff_last_error_string()
    assert call(4, 32, 32, 32, 32) == -1                                          # supported, but no tensors
