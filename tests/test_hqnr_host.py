"""The float64 host definitions of HQNR (tmdiff_amd/metrics.py: uqi_blocks, d_s_block, pan_lowpass, d_lambda_k, hqnr).  They
are unpinned -- the Pansharpening Toolbox is not available to this project -- and are held here to independent statements: the
existing q_index on every window, the closed form of Q under scaling, explicit against implicit padding, the formulas written
out, a delta filter, and the registration of the interpolator.  Everything agrees to 1e-12 unless a test says otherwise."""
import numpy as np
import pytest

from tmdiff_amd import metrics as M

TOL = 1e-12
UNSUPPORTED = -2          # TMDIFF_E_UNSUPPORTED


def _rand(seed, *shape):
    return np.random.default_rng(seed).uniform(0.05, 1.0, shape)


def _delta(k=41):
    d = np.zeros((k, k))
    d[k // 2, k // 2] = 1.0
    return d


def test_single_window_is_q_index():
    for block in (8, 16, 32):
        a, b = _rand(1, 3, block, block), _rand(2, 3, block, block)
        got = M.uqi_blocks(a, b, block)
        assert got.shape == (3, 1, 1)
        for c in range(3):
            assert abs(got[c, 0, 0] - M.q_index(a[c], b[c], hwc=False)) <= TOL
        one = M.uqi_blocks(a, b[1], block)                                   # one band of b, shared
        for c in range(3):
            assert abs(one[c, 0, 0] - M.q_index(a[c], b[1], hwc=False)) <= TOL


def test_every_window_is_q_index_of_its_slice():
    a, b = _rand(3, 3, 64, 96), _rand(4, 3, 64, 96)
    got = M.uqi_blocks(a, b)
    assert got.shape == (3, 2, 3)
    for c in range(3):
        for j in range(2):
            for i in range(3):
                win = (slice(32 * j, 32 * j + 32), slice(32 * i, 32 * i + 32))
                assert abs(got[c, j, i] - M.q_index(a[c][win], b[c][win], hwc=False)) <= TOL
    hwc = M.uqi_blocks(np.moveaxis(a, 0, -1), np.moveaxis(b, 0, -1), hwc=True)
    assert np.array_equal(hwc, got)


def test_scaling():
    x = _rand(5, 2, 64, 32)
    assert np.abs(M.uqi_blocks(x, x) - 1.0).max() <= TOL
    for s in (0.5, 3.0):
        assert np.abs(M.uqi_blocks(x, s * x) - (2.0 * s / (1.0 + s * s)) ** 2).max() <= TOL


def test_padding():
    a, b = _rand(6, 2, 40, 72), _rand(7, 1, 40, 72)
    pad = ((0, 0), (0, 24), (0, 24))
    got = M.uqi_blocks(a, b)
    assert got.shape == (2, 2, 3)
    want = M.uqi_blocks(np.pad(a, pad, mode="symmetric"), np.pad(b, pad, mode="symmetric"))
    assert np.abs(got - want).max() <= TOL
    with pytest.raises(ValueError, match="mirrored"):
        M.uqi_blocks(np.ones((1, 8, 8)), np.ones((1, 8, 8)), 32)
    with pytest.raises(ValueError, match="mirrored"):
        M.q2n_grid(8, 8, 32, 32)
    with pytest.raises(ValueError):
        M.uqi_blocks(a, _rand(8, 3, 40, 72))                                  # neither one band nor two


def test_d_s_block():
    pan, pan_lp = _rand(9, 1, 64, 96), _rand(10, 1, 64, 96)
    assert M.d_s_block(np.repeat(pan, 4, 0), np.repeat(pan_lp, 4, 0), pan, pan_lp) == 0.0
    ps, ms = _rand(11, 4, 64, 96), _rand(12, 4, 64, 96)
    ps, ms = 0.5 * ps + 0.5 * pan, 0.5 * ms + 0.5 * pan_lp                     # correlated with the PAN, as real bands are
    hi = np.array([[M.q_index(ps[c, 32 * j:32 * j + 32, 32 * i:32 * i + 32], pan[0, 32 * j:32 * j + 32, 32 * i:32 * i + 32],
                              hwc=False) for j in range(2) for i in range(3)] for c in range(4)]).mean(1)
    lo = np.array([[M.q_index(ms[c, 32 * j:32 * j + 32, 32 * i:32 * i + 32], pan_lp[0, 32 * j:32 * j + 32, 32 * i:32 * i + 32],
                              hwc=False) for j in range(2) for i in range(3)] for c in range(4)]).mean(1)
    d = np.abs(hi - lo)
    assert d.max() > 1e-3
    assert abs(M.d_s_block(ps, ms, pan, pan_lp) - d.sum() / 4.0) <= TOL
    assert abs(M.d_s_block(ps, ms, pan, pan_lp, q=2) - np.sqrt((d * d).sum() / 4.0)) <= TOL
    val, mh, ml = M.d_s_block(ps, ms, pan, pan_lp, return_maps=True)
    assert mh.shape == ml.shape == (4, 2, 3)
    assert np.abs(mh.mean((1, 2)) - hi).max() <= TOL and np.abs(ml.mean((1, 2)) - lo).max() <= TOL
    assert abs(val - np.abs(mh.mean((1, 2)) - ml.mean((1, 2))).mean()) <= TOL
    with pytest.raises(ValueError):
        M.d_s_block(ps, ms, pan, pan_lp, q=0)


def test_d_lambda_k():
    ps, ms = _rand(13, 4, 64, 64), _rand(14, 4, 64, 64)
    assert abs(M.d_lambda_k(ps, ms, "QB", taps=_delta()) - (1.0 - M.q2n(ms, ps, hwc=False))) <= TOL
    # One band: Q2n is |UIQI| of the block NORMALISED by the ground truth's mean a and deviation s (tests/test_q2n_host.py),
    # x = (g - a) / s + 1, y = (f - a) / s + 1.  Covariance and variances scale alike, so that equals the UIQI of the raw block
    # when mean(y) / (1 + mean(y)^2) == a mean(f) / (a^2 + mean(f)^2), i.e. when the two windows have the same mean (or s == a),
    # and the index is positive.  The statement is made on such a pair, and in its general form on any pair.
    taps = M.mtf_kernel(0.3, 4)
    filtered = M.fir_decimate(ps[:1], taps, 1)
    noise = _rand(21, 1, 64, 64) - 0.5
    blocks = lambda t: t.reshape(1, 2, 32, 2, 32)
    same_mean = 0.3 * (blocks(noise) - blocks(noise).mean((2, 4), keepdims=True)) + blocks(filtered)
    same_mean = same_mean.reshape(1, 64, 64)
    raw = M.uqi_blocks(same_mean, filtered)
    assert (raw > 0.05).all() and (raw < 0.95).all()
    assert abs(M.d_lambda_k(ps[:1], same_mean, 0.3) - (1.0 - raw.mean())) <= TOL
    g = blocks(ms[:1])
    a, s = g.mean((2, 4), keepdims=True), g.std((2, 4), ddof=1, keepdims=True)
    x, y = ((g - a) / s + 1.0).reshape(1, 64, 64), ((blocks(filtered) - a) / s + 1.0).reshape(1, 64, 64)
    assert abs(M.d_lambda_k(ps[:1], ms[:1], 0.3) - (1.0 - np.abs(M.uqi_blocks(x, y)).mean())) <= TOL
    # the table is looked up per band; the image equal to the filtered fused image scores 0
    table = np.stack([M.mtf_kernel(g, 4) for g in M.MTF_GAINS["QB"][0]])
    assert abs(M.d_lambda_k(ps, M.fir_decimate(ps, table, 1), "QB")) <= TOL
    assert M.d_lambda_k(ps, ms, "QB") == M.d_lambda_k(ps, ms, M.MTF_GAINS["QB"][0]) == M.d_lambda_k(ps, ms, None, taps=table)
    # the ratio only shapes the filter: no decimation at ratio 2 either
    table2 = np.stack([M.mtf_kernel(g, 2) for g in M.MTF_GAINS["QB"][0]])
    assert abs(M.d_lambda_k(ps, M.fir_decimate(ps, table2, 1), "QB", ratio=2)) <= TOL
    with pytest.raises(ValueError):
        M.d_lambda_k(ps[:3], ms[:3], "QB")                                    # four gains for three bands


def test_pan_lowpass():
    p = _rand(15, 1, 32, 48)
    assert np.array_equal(M.pan_lowpass(p, 0.15, 4)[..., 2::4, 2::4], M.mtf_degrade(p, 0.15, 4, pan=True))
    assert np.array_equal(M.pan_lowpass(p, 0.15, 2)[..., 1::2, 1::2], M.mtf_degrade(p, 0.15, 2, pan=True))
    assert np.array_equal(M.pan_lowpass(p, "QB"), M.pan_lowpass(p, M.MTF_GAINS["QB"][1]))
    assert M.pan_lowpass(p[0], "QB").shape == (32, 48) and M.pan_lowpass(p, "QB").shape == (1, 32, 48)
    for shape, ratio in (((1, 30, 48), 4), ((1, 32, 46), 4), ((1, 31, 48), 2), ((1, 32, 48), 3), ((2, 32, 48), 4)):
        with pytest.raises(ValueError):
            M.pan_lowpass(np.ones(shape), 0.15, ratio)


def test_hqnr():
    pan = _rand(16, 1, 64, 64)
    ms = 0.6 * _rand(17, 4, 64, 64) + 0.4 * M.pan_lowpass(pan, "QB")
    ps = 0.6 * ms + 0.4 * pan
    dl, ds = M.d_lambda_k(ps, ms, "QB"), M.d_s_block(ps, ms, pan, M.pan_lowpass(pan, "QB"))
    assert 0.0 < dl < 1.0 and 0.0 < ds < 1.0
    for alpha, beta in ((1, 1), (2, 0.5)):
        h, got_dl, got_ds = M.hqnr(ps, ms, pan, "QB", alpha=alpha, beta=beta)
        assert got_dl == dl and got_ds == ds
        assert abs(h - (1.0 - dl) ** alpha * (1.0 - ds) ** beta) <= TOL
    assert M.hqnr(ps, ms, pan, M.MTF_GAINS["QB"]) == M.hqnr(ps, ms, pan, "QB")          # explicit gains
    _, dl0, ds0 = M.hqnr(ms, ms, pan, "QB", pan_lp=pan)
    assert ds0 == 0.0 and dl0 > 0.0
    _, _, ds2 = M.hqnr(ps, ms, pan, "QB", ratio=2)
    assert abs(ds2 - M.d_s_block(ps, ms, pan, M.pan_lowpass(pan, "QB", 2))) <= TOL
    assert M.HQNR_FIELDS == ("d_lambda_k", "d_s", "hqnr")


def test_constant_window_is_nan():
    a, b = _rand(18, 2, 32, 64), _rand(19, 1, 32, 64)
    a, b = a.astype(np.float32), b.astype(np.float32)
    a[1, :, 32:] = 0.25
    b[0, :, 32:] = 0.5
    got = M.uqi_blocks(a, b)
    assert np.isnan(got[1, 0, 1]) and np.isfinite(np.delete(got.ravel(), 3)).all()
    assert np.isnan(M.d_s_block(a, a, b, b)) and np.isnan(M.d_s_block(a, _rand(20, 2, 32, 64), b, b))
    zero = np.zeros((1, 32, 32))
    assert np.isnan(M.uqi_blocks(zero, zero)[0, 0, 0])


def test_entry_points_are_declared_exported_and_bound():
    import ctypes
    import os
    import re
    from conftest import ROOT
    from tmdiff_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmdiff_hip.h")).read(), flags=re.S)
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("tmdiff_metrics_dsblock_supported", 5), ("tmdiff_metrics_dsblock_workspace_bytes", 5),
                        ("tmdiff_metrics_dsblock", 24)):
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in include/tmdiff_hip.h"
        assert hasattr(cdll, name) and len(_lib.SIGNATURES[name][1]) == nargs


def test_entry_point_refuses_what_it_does_not_take():
    """The extent checks come before any launch and before the null-pointer check, so they run without a GPU."""
    from tmdiff_amd import _lib
    lib = _lib.lib

    def run(b=1, c=4, h=64, w=64, block=32, q=1.0):
        return lib.tmdiff_metrics_dsblock(None, 0, 0, None, 0, 0, None, 0, None, 0, b, c, h, w, block, q, None, 1.0, 1.0, None, None,
                                          None, 0, None)

    assert lib.tmdiff_metrics_dsblock_supported(1, 4, 64, 64, 32) == 1
    assert lib.tmdiff_metrics_dsblock_workspace_bytes(2, 4, 40, 72, 32) == 2 * 4 * 2 * 2 * 3 * 8
    assert run(b=0) == 0                                                      # nothing to do
    for kw in (dict(c=17), dict(c=0), dict(block=12), dict(h=8, w=8), dict(h=15), dict(b=2, c=16, h=8192, w=8192)):
        args = {"b": 1, "c": 4, "h": 64, "w": 64, "block": 32, **kw}
        assert lib.tmdiff_metrics_dsblock_supported(*args.values()) == 0, kw
        assert lib.tmdiff_metrics_dsblock_workspace_bytes(*args.values()) == 0, kw
        assert run(**kw) == UNSUPPORTED and "metrics_dsblock" in lib.tmdiff_last_error_string().decode(), kw
    for q in (0.0, -1.0, float("nan")):
        assert run(q=q) == UNSUPPORTED
    assert run() not in (0, UNSUPPORTED)                                # supported extents, null tensors: refused later


def test_val_dataset_argument_errors(tmp_path):
    from tmdiff_amd import evaluate
    with pytest.raises(ValueError, match="full_resolution"):
        evaluate.val_dataset(None, "QB", [], str(tmp_path), protocol="hqnr", full_resolution=False)
    with pytest.raises(ValueError, match="protocol"):
        evaluate.val_dataset(None, "QB", [], str(tmp_path), protocol="khan", full_resolution=True)
    with pytest.raises(ValueError, match="sensor"):
        evaluate.val_dataset(None, "GF2", [], str(tmp_path), protocol="hqnr", full_resolution=True)    # no row of its own


def test_validation_options_select_the_protocol():
    from tmdiff_amd.train import validation_options
    assert validation_options({}) == {} and validation_options({"full_resolution": False}) == {}
    assert validation_options({"full_resolution": True}) == {"full_resolution": True}                  # QNR, as before
    assert validation_options({"full_resolution": "hqnr"}) == {"full_resolution": True, "protocol": "hqnr", "sensor": None}
    assert validation_options({"full_resolution": "HQNR", "sensor": "WV3"})["sensor"] == "WV3"
    with pytest.raises(ValueError, match="full_resolution"):
        validation_options({"full_resolution": "khan"})
