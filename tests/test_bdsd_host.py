"""CPU-only tests of BDSD: the float64 host definitions ``metrics.bdsd_moments``, ``bdsd_coeffs``, ``bdsd_inject`` and ``bdsd``,
``tiling.bdsd_fuse`` on host arrays and the ``bdsd`` names of ``evaluate.val_dataset(baselines=...)``.  Unpinned: the Pansharpening
Toolbox is not available, so the definition is held to its own algebra, to numpy's least squares and to a scene on which the method
must help.

The file also holds what the GPU test (tests/test_gpu_bdsd.py) needs: the shapes, the inputs and the reduced-scale triples.
Every input keeps cond(N) <= 1e6 in every block (``worst_cond``; each test prints its worst value): the bounds that carry a factor
cond(N) mean something only then."""
import numpy as np
import pytest
import torch

from test_glp_host import _scene, glp_inputs
from tmdiff_amd import metrics as M

COND_MAX = 1e6
# [B, C, H, W], ratio, sensor or gains, full-scale block side (None: the whole image)
BDSD_CASES = [
    ((1, 4, 64, 64), 4, "QB", None),
    ((1, 4, 64, 64), 4, "QB", 32),                                  # 2 x 2 blocks of 64 reduced pixels
    ((1, 8, 64, 64), 4, "WV3", 32),
    ((2, 3, 36, 72), 2, "none", 12),                                # 3 x 6 blocks of 36 reduced pixels, W % 4 == 0, block % 4 == 0
    ((1, 1, 8, 8), 4, ((0.29,), 0.15), None),                       # one band, four reduced pixels
]
BDSD_IDS = ["64x64x4", "64x64x4/32", "64x64x8/32", "36x72x3@x2/12", "8x8x1"]


def bdsd_inputs(seed, b, c, h, w):
    """(ms_exp, pan) float32 tensors as ``glp_inputs`` makes them: independent bands, the PAN a mix of them plus noise."""
    return glp_inputs(seed, b, c, h, w)


def reduced_inputs(seed, b, c, h, w):
    """A reduced-scale triple (low_lp, low_pan, low_ms) of float32 tensors for the moments alone: independent uniform planes."""
    g = torch.Generator().manual_seed(seed)
    return tuple(0.1 + 0.8 * torch.rand(b, k, h, w, generator=g) for k in (c, 1, c))


def worst_cond(moments):
    """The largest cond(N) over the blocks of a [..., C + 1, 2 C + 1] array of ``bdsd_moments``."""
    k = moments.shape[-2]
    return float(np.linalg.cond(moments[..., :k]).max())


def _blocks(x, bs):
    """x [K, h, w] -> a list over the blocks, row-major, of [K, bs * bs] arrays."""
    k, h, w = x.shape
    return [x[:, i:i + bs, j:j + bs].reshape(k, -1) for i in range(0, h, bs) for j in range(0, w, bs)]


def _triple(seed=0, b=2, c=4, h=16, w=24):
    rng = np.random.default_rng(seed)
    return 0.1 + 0.8 * rng.random((b, c, h, w)), 0.1 + 0.8 * rng.random((b, h, w)), 0.1 + 0.8 * rng.random((b, c, h, w))


def test_moments_against_numpy():
    assert M.BDSD_MAX_BANDS == 15
    lp, pan, ms = _triple()
    b, c = lp.shape[:2]
    for bs in (None, 8):
        mo = M.bdsd_moments(lp, pan, ms, bs)
        nby, nbx = (1, 1) if bs is None else (2, 3)
        assert mo.shape == (b, nby, nbx, c + 1, 2 * c + 1)
        print(f"moments bs={bs}: worst cond(N) {worst_cond(mo):.3e}")
        assert worst_cond(mo) <= COND_MAX
        for i in range(b):
            hm_all, d_all = np.concatenate([lp[i], pan[i][None]]), ms[i] - lp[i]
            tiles = [(hm_all.reshape(c + 1, -1), d_all.reshape(c, -1))] if bs is None else list(zip(_blocks(hm_all, bs), _blocks(d_all, bs)))
            for t, (hm, d) in enumerate(tiles):
                got = mo[i, t // nbx, t % nbx]
                assert np.abs(got[:, :c + 1] - hm @ hm.T).max() <= 1e-12 * np.abs(hm @ hm.T).max()
                assert np.abs(got[:, c + 1:] - hm @ d.T).max() <= 1e-12 * np.abs(hm @ hm.T).max()
                assert np.array_equal(got[:, :c + 1], got[:, :c + 1].T)               # exactly symmetric
    assert np.array_equal(M.bdsd_moments(lp, pan[:, None], ms), M.bdsd_moments(lp, pan, ms))   # pan as [..., 1, h, w]
    assert np.array_equal(M.bdsd_moments(lp[0], pan[0], ms[0], 8), M.bdsd_moments(lp, pan, ms, 8)[0])


def test_coeffs_are_the_least_squares_fit():
    lp, pan, ms = _triple(1)
    b, c = lp.shape[:2]
    for bs in (None, 8):
        mo = M.bdsd_moments(lp, pan, ms, bs)
        gamma = M.bdsd_coeffs(mo)
        nbx = mo.shape[2]
        assert gamma.shape == mo.shape[:3] + (c + 1, c)
        for i in range(b):
            hm_all, d_all = np.concatenate([lp[i], pan[i][None]]), ms[i] - lp[i]
            tiles = [(hm_all.reshape(c + 1, -1), d_all.reshape(c, -1))] if bs is None else list(zip(_blocks(hm_all, bs), _blocks(d_all, bs)))
            for t, (hm, d) in enumerate(tiles):
                got = gamma[i, t // nbx, t % nbx]
                want = np.linalg.lstsq(hm.T, d.T, rcond=None)[0]
                cond = np.linalg.cond(hm @ hm.T)
                err, bound = np.abs(got - want).max(), 1e-9 * cond * np.abs(want).max()
                assert cond <= COND_MAX and err <= bound, (cond, err, bound)
                # the residual is orthogonal to every regressor, at the rounding level of the sums
                res = hm @ (d.T - hm.T @ got)
                assert np.abs(res).max() <= 64 * (c + 1) * hm.shape[1] * 2.0 ** -53 * np.abs(hm @ hm.T).max() * max(1.0, np.abs(got).max())
        print(f"coeffs bs={bs}: worst cond(N) {worst_cond(mo):.3e}, max |gamma| {np.abs(gamma).max():.3f}")


def test_coeffs_recover_planted_weights():
    rng = np.random.default_rng(2)
    c, n = 5, 200
    hm = 0.1 + 0.8 * rng.random((3, 2, c + 1, n))                                    # 3 x 2 blocks
    gamma0 = rng.standard_normal((3, 2, c + 1, c))
    big_n = hm @ np.swapaxes(hm, -1, -2)
    mo = np.concatenate([big_n, big_n @ gamma0], -1)                                  # R = Hm' (Hm gamma0)
    cond = worst_cond(mo)
    got = M.bdsd_coeffs(mo)
    err = np.abs(got - gamma0).max()
    print(f"planted weights: cond(N) {cond:.3e}, worst error {err:.3e}")
    assert cond <= COND_MAX and err <= 64 * (c + 1) ** 2 * cond * 2.0 ** -53 * np.abs(gamma0).max()


def test_block_equal_to_the_image_is_the_global_fit():
    ms, pan = (t.numpy().astype(np.float64) for t in bdsd_inputs(3, 2, 4, 32, 32))
    want = M.bdsd(ms, pan, "QB", 4)
    got = M.bdsd(ms, pan, "QB", 4, block=32)
    assert np.isfinite(want).all() and np.array_equal(got, want)
    lp, p, low = M.bdsd_reduced(ms, pan, "QB", 4)
    assert np.array_equal(M.bdsd_moments(lp, p, low, 8), M.bdsd_moments(lp, p, low))


def test_equal_weights_in_every_block_are_the_global_injection():
    rng = np.random.default_rng(4)
    ms, pan = rng.random((2, 3, 16, 24)), rng.random((2, 16, 24))
    gamma = rng.standard_normal((2, 1, 1, 4, 3))
    want = M.bdsd_inject(ms, pan, gamma)
    assert np.array_equal(M.bdsd_inject(ms, pan, np.broadcast_to(gamma, (2, 2, 3, 4, 3)), 8), want)
    direct = ms + np.einsum("bkc,bkhw->bchw", gamma[:, 0, 0], np.concatenate([ms, pan[:, None]], 1))
    assert np.abs(want - direct).max() <= 1e-14 * np.abs(direct).max() * 4
    local = rng.standard_normal((2, 2, 3, 4, 3))                                      # ... and each pixel takes its own block's
    got = M.bdsd_inject(ms, pan, local, 8)
    for iy in range(2):
        for ix in range(3):
            sl = (slice(None), slice(None), slice(8 * iy, 8 * iy + 8), slice(8 * ix, 8 * ix + 8))
            one = M.bdsd_inject(ms[sl], pan[sl[0], sl[2], sl[3]], local[:, iy:iy + 1, ix:ix + 1])
            assert np.array_equal(got[sl], one)


def singular_moments():
    """(ms_exp, pan, moments) of a [2, 3, 48, 48] x2 "none" scene in 2 x 2 blocks of 12 x 12 reduced pixels whose reduced block
    (1, 0) of image 0 holds band 0 once more as band 2, in the low-pass and in the raw MS."""
    ms, pan = (t.numpy().astype(np.float64) for t in bdsd_inputs(5, 2, 3, 48, 48))
    lp, p, low = (x.copy() for x in M.bdsd_reduced(ms, pan, "none", 2))
    lp[0, 2, 12:, :12], low[0, 2, 12:, :12] = lp[0, 0, 12:, :12], low[0, 0, 12:, :12]
    return ms, pan, M.bdsd_moments(lp, p, low, 12)


def singular_case():
    ms, pan, mo = singular_moments()
    return ms, pan, M.bdsd_coeffs(mo)


def test_singular_block_is_nan_and_alone():
    """A duplicated band under equal gains ("none") repeats its low-pass bit for bit: the pivot of the copy is exactly 0 minus
    squares.  That block's weights and pixels are NaN; the other blocks and the other image stay finite."""
    ms, pan = (t.numpy().astype(np.float64) for t in bdsd_inputs(5, 2, 3, 48, 48))
    ms, pan, gamma = singular_case()
    bad = np.isnan(gamma).all((-2, -1))
    assert bad[0, 1, 0] and bad.sum() == 1 and np.isfinite(gamma[~bad]).all()
    f = M.bdsd_inject(ms, pan, gamma, 24)
    assert np.isnan(f[0, :, 24:, :24]).all()
    f[0, :, 24:, :24] = 0.0
    assert np.isfinite(f).all()
    # through the whole chain the low-pass reaches across block borders, so the copy must hold on the filter's whole support: a
    # band duplicated throughout image 0 makes every block of that image NaN and leaves image 1 alone
    lr = ms[..., 1::2, 1::2].copy()
    lr[0, 2] = lr[0, 0]
    f = M.bdsd(ms, pan, "none", 2, 24, lr_ms=lr)
    assert np.isnan(f[0]).all() and np.isfinite(f[1]).all()


def test_bdsd_beats_the_interpolated_ms():
    """Sanity of the method on the scene of test_glp_host: against the scene, BDSD has a strictly lower ERGAS than ms_exp has, with
    one set of weights and with one per 32 x 32 block.  Measured on this scene: ms_exp 3.4862, bdsd 0.9784, bdsd block 32 1.1383."""
    scene, pan = _scene()
    ms = M.upsample_poly23(M.mtf_degrade(scene, "QB"))
    base = M.ergas(scene, ms, hwc=False)
    got = {b: M.ergas(scene, M.bdsd(ms, pan, "QB", 4, b), hwc=False) for b in (None, 32)}
    print(f"ERGAS: ms_exp {base:.4f}  bdsd {got[None]:.4f}  bdsd block 32 {got[32]:.4f}")
    assert all(v < base for v in got.values()), (base, got)


def test_hwc_layout_and_lent_lr_ms():
    ms, pan = (t.numpy().astype(np.float64)[0] for t in bdsd_inputs(6, 1, 4, 32, 48))
    want = M.bdsd(ms, pan, "QB", 4, 16)
    got = M.bdsd(np.moveaxis(ms, 0, -1), pan[0][..., None], "QB", 4, 16, hwc=True)
    assert got.shape == (32, 48, 4) and np.array_equal(np.moveaxis(got, -1, 0), want)
    lr = ms[..., 2::4, 2::4].copy()
    assert np.array_equal(M.bdsd(ms, pan, "QB", 4, 16, lr_ms=lr), want)               # the default reduced MS, lent
    other = M.bdsd(ms, pan, "QB", 4, 16, lr_ms=lr[::-1].copy())
    assert np.isfinite(other).all() and not np.array_equal(other, want)               # ... and lr_ms is what is used
    assert np.array_equal(M.bdsd(np.moveaxis(ms, 0, -1), pan[0], "QB", 4, 16, lr_ms=np.moveaxis(lr, 0, -1), hwc=True), got)


def test_reduced_images_are_the_stated_filters():
    rng = np.random.default_rng(7)
    lr = rng.random((2, 4, 8, 12))
    ms_exp, pan = M.upsample_poly23(lr, 4), rng.random((2, 32, 48))
    lp, p, low = M.bdsd_reduced(ms_exp, pan, "QB", 4)
    assert np.array_equal(low, lr)                                                    # the raw MS bit for bit
    assert np.array_equal(p, M.mtf_degrade(pan[:, None], 0.15, 4)[:, 0])
    for c, g in enumerate(M.MTF_GAINS["QB"][0]):
        assert np.array_equal(lp[:, c], M.fir_decimate(lr[:, c], M.mtf_kernel(g, 4), 1))


def test_bad_arguments():
    ms, pan = (t.numpy().astype(np.float64) for t in bdsd_inputs(8, 1, 4, 32, 32))
    with pytest.raises(ValueError, match="C <= 15"):
        M.bdsd(np.zeros((16, 8, 8)), np.zeros((8, 8)), "none")
    with pytest.raises(ValueError, match="ratio 2 or 4"):
        M.bdsd(ms, pan, "QB", ratio=3)
    with pytest.raises(ValueError, match="multiples"):
        M.bdsd(ms[..., :30], pan[..., :30], "QB")
    with pytest.raises(ValueError, match="divides H and W"):
        M.bdsd(ms, pan, "QB", 4, block=12)                                            # 32 % 12 != 0
    with pytest.raises(ValueError, match="multiple of the ratio"):
        M.bdsd(ms, pan, "QB", 4, block=2)                                             # 2 % 4 != 0
    with pytest.raises(ValueError, match="belong"):
        M.bdsd(ms, pan[..., :28], "QB")
    with pytest.raises(ValueError, match="lr_ms"):
        M.bdsd(ms, pan, "QB", lr_ms=np.zeros((1, 4, 5, 4)))
    with pytest.raises(ValueError, match="MS bands"):
        M.bdsd(ms, pan, "WV3")
    with pytest.raises(ValueError, match="moments"):
        M.bdsd_coeffs(np.zeros((5, 8)))
    with pytest.raises(ValueError, match="gamma"):
        M.bdsd_inject(ms, pan, np.zeros((1, 1, 1, 5, 3)))
    with pytest.raises(ValueError, match="differ"):
        M.bdsd_moments(ms, pan, ms[:, :3])


def test_tiling_bdsd_fuse_on_host_arrays():
    from tmdiff_amd.tiling import bdsd_fuse, consistency_refine
    rng = np.random.default_rng(9)
    lr, pan = 0.1 + 0.8 * rng.random((2, 4, 8, 16)), 0.1 + 0.8 * rng.random((2, 1, 32, 64))
    for block in (None, 32):
        want = M.bdsd(M.upsample_poly23(lr), pan, "QB", 4, block, lr_ms=lr)
        got = bdsd_fuse(lr, pan, "QB", block=block)
        assert isinstance(got, np.ndarray) and np.array_equal(got, want)
        assert np.array_equal(want, M.bdsd(M.upsample_poly23(lr), pan, "QB", 4, block))   # lr_ms itself is the reduced MS
    got = bdsd_fuse(torch.from_numpy(lr), torch.from_numpy(pan), "QB")
    assert torch.is_tensor(got) and np.array_equal(got.numpy(), M.bdsd(M.upsample_poly23(lr), pan, "QB"))
    refined = bdsd_fuse(lr, pan, "QB", consistency={"iters": 2})
    assert np.array_equal(refined, consistency_refine(M.bdsd(M.upsample_poly23(lr), pan, "QB"), lr, "QB", 4, iters=2))
    with pytest.raises(ValueError, match="score"):
        bdsd_fuse(lr, pan, "QB", score=True)
    with pytest.raises(ValueError, match="sensor"):
        bdsd_fuse(lr, pan, None)
    with pytest.raises(ValueError, match="pan"):
        bdsd_fuse(lr, pan[..., :40], "QB")
    with pytest.raises(ValueError, match="block"):
        bdsd_fuse(lr, pan, "QB", block=24)


def test_baseline_names():
    from tmdiff_amd import evaluate
    from tmdiff_amd.train import validation_options
    assert evaluate.BDSD_BASELINES == ("bdsd", "bdsd-local")
    assert evaluate.BASELINES == ("exp", "glp", "cbd", "hpm")
    assert evaluate.CS_BASELINES == ("cs-gs", "cs-gsa", "cs-brovey")
    assert M.CS_METHODS == ("gs", "gsa", "brovey") and M.CS_MAX_BANDS == 14 and M.GLP_MODES == ("glp", "cbd", "hpm")
    assert validation_options({"full_resolution": "hqnr", "sensor": "QB", "baselines": ["exp", "bdsd"]}) == \
        {"full_resolution": True, "protocol": "hqnr", "sensor": "QB", "baselines": ("exp", "bdsd")}
    with pytest.raises(ValueError, match="baselines"):
        evaluate.val_dataset(None, "QB", [], "unused", full_resolution=True, baselines=("bdsd-nope",))
    with pytest.raises(ValueError, match="baselines"):
        evaluate.val_dataset(None, "QB", [], "unused", full_resolution=True, baselines=("bdsd", "bdsd"))
    with pytest.raises(ValueError, match="baselines"):
        evaluate.val_dataset(None, "QB", [], "unused", baselines=("bdsd",))            # the host-metric mode


def test_gpu_cases_are_well_conditioned():
    """Every scene the GPU test fuses keeps cond(N) <= 1e6 in every block (float64 definitions)."""
    for i, ((b, c, h, w), ratio, sensor, block) in enumerate(BDSD_CASES):
        ms, pan = (t.numpy().astype(np.float64) for t in bdsd_inputs(400 + i, b, c, h, w))
        mo = M.bdsd_moments(*M.bdsd_reduced(ms, pan, sensor, ratio), None if block is None else block // ratio)
        cond = worst_cond(mo)
        print(f"case {BDSD_IDS[i]}: worst cond(N) {cond:.3e}")
        assert cond <= COND_MAX
