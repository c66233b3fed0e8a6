"""The root-free Cholesky pair of tmdiff_amd/metrics.py, ``_ldl_factor`` and ``_ldl_solve``, which ``cs_coeffs`` ("gsa") and
``bdsd_coeffs`` share and whose loops the device repeats (csrc/classical.h): the factor reconstructs its matrix, the solve agrees
with numpy's, and a duplicated row gives a pivot that is exactly not positive."""
import numpy as np

from tmdiff_amd import metrics as M

EPS = 2.0 ** -53


def _spd(n, seed, batch=()):
    g = np.random.default_rng(seed).standard_normal(batch + (n, 4 * n))
    return g @ np.swapaxes(g, -1, -2) / (4 * n) + np.eye(n)


def _check(a, n, rhs):
    """Factor the leading n x n part of ``a``, solve every column of ``rhs`` [..., n, R]; assert both bounds; return the factor."""
    with np.errstate(divide="ignore", invalid="ignore"):
        fac, piv, bad = M._ldl_factor(a, n)
        x = np.stack([M._ldl_solve(fac, piv, rhs[..., r]) for r in range(rhs.shape[-1])], -1)
    assert fac.shape == a.shape[:-2] + (n, n) and piv.shape == a.shape[:-2] + (n,) and bad.shape == a.shape[:-2]
    assert not bad.any() and (piv > 0).all() and not np.triu(fac).any()
    sq = a[..., :n, :n]
    low = np.tril(fac, -1) + np.eye(n)
    back = (low * piv[..., None, :]) @ np.swapaxes(low, -1, -2)
    err = np.abs(back - sq).max((-2, -1))
    bound = 64 * n ** 2 * EPS * np.abs(sq).max((-2, -1))
    print(f"n={n}: reconstruction error / bound {np.max(err / bound):.3e}")
    assert (err <= bound).all(), (err, bound)
    want = np.linalg.solve(sq, rhs)
    err = np.abs(x - want).max((-2, -1))
    bound = 64 * n ** 2 * np.linalg.cond(sq) * EPS * np.abs(want).max((-2, -1))
    print(f"n={n}: solve error / bound {np.max(err / bound):.3e}, worst cond {np.linalg.cond(sq).max():.3e}")
    assert (err <= bound).all(), (err, bound)
    return fac, piv


def test_one_band():
    a = np.array([[[2.5, 7.0]], [[0.125, -3.0]]])                     # two 1 x 1 systems with their right-hand side beside them
    fac, piv = _check(a, 1, a[..., :, 1:])
    assert np.array_equal(piv, a[..., 0, :1]) and not fac.any()
    assert np.array_equal(M._ldl_solve(fac, piv, a[..., :, 1]), a[..., :, 1] / a[..., :, 0])


def test_sixteen_by_sixteen_with_several_right_hand_sides():
    n, r = 16, 5
    a = _spd(n, 11, (3,))
    assert np.linalg.cond(a).max() < 50
    rhs = np.random.default_rng(12).standard_normal((3, n, r))
    # the right-hand sides stand beside the matrix, as the moments of cs_coeffs and bdsd_coeffs hold them: a is wider than n
    _check(np.concatenate([a, rhs], -1), n, rhs)


def test_duplicated_row_and_column():
    n, dup, orig = 6, 4, 1
    idx = np.arange(n)
    idx[dup] = orig
    good = _spd(n, 21, (3,))
    a = good.copy()
    a[1] = good[1][np.ix_(idx, idx)]                                  # system 1: row and column `dup` repeat `orig` exactly
    assert np.array_equal(a[1, dup], a[1, orig]) and np.array_equal(a[1, :, dup], a[1, :, orig])
    with np.errstate(divide="ignore", invalid="ignore"):
        fac, piv, bad = M._ldl_factor(a, n)
    print(f"duplicated row: pivots {piv[1]}")
    assert piv[1, dup] <= 0.0 and (piv[1, :dup] > 0).all()
    assert bad.tolist() == [False, True, False]
    rhs = np.random.default_rng(22).standard_normal((2, n, 2))
    _check(a[[0, 2]], n, rhs)                                         # the neighbours are factored and solved as if alone
    assert np.array_equal(fac[[0, 2]], M._ldl_factor(a[[0, 2]], n)[0])
