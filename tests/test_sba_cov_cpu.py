"""CPU: the numpy restatement of the SBA covariance (tests/sba_cov_ref.py) that the GPU tests
compare against, and the claim behind the feature: H^-1 predicts the solver's real scatter.

* The helper's LDL^T inverse against np.linalg.inv on `six` and `ring` (both models) in the
  measure max |S - R| / sqrt(diag R (x) diag R). Both are backward-stable 3x3 factorisations
  (LDL^T without pivoting of a positive definite matrix; LU with partial pivoting), each with a
  forward error of a few cond(H) eps, so the bound is the GPU tests' own: 10 cond(H) 2.2e-16.
  Measured: at most 0.56 cond eps (fisheye 0.48).
* Its status rule on `six`: exactly 1 NOOBS, 6 DEGENERATE (the single-camera points), 60 OK; the
  pivot ratio separates them by decades on either side of 1e-9.
* Monte-Carlo: 2,000 noise draws (1 px) per case, 3 points x the camera sets {all six, (0, 1),
  (2, 5)} of the dummy scene, solved by the oracle. Along every eigenvector of the predicted
  covariance the ratio sample variance / predicted variance must lie in [0.85, 1.15]: the
  statistical sd of a ratio is sqrt(2 / 1999) = 3.2 %, so the band is about 4.7 sigma.
"""
import numpy as np
import pytest

import sba_cov_problems as probs
import sba_cov_ref as cref

EPS = 2.2e-16
CASES = [(n, m) for n in ('six', 'ring') for m in ('fisheye', 'standard')]


def test_new_symbols_are_bound():
    from acinoset_amd import _native
    for s in ('acs_sba_points_covariance', 'acs_sba_points_dense_covariance'):
        assert s in _native.SYMBOLS and hasattr(_native.load_library(), s)
    for m in ('sba_points_covariance', 'sba_points_dense_covariance', 'sba_points_dense_covariance_dev'):
        assert hasattr(_native.Context, m)


@pytest.mark.parametrize('name,model', CASES)
def test_ldl_inverse_matches_numpy(name, model):
    prob = probs.get(name, model)
    ref = prob.reference()
    ok = ref['status'] == cref.OK
    H = ref['H'][ok]
    inv, d = cref.ldl_inverse(H)
    exact = np.linalg.inv(H)
    cond = np.linalg.cond(H)
    err = cref.rel_error(inv, exact)
    print('%s %s: %d OK points, cond max %.3g, max err / (cond eps) %.3f' % (name, model, ok.sum(), cond.max(),
                                                                            (err / (cond * EPS)).max()))
    assert (err <= 10 * cond * EPS).all()
    assert np.array_equal(inv, np.swapaxes(inv, 1, 2))
    assert cond.max() <= 2.1e3


def test_status_rule_on_six():
    prob = probs.six()
    ref = prob.reference()
    st = ref['status']
    assert (np.sum(st == cref.NOOBS), np.sum(st == cref.DEGENERATE), np.sum(st == cref.OK)) == (1, 6, 60)
    assert np.array_equal(st == cref.NOOBS, prob.nobs == 0)
    assert np.array_equal(st == cref.DEGENERATE, prob.nobs == 1)
    assert np.isnan(ref['cov'][st != cref.OK]).all() and np.isfinite(ref['cov'][st == cref.OK]).all()
    ratio = cref.pivot_ratio(ref['H'])
    print('pivot ratio: single view max %.3g, >= 2 views min %.3g' % (ratio[prob.nobs == 1].max(),
                                                                      ratio[prob.nobs >= 2].min()))
    assert ratio[prob.nobs == 1].max() <= 1e-11 and ratio[prob.nobs >= 2].min() >= 1e-3
    rep = ref['report']
    assert (rep['n_points'], rep['n_ok'], rep['n_noobs'], rep['n_degenerate']) == (67, 60, 1, 6)
    np.testing.assert_allclose(rep['sigma_hat_px'], 0.9629, atol=5e-5)
    np.testing.assert_allclose(probs.ring().reference()['report']['sigma_hat_px'], 1.0363, atol=5e-5)


def test_nan_point_is_degenerate():
    prob = probs.six()
    pts = prob.ref.copy()
    pts[66] = np.nan
    ref = prob.reference(pts=pts)
    assert ref['status'][66] == cref.DEGENERATE and np.isnan(ref['cov'][66]).all()
    assert np.array_equal(ref['status'][:66], prob.reference()['status'][:66])


@pytest.mark.parametrize('k', range(9))
def test_monte_carlo_scatter_matches_prediction(k):
    prob = probs.six()
    uv, mask, pts0 = probs.mc_case(k)
    sol = prob.solve(uv, mask, pts0)
    ref = prob.reference(pts=sol, uv=uv, mask=mask)
    assert (ref['status'] == cref.OK).all()
    ratio, sd = probs.variance_ratios(sol, ref['cov'])
    bias = np.abs(np.linalg.eigh(ref['cov'].mean(0))[1].T @ (sol.mean(0) - pts0[0])) / sd
    print('case %d cameras %s point %d: predicted sd %s mm, variance ratios %s, bias %s sd' % (
        k, probs.MC_CAMERA_SETS[k // 3], probs.MC_POINTS[k % 3], np.round(1e3 * sd, 2), np.round(ratio, 3),
        np.round(bias, 3)))
    assert (ratio >= 0.85).all() and (ratio <= 1.15).all()
