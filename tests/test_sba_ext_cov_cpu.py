"""CPU: the definition of the extrinsics SBA's covariances (tests/sba_ext_cov_ref.py, restating
DESIGN §3 / include/acinoset_hip.h) checked against independent formulations and against the
oracle solver's real scatter, and the Python entry points' new arguments.

Bounds. Identities between two formulations of one inverse are bounded by 10 cond2 2.2e-16 in the
measure max |A - B| / sqrt(diag B (x) diag B), cond2 of the Jacobi-scaled matrix that is inverted
(the constant of the GPU covariance tests). The Monte-Carlo bounds are the issue's: variance
ratios in [0.80, 1.20] (+- 4.4 statistical sd at 1000 draws) and bias <= 0.15 sd.
"""
import inspect

import numpy as np
import pytest

import sba_ext_cov_ref as xref
from oracle import sba_ext as oext

EPS = 2.2e-16
F_SCALE = 50.0


def _scene(n, C, seed=7, noise=0.5):
    K, D, R, t, X, uv, pi, ci = xref.synthetic(n, C, seed)
    if noise:
        uv = uv + np.random.default_rng(seed + 100).normal(0, noise, uv.shape)
    return K, D, R, t, X, uv, pi, ci


def _cond_scaled(A):
    d = 1.0 / np.sqrt(A.diagonal())
    return np.linalg.cond(A * np.outer(d, d))


@pytest.mark.parametrize('C,n', [(2, 12), (3, 40), (4, 40), (6, 80), (16, 400)])
def test_generators_annihilate_s_and_seven_zero_eigenvalues(C, n):
    K, D, R, t, X, uv, pi, ci = _scene(n, C)
    sys_ = xref.reduced_system(X, R, t, K, D, uv, pi, ci, F_SCALE)
    S, G = sys_['S'], xref.gauge_generators(R, t)
    assert np.linalg.norm(S @ G) <= 1e-14 * np.linalg.norm(S) * np.linalg.norm(G)
    w = np.sort(np.abs(np.linalg.eigvalsh(S)))
    assert w[6] <= 1e-12 * w[-1] < w[7]
    assert np.linalg.matrix_rank(G) == 7


@pytest.mark.parametrize('C,n', [(2, 12), (3, 40), (6, 80), (16, 400)])
def test_free_gauge_is_the_pseudo_inverse(C, n):
    K, D, R, t, X, uv, pi, ci = _scene(n, C)
    r = xref.covariance(X, R, t, K, D, uv, pi, ci, F_SCALE, 1.0, 'free')
    assert r['report']['status'] == 0
    err = xref.rel_error(r['cov_cams'], np.linalg.pinv(r['S']))
    bound = 10 * np.linalg.cond(r['Ah']) * EPS
    print('C = %d: |free - pinv| %.3g, bound %.3g' % (C, err, bound))
    assert err <= bound
    # sigma_px scales it
    r2 = xref.covariance(X, R, t, K, D, uv, pi, ci, F_SCALE, 2.0, 'free')
    np.testing.assert_allclose(r2['cov_cams'], 4.0 * r['cov_cams'], rtol=1e-14)


@pytest.mark.parametrize('C,n,anchor', [(2, 12, (0, 1)), (3, 40, (0, 1)), (3, 40, (2, 0)), (6, 80, (1, 4)),
                                        (16, 400, (5, 13))])
def test_s_transform_matches_null_basis_form(C, n, anchor):
    K, D, R, t, X, uv, pi, ci = _scene(n, C)
    r = xref.covariance(X, R, t, K, D, uv, pi, ci, F_SCALE, 1.0, 'anchor', anchor)
    a = anchor[0]
    Cm = xref.constraint_matrix(R, t, *anchor)
    alt = xref.anchor_nullspace(r['S'], Cm)
    _, _, Vt = np.linalg.svd(Cm)
    N = Vt[7:].T
    bound = 10 * max(np.linalg.cond(r['Ah']), _cond_scaled(N.T @ r['S'] @ N)) * EPS
    err = xref.rel_error(r['cov_cams'], alt)
    print('C = %d anchor %s: |S-transform - null basis| %.3g, bound %.3g' % (C, anchor, err, bound))
    assert err <= bound
    blk = r['cov_cams'][6 * a:6 * a + 6]
    assert not blk.any() and not r['cov_cams'][:, 6 * a:6 * a + 6].any()
    assert abs(alt[6 * a:6 * a + 6]).max() <= 1e-12 * abs(alt).max()
    # the constrained directions carry no variance
    assert abs(Cm @ r['cov_cams'] @ Cm.T).max() <= 1e-9 * abs(r['cov_cams']).max()


def test_point_formula_matches_full_system_inverse():
    """12 points x 3 cameras: cov_cams and every joint point covariance against the inverse of the
    full (cameras + points) Gauss-Newton matrix on the subspace the anchor constraints leave."""
    K, D, R, t, X, uv, pi, ci = _scene(12, 3)
    r = xref.covariance(X, R, t, K, D, uv, pi, ci, F_SCALE, 1.0, 'anchor', (0, 1))
    assert (r['status'] == xref.OK).all()
    n, C = 12, 3
    _, U, _, V, _, Wm, _, _ = oext.linearize(X, R, t, K, D.reshape(-1, 4), uv, pi.astype(np.int64), ci.astype(np.int64),
                                            F_SCALE)
    H = np.zeros((6 * C + 3 * n, 6 * C + 3 * n))
    for c in range(C):
        H[6 * c:6 * c + 6, 6 * c:6 * c + 6] = U[c]
    for i in range(n):
        H[18 + 3 * i:21 + 3 * i, 18 + 3 * i:21 + 3 * i] = V[i]
    for o in range(len(pi)):
        H[6 * ci[o]:6 * ci[o] + 6, 18 + 3 * pi[o]:21 + 3 * pi[o]] += Wm[o]
        H[18 + 3 * pi[o]:21 + 3 * pi[o], 6 * ci[o]:6 * ci[o] + 6] += Wm[o].T
    Cm = xref.constraint_matrix(R, t, 0, 1)
    _, _, Vt = np.linalg.svd(Cm)
    Nf = np.zeros((len(H), len(H) - 7))
    Nf[:18, :11] = Vt[7:].T
    Nf[18:, 11:] = np.eye(3 * n)
    A = Nf.T @ H @ Nf
    full = Nf @ np.linalg.solve(A, Nf.T)
    bound = 10 * _cond_scaled(A) * EPS
    err_c = xref.rel_error(r['cov_cams'], full[:18, :18])
    err_p = max(xref.rel_error(r['cov_points'][i], full[18 + 3 * i:21 + 3 * i, 18 + 3 * i:21 + 3 * i]) for i in range(n))
    print('cameras %.3g, points %.3g, bound %.3g' % (err_c, err_p, bound))
    assert err_c <= bound and err_p <= bound
    # the joint covariance is never smaller than the fixed-camera one
    for i in range(n):
        fixed = np.linalg.inv(V[i])
        assert np.linalg.eigvalsh(r['cov_points'][i] - fixed).min() >= -1e-9 * np.trace(fixed)


def test_centre_jacobian_by_finite_differences():
    K, D, R, t, *_ = _scene(12, 3)
    h = 1e-6
    for c in range(3):
        J = xref.centre_jacobian(R[c], t[c])
        fd = np.zeros((3, 6))
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            cp = -(oext.rodrigues(d[:3]) @ R[c]).T @ (t[c] + d[3:])
            cm = -(oext.rodrigues(-d[:3]) @ R[c]).T @ (t[c] - d[3:])
            fd[:, k] = (cp - cm) / (2 * h)
        np.testing.assert_allclose(J, fd, atol=1e-8 * max(1.0, np.abs(J).max()))
    # and the library's helper for world-frame centres uses the same Jacobian
    from acinoset_amd.lib import sba as lsba
    cov = np.diag([1e-6, 2e-6, 3e-6, 1e-4, 2e-4, 3e-4])
    J = xref.centre_jacobian(R[1], t[1])
    np.testing.assert_allclose(lsba.camera_centre_covariance(cov, R[1], t[1].reshape(3, 1)), J @ cov @ J.T, rtol=1e-13)
    np.testing.assert_allclose(lsba.camera_centres(R, t.reshape(-1, 3, 1)), xref.centres(R, t), rtol=1e-14)
    assert lsba.default_anchor(R, t) == xref.default_anchor(R, t)


def _starved(k):
    """A ring of 4 cameras, 40 points; the last camera keeps only k observations, all of points
    that two other cameras see."""
    K, D, R, t, X, uv, pi, ci = _scene(40, 4)
    others = np.bincount(pi[ci != 3], minlength=40)
    last = np.flatnonzero((ci == 3) & (others[pi] >= 2))
    keep = np.ones(len(pi), bool)
    keep[ci == 3] = False
    keep[last[:k]] = True
    return K, D, R, t, X, uv[keep], pi[keep], ci[keep]


@pytest.mark.parametrize('k,degenerate', [(None, False), (4, False), (3, False), (2, True), (1, True), (0, True)])
def test_degeneracy_on_its_side_of_the_threshold(k, degenerate):
    prob = _scene(40, 4) if k is None else _starved(k)
    K, D, R, t, X, uv, pi, ci = prob
    r = xref.covariance(X, R, t, K, D, uv, pi, ci, F_SCALE, 1.0, 'anchor', (0, 1))
    rep = r['report']
    print('k = %s: min pivot %.3g, status %d' % (k, rep['min_pivot'], rep['status']))
    assert rep['status'] == int(degenerate)
    if degenerate:
        assert not rep['min_pivot'] > 1e-12
        assert np.isnan(r['cov_cams']).all() and np.isnan(r['cov_points']).all()
        assert np.isnan(rep['rot_sd_max']) and np.isnan(rep['trans_sd_max'])
    else:
        assert rep['min_pivot'] > 1e-6
        assert np.isfinite(r['cov_cams']).all()


def test_one_camera_is_degenerate():
    K, D, R, t, X, uv, pi, ci = _scene(12, 2)
    one = ci == 0
    r = xref.covariance(X, R[:1], t[:1], K[:1], D[:1], uv[one], pi[one], ci[one], F_SCALE, 1.0, 'free')
    assert r['report']['status'] == 1 and r['report']['n_degenerate'] == 12
    assert np.isnan(r['cov_cams']).all() and np.isnan(r['cov_points']).all()


def test_points_that_are_not_ok_leave_s_unchanged():
    K, D, R, t, X, uv, pi, ci = _scene(40, 3)
    base = xref.covariance(X, R, t, K, D, uv, pi, ci, F_SCALE, 1.0, 'anchor', (0, 1))
    # point 40 unobserved, points 41 and 42 seen by one camera each
    X2 = np.vstack([X, [[0.1, 0.2, 0.3]], X[:2] + 0.05])
    uv2 = np.vstack([uv, uv[pi == 0][:1], uv[pi == 1][:1]])
    pi2 = np.concatenate([pi, [41, 42]]).astype(np.int32)
    ci2 = np.concatenate([ci, ci[pi == 0][:1], ci[pi == 1][:1]]).astype(np.int32)
    r = xref.covariance(X2, R, t, K, D, uv2, pi2, ci2, F_SCALE, 1.0, 'anchor', (0, 1))
    np.testing.assert_array_equal(r['status'][40:], [xref.NOOBS, xref.DEGENERATE, xref.DEGENERATE])
    np.testing.assert_array_equal(r['S'], base['S'])
    np.testing.assert_array_equal(r['cov_cams'], base['cov_cams'])
    assert np.isnan(r['cov_points'][40:]).all() and np.isfinite(r['cov_points'][:40]).all()
    rep = r['report']
    assert (rep['n_ok'], rep['n_noobs'], rep['n_degenerate']) == (40, 1, 2)
    assert rep['sigma_hat_px'] == base['report']['sigma_hat_px'] and rep['dof'] == base['report']['dof']


def _log_so3(R):
    c = np.clip((np.trace(R) - 1) * 0.5, -1.0, 1.0)
    th = np.arccos(c)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * 0.5
    return v if th < 1e-12 else v * (th / np.sin(th))


def test_monte_carlo_scatter_of_the_oracle_solver():
    """1000 noise draws (sigma = 1 px, f_scale = 50, seeds 1000 + k, started at the truth) of the
    oracle solver on the 40 points x 3 cameras scene, each solution mapped to the anchor gauge by
    the similarity that puts camera 0 on its true pose and the 0-1 baseline at its true length.
    Along every eigenvector of the predicted covariance (11 camera axes, 120 point axes) the
    sample variance over the prediction lies in [0.80, 1.20] and the bias within 0.15 sd."""
    K, D, R, t, X, uv0, pi, ci = xref.synthetic(40, 3, 7)
    pi64, ci64 = pi.astype(np.int64), ci.astype(np.int64)
    pred = xref.covariance(X, R, t, K, D, uv0, pi, ci, F_SCALE, 1.0, 'anchor', (0, 1))
    assert pred['report']['status'] == 0
    c_true = xref.centres(R, t)
    L = np.linalg.norm(c_true[1] - c_true[0])
    n_draws = 1000
    dc = np.empty((n_draws, 18))
    dx = np.empty((n_draws, 40, 3))
    for k in range(n_draws):
        uv = uv0 + np.random.default_rng(1000 + k).normal(0, 1.0, uv0.shape)
        Xs, Rs, ts, info = oext.sba_extrinsics(uv, X, pi64, ci64, K, D.reshape(-1, 4), R, t, f_scale=F_SCALE)
        ts = ts.reshape(-1, 3)
        # X' = s Q X + tau; R' = R Q^T, t' = s t - R' tau
        Q = R[0].T @ Rs[0]
        c = xref.centres(Rs, ts)
        s = L / np.linalg.norm(c[1] - c[0])
        tau = c_true[0] - s * Q @ c[0]
        Ra = Rs @ Q.T
        ta = s * ts - np.einsum('cij,j->ci', Ra, tau)
        dx[k] = (s * Xs @ Q.T + tau) - X
        for cam in range(3):
            dc[k, 6 * cam:6 * cam + 3] = _log_so3(Ra[cam] @ R[cam].T)
            dc[k, 6 * cam + 3:6 * cam + 6] = ta[cam] - t[cam]
    w, V = np.linalg.eigh(pred['cov_cams'])
    axes = w > 1e-9 * w.max()
    assert axes.sum() == 11
    proj = dc @ V[:, axes]
    ratio = proj.var(0) / w[axes]
    bias = np.abs(proj.mean(0)) / np.sqrt(w[axes])
    print('cameras: variance ratios %.3f..%.3f, bias <= %.3f sd' % (ratio.min(), ratio.max(), bias.max()))
    rp, bp = [], []
    for i in range(40):
        wi, Vi = np.linalg.eigh(pred['cov_points'][i])
        pr = dx[:, i] @ Vi
        rp.append(pr.var(0) / wi)
        bp.append(np.abs(pr.mean(0)) / np.sqrt(wi))
    rp, bp = np.array(rp), np.array(bp)
    print('points: variance ratios %.3f..%.3f, bias <= %.3f sd' % (rp.min(), rp.max(), bp.max()))
    # the gauge directions did not move
    assert np.abs(dc[:, :6]).max() <= 1e-9
    assert ratio.min() >= 0.80 and ratio.max() <= 1.20 and bias.max() <= 0.15
    assert rp.min() >= 0.80 and rp.max() <= 1.20 and bp.max() <= 0.15
    # what the joint covariance adds over the fixed-camera one, by trace
    fixed = np.array([np.trace(np.linalg.inv(v)) for v in pred['V']])
    joint = np.array([np.trace(c) for c in pred['cov_points']])
    print('joint / fixed-camera point covariance by trace: %.2f..%.2f' % ((joint / fixed).min(), (joint / fixed).max()))
    assert (joint >= fixed).all()


def test_python_entry_points_carry_the_new_arguments():
    from acinoset_amd import _native
    from acinoset_amd.lib import app, sba as lsba
    p = inspect.signature(lsba.bundle_adjust_points_and_extrinsics).parameters
    assert p['covariance'].default is False and p['sigma_px'].default == 1.0
    assert p['gauge'].default == 'anchor' and p['anchor'].default is None
    for fn in (lsba._sba_board_points, app.sba_board_points_fisheye):
        p = inspect.signature(fn).parameters
        assert p['covariance'].default is False and p['sigma_px'].default == 1.0
    p = inspect.signature(_native.Context.sba_extrinsics_covariance).parameters
    assert p['gauge'].default == 'anchor' and p['sigma_px'].default == 1.0
    assert 'acs_sba_extrinsics_covariance' in _native.SYMBOLS and 'acs_sba_ext_cov_default_opts' in _native.SYMBOLS
    o = _native.SbaExtCovOpts()
    _native.load_library().acs_sba_ext_cov_default_opts(_native.C.byref(o))
    assert (o.gauge, o.anchor_cam, o.scale_cam, o.f_scale, o.sigma_px) == (1, 0, 1, 1.0, 1.0)
