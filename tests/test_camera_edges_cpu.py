"""CPU: the float64 references of tests/test_gpu_camera_edges.py pinned at the camera models' edges
(tests/camera_edges.py: the optical axis and OpenCV's r > 1e-8 guard, atan_pos's range limits, the
image rim, points behind the camera and in its plane), so that "GPU equals oracle" there means
"GPU is right".

* oracle/fisheye.project (both forms), project_jac and tests/standard_model.project / project_jac
  against a 50-digit mpmath evaluation from the same float64 inputs: values within 1e-11 px
  (measured worst 7.6e-13: a factor of 13 for another libm), Jacobians within 1e-9 max(1, |J|inf)
  of a central difference taken in 50 digits (measured 1.3e-13). In the camera's plane (Y2 = 0)
  both references are non-finite.
* The undistortion class table of camera_edges.UNDISTORT_CLASSES: converged, sentinel (not
  converged), flipped, or both, unchanged when theta_d moves by 1e-9 either way.
* The triangulation error budget: the oracle's distance from the 50-digit null vector per class;
  the constants test_gpu_camera_edges.TRI_BUDGET carries must be within [1, 2] times it.
* The SBA edge problems are well posed: the oracle ends every point in gtol, ftol or xtol with
  finite results after at most 30 passes, and no point's status hangs on a rounding
  (camera_edges.undecided).
"""
import numpy as np
import pytest

import camera_edges as ce
import standard_model as sm
import test_gpu_camera_edges as gpu_file
from oracle import fisheye, sba as osba

CLASSES = ('axis', 'seam', 'rim', 'behind')


@pytest.fixture(scope='module')
def cams():
    return ce.cameras()


def _per_class(e, d):
    return {c: float(d[e.cls == c].max()) for c in CLASSES if (e.cls == c).any()}


@pytest.mark.parametrize('form', ['opencv', 'fte'])
def test_fisheye_projection_matches_50_digits(cams, form):
    e = ce.edge_points(cams)
    assert {c: int((e.cls == c).sum()) for c in CLASSES} == ce.class_counts(cams)
    K, D, R, t = cams.K[e.cam], cams.D[e.cam], cams.R[e.cam], cams.t[e.cam]
    ref = ce.project_mp(e.X, K, D, R, t, form)
    worst = _per_class(e, ce.mp_absdiff(ref, fisheye.project(e.X, K, D, R, t, fte_form=form == 'fte')).max(1))
    print(form, 'max |oracle - 50 digits| (px):', worst)
    assert max(worst.values()) <= 1e-11


def test_fisheye_jacobian_matches_50_digit_difference(cams):
    e = ce.edge_points(cams)
    K, D, R, t = cams.K[e.cam], cams.D[e.cam], cams.R[e.cam], cams.t[e.cam]
    uv, J = fisheye.project_jac(e.X, K, D, R, t)
    assert ce.mp_absdiff(ce.project_mp(e.X, K, D, R, t), uv).max() <= 1e-11
    err = ce.mp_absdiff(ce.project_jac_mp(e.X, K, D, R, t), J).reshape(len(J), -1).max(1)
    scale = np.maximum(1.0, np.abs(J).reshape(len(J), -1).max(1))
    worst = _per_class(e, err / scale)
    print('max |J - difference| / max(1, |J|inf):', worst)
    assert max(worst.values()) <= 1e-9


@pytest.mark.parametrize('name', ['five', 'eight', 'zero'])
def test_standard_model_matches_50_digits(cams, name):
    e = ce.edge_points(cams, 'standard')
    counts = ce.class_counts(cams, 'standard')
    assert counts['rim'] == 0 and e.r.max() == 1.0
    assert {c: int((e.cls == c).sum()) for c in CLASSES} == counts
    d = sm.pad8(ce.standard_coeffs(cams.n)[name], cams.n)[e.cam]
    K, R, t = cams.K[e.cam], cams.R[e.cam], cams.t[e.cam]
    ref = ce.project_mp(e.X, K, d, R, t, 'standard')
    uv, J = sm.project_jac(e.X, K, d, R, t)
    worst = _per_class(e, np.maximum(ce.mp_absdiff(ref, sm.project(e.X, K, d, R, t)), ce.mp_absdiff(ref, uv)).max(1))
    print(name, 'max |helper - 50 digits| (px):', worst)
    assert max(worst.values()) <= 1e-11
    err = ce.mp_absdiff(ce.project_jac_mp(e.X, K, d, R, t, 'standard'), J).reshape(len(J), -1).max(1)
    scale = np.maximum(1.0, np.abs(J).reshape(len(J), -1).max(1))
    print(name, 'max |J - difference| / max(1, |J|inf): %.3e' % (err / scale).max())
    assert (err / scale).max() <= 1e-9


def test_plane_is_non_finite(cams):
    X, c = ce.plane_points(cams)
    with np.errstate(all='ignore'):
        for fte in (False, True):
            assert not np.isfinite(fisheye.project(X, cams.K[c], cams.D[c], cams.R[c], cams.t[c], fte_form=fte)).any()
        assert not np.isfinite(fisheye.project_jac(X, cams.K[c], cams.D[c], cams.R[c], cams.t[c])[0]).any()
        for co in ce.standard_coeffs(cams.n).values():
            assert not np.isfinite(sm.project(X, cams.K[c], sm.pad8(co, cams.n)[c], cams.R[c], cams.t[c])).any()


def test_undistortion_class_table():
    tc = ce.tri_cameras()
    assert set(ce.UNDISTORT_CLASSES['scene']) == set(ce.RIM_THETA_D)
    assert set(ce.UNDISTORT_CLASSES['sentinel']) == set(ce.SENT_THETA_D)
    for name, table in ce.UNDISTORT_CLASSES.items():
        cams_of = range(6) if name == 'scene' else [{'sentinel': tc.sentinel, 'flip': tc.flip}[name]]
        for theta_d, want in table.items():
            for c in cams_of:
                for step in (-1e-9, 0.0, 1e-9):
                    assert ce.undistort_class(theta_d + step, tc.K[c], tc.D[c]) == want, (name, theta_d, c, step)
    got = set(v for table in ce.UNDISTORT_CLASSES.values() for v in table.values())
    assert got == {'converged', 'sentinel', 'flipped', 'flipped_unconverged'}


def _tri_distances(cams, cs, undistort, ref):
    out = np.empty(len(ref))
    for i, (a, b) in enumerate(zip(cs.ca, cs.cb)):
        xa = undistort(cs.uva[i:i + 1], cams.K[a], cams.D[a])[0]
        xb = undistort(cs.uvb[i:i + 1], cams.K[b], cams.D[b])[0]
        A = ce.dlt_matrix(xa, xb, cams.R[a], cams.t[a], cams.R[b], cams.t[b])
        out[i] = ce.mp_absdiff(np.array(ce.dlt_point_mp(A), dtype=object), ref[i]).max()
    return out


def test_triangulation_error_budget():
    """The oracle's own distance (LAPACK's SVD in float64) from the 50-digit null vector of the same
    4 x 4, after the division by h[3], per class."""
    cams, cs = ce.tri_pair_cases()
    dist = _tri_distances(cams, cs, fisheye.undistort, ce.tri_pair_reference(cams, cs))
    measured = {c: float(dist[cs.cls == c].max()) for c in gpu_file.TRI_COUNTS if c not in ('standard', 'dense')}
    scm, css = ce.tri_standard_cases()
    measured['standard'] = float(_tri_distances(scm, css, sm.undistort, ce.tri_standard_reference(scm, css)).max())
    # T5's pairs, noise and all, through the same measure
    scene, uv, mask, _ = ce.tri_dense_problem(6, 257)
    sel = np.flatnonzero(mask[:, 0] & mask[:, 1])
    dc = types_ns(K=scene.K, D=scene.D.reshape(-1, 4), R=scene.R, t=scene.t.reshape(-1, 3))
    dn = types_ns(ca=np.zeros(len(sel), np.int32), cb=np.ones(len(sel), np.int32), uva=uv[sel, 0], uvb=uv[sel, 1])
    measured['dense'] = float(_tri_distances(dc, dn, fisheye.undistort, ce.tri_pair_reference(dc, dn)).max())
    print('oracle - 50 digits (m):', {k: '%.3e' % v for k, v in measured.items()})
    assert set(measured) == set(gpu_file.TRI_BUDGET)
    for c, d in measured.items():
        assert d <= gpu_file.TRI_BUDGET[c] <= 2.0 * d, (c, d, gpu_file.TRI_BUDGET[c])
    # the classes held to DESIGN section 4's 1e-9 m are an order of magnitude inside it themselves
    for c in gpu_file.TRI_CONTRACT:
        assert measured[c] < 1e-10, (c, measured[c])
    assert {c: int((cs.cls == c).sum()) for c in set(cs.cls)} | {'standard': len(css.ca)} == \
        {c: n for c, n in gpu_file.TRI_COUNTS.items() if c != 'dense'}
    hit = ce.standard_put_back(scm, css)
    assert hit.any() and not hit.all()


def types_ns(**kw):
    import types
    return types.SimpleNamespace(**kw)


@pytest.mark.parametrize('name', list(ce.sba_cases()))
def test_sba_edge_problem_is_well_posed(name):
    prob, mask, pts0, repeat = ce.sba_cases()[name]
    Y2 = np.einsum('cj,nj->nc', prob.scene.R[:, 2], prob.truth) + prob.scene.t.reshape(-1, 3)[:, 2]
    assert Y2.min() > 0.5                                  # in front of every camera
    ref, info = ce.solve_oracle(prob, mask, pts0, repeat=repeat)
    seen = mask.sum(1) > 0
    assert np.isin(info['status'][seen], (osba.GTOL, osba.FTOL, osba.XTOL)).all(), info['status']
    assert (info['status'][~seen] == osba.NOOBS).all()
    assert np.isfinite(ref).all() and info['iters'].max() <= 30
    assert len(ce.undecided(info)) == 0, (ce.undecided(info), info['margins'][ce.undecided(info)])
    print('%s: %d points, status counts %s, iters_sum %d, nfev_sum %d' % (
        name, len(ref), np.bincount(info['status'], minlength=7).tolist(), info['iters'].sum(), info['nfev'].sum()))


@pytest.mark.parametrize('what', ['start', 'observation'])
def test_oracle_runs_a_nan_point(what):
    """A NaN start point (what the dense triangulation returns for a point without a pair) or a NaN
    observation: the point's matrix is never positive definite, so every pass is a rejection without
    a trial until lambda passes 1e16; no other point changes."""
    prob = ce.axis6()
    base, ibase = ce.solve_oracle(prob)
    pts0, uv = prob.pts0.copy(), prob.uv.copy()
    if what == 'start':
        pts0[ce.NAN_POINT] = np.nan
    else:
        uv[ce.NAN_POINT, 2, 0] = np.nan
    ref, info = ce.solve_oracle(prob, pts0=pts0, uv=uv)
    k = ce.NAN_POINT
    assert (info['status'][k], info['iters'][k], info['nfev'][k]) == (osba.STALLED, 20, 1)
    np.testing.assert_array_equal(ref[k], pts0[k])
    others = np.arange(len(ref)) != k
    np.testing.assert_array_equal(ref[others], base[others])
    for key in ('status', 'iters', 'nfev'):
        np.testing.assert_array_equal(info[key][others], ibase[key][others])
