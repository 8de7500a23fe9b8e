"""GPU: the camera models at the optical axis, the image rim and behind the camera.

Every solver goes through fisheye_project / fisheye_uvj / standard_project / standard_uvj,
fisheye_undistort / standard_undistort, dlt_null4 and the short-latency rcp_nr / rsq_nr / atan_pos
(csrc/common.hpp, tri.hip, fastmath.hpp). Their delicate parts are the edges of the input domain:
OpenCV's r > 1e-8 guard written as a select on r2 > 1e-16, atan_pos's three argument ranges,
rcp_nr(0) = NaN, the undistortion's clamp at pi/2 and its -1e6 sentinel, the Jacobi null vector's
skipped pairs. tests/camera_edges.py builds inputs that sit on them; tests/test_camera_edges_cpu.py
pins the float64 references used here against 50 digits.

Tolerances. Projection and residuals: 1e-9 px wherever |Y2| >= 0.5 m, which every
class but `plane` satisfies by construction; in the camera's plane both sides are non-finite.
SBA covariance: test_gpu_sba_cov.py's measure and bound, 10 cond(H) 2.2e-16. Points-only SBA: 1e-7 m
from the oracle with its status counts, iteration and evaluation sums. Triangulation: 1e-9 m for
the classes of TRI_CONTRACT (whose own float64 error is below 1e-10 m), else 10 x the oracle's own
distance from the 50-digit null vector (TRI_BUDGET, kept within [1, 2] x the recomputed distance by
the CPU test), floored at 1e-9 m: 10 is C_BOUND, the allowance for a different, equally stable
algorithm (Jacobi here, LAPACK there) on the same conditioning.
"""
import numpy as np
import pytest

import camera_edges as ce
import sba_cov_ref as cref
import standard_model as sm
import test_gpu_sba_cov as cov_file
import test_gpu_sba_pass as pass_file
from acinoset_amd import _native
from oracle import fisheye, sba as osba, sba_ext as oext

pytestmark = pytest.mark.gpu

PX_TOL = 1e-9
C_BOUND = 10.0
# the oracle's own distance (m) from the 50-digit null vector per triangulation class, recorded
# from tests/test_camera_edges_cpu.py::test_triangulation_error_budget (which holds each within
# [1, 2] x what it recomputes)
# (measured 8.34e-14, 1.11e-13, 1.61e-13, 2.62e-10, 4.15e-11, 3.52e-11, 6.48e-14; recorded 1.4 x that)
TRI_BUDGET = {'centre': 1.17e-13, 'rim': 1.55e-13, 'sentinel_conv': 2.25e-13, 'sentinel': 3.67e-10, 'far': 5.8e-11,
              'standard': 4.93e-11, 'dense': 9.07e-14}
TRI_CONTRACT = ('centre', 'sentinel_conv', 'standard', 'dense')      # held to 1e-9 m
TRI_COUNTS = {'centre': 36, 'rim': 48, 'sentinel_conv': 8, 'sentinel': 24, 'far': 12, 'standard': 72, 'dense': 257}
# measured on the MI355X: max |gpu - reference| (the tests print them)
MEASURED = {
    'projection, px (bound 1e-9)': {'fisheye axis': 4.55e-13, 'fisheye seam': 6.82e-13, 'fisheye rim': 9.09e-13,
                                    'fisheye behind': 1.36e-12, 'standard axis': 9.09e-13, 'standard seam': 5.12e-13,
                                    'standard behind': 9.09e-13, 'residuals': 1.36e-12},
    'covariance, error / (cond eps) (bound 10)': {'axis + seam fisheye': 4.196, 'axis + seam standard': 4.970,
                                                  'hub(6)': 1.824, 'hub(12)': 1.726},
    'points-only SBA, m (bound 1e-7)': 2.865e-09,
    'triangulation, m': {'centre': 8.34e-14, 'rim': 1.16e-13, 'sentinel_conv': 1.28e-13, 'sentinel': 9.12e-10,
                         'far': 6.37e-11, 'standard': 3.58e-11, 'dense': 7.34e-14},
}
CLASSES = ('axis', 'seam', 'rim', 'behind')
BLOCK_EDGE = (1, 255, 256, 257)


def _tri_bound(cls):
    return 1e-9 if cls in TRI_CONTRACT else max(C_BOUND * TRI_BUDGET[cls], 1e-9)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope='module')
def cams():
    return ce.cameras()


def _pack(c, model='fisheye', coeffs=None):
    if model == 'fisheye':
        return _native.pack_cameras(c.K, c.D, c.R, c.t)
    return _native.pack_cameras_standard(c.K, coeffs, c.R, c.t)


def _report(label, e, err):
    worst = {c: float(err[e.cls == c].max()) for c in CLASSES if (e.cls == c).any()}
    print(label, 'max |gpu - reference| (px):', {k: '%.2e' % v for k, v in worst.items()})
    return worst


# ---- 1. projection and residuals ---------------------------------------------------------------

@pytest.mark.parametrize('form', ['opencv', 'fte'])
def test_fisheye_projection_at_the_edges(ctx, cams, form):
    e = ce.edge_points(cams)
    assert {c: int((e.cls == c).sum()) for c in CLASSES} == ce.class_counts(cams)
    assert min(ce.class_counts(cams).values()) > 0
    fte = form == 'fte'
    uv = ctx.project(_pack(cams), e.X, e.cam, fte_form=fte)
    ref = fisheye.project(e.X, cams.K[e.cam], cams.D[e.cam], cams.R[e.cam], cams.t[e.cam], fte_form=fte)
    _report('fisheye ' + form, e, np.abs(uv - ref).max(1))
    np.testing.assert_allclose(uv, ref, rtol=0, atol=PX_TOL)
    # in the camera's plane: non-finite on both sides
    Xp, cp = ce.plane_points(cams)
    with np.errstate(all='ignore'):
        assert not np.isfinite(fisheye.project(Xp, cams.K[cp], cams.D[cp], cams.R[cp], cams.t[cp], fte_form=fte)).any()
    assert not np.isfinite(ctx.project(_pack(cams), Xp, cp, fte_form=fte)).any()
    # a camera index out of range gives NaN
    bad = e.cam[:4].copy()
    bad[1], bad[2] = cams.n, -1
    out = ctx.project(_pack(cams), e.X[:4], bad, fte_form=fte)
    assert np.isnan(out[1:3]).all()
    np.testing.assert_array_equal(_bits(out[[0, 3]]), _bits(uv[[0, 3]]))


@pytest.mark.parametrize('name', ['five', 'eight', 'zero'])
def test_standard_projection_at_the_edges(ctx, cams, name):
    e = ce.edge_points(cams, 'standard')
    counts = ce.class_counts(cams, 'standard')
    assert {c: int((e.cls == c).sum()) for c in CLASSES} == counts
    assert counts['rim'] == 0 and min(counts[c] for c in ('axis', 'seam', 'behind')) > 0
    co = ce.standard_coeffs(cams.n)[name]
    d = sm.pad8(co, cams.n)
    rec = _pack(cams, 'standard', co)
    uv = ctx.project(rec, e.X, e.cam)
    ref = sm.project(e.X, cams.K[e.cam], d[e.cam], cams.R[e.cam], cams.t[e.cam])
    _report('standard ' + name, e, np.abs(uv - ref).max(1))
    np.testing.assert_allclose(uv, ref, rtol=0, atol=PX_TOL)
    # on the axis exactly (the identity camera, r = 0): the principal point, no guard needed
    on = np.flatnonzero((e.cam == cams.identity) & (e.r == 0.0))
    assert len(on) == 3
    np.testing.assert_array_equal(uv[on], np.broadcast_to([cams.K[0, 0, 2], cams.K[0, 1, 2]], (3, 2)))
    Xp, cp = ce.plane_points(cams)
    with np.errstate(all='ignore'):
        assert not np.isfinite(sm.project(Xp, cams.K[cp], d[cp], cams.R[cp], cams.t[cp])).any()
    assert not np.isfinite(ctx.project(rec, Xp, cp)).any()
    bad = e.cam[:3].copy()
    bad[1] = cams.n
    assert np.isnan(ctx.project(rec, e.X[:3], bad)[1]).all()


@pytest.mark.parametrize('model', ['fisheye', 'eight'])
def test_residuals_at_the_edges(ctx, cams, model):
    std = model != 'fisheye'
    e = ce.edge_points(cams, 'standard' if std else 'fisheye')
    co = ce.standard_coeffs(cams.n)[model] if std else None
    rec = _pack(cams, 'standard' if std else 'fisheye', co)
    Xp, cp = ce.plane_points(cams)
    X = np.concatenate([e.X, Xp])
    cam = np.concatenate([e.cam, cp])
    n = len(e.X)
    if std:
        ref = sm.project(e.X, cams.K[e.cam], sm.pad8(co, cams.n)[e.cam], cams.R[e.cam], cams.t[e.cam])
    else:
        ref = fisheye.project(e.X, cams.K[e.cam], cams.D[e.cam], cams.R[e.cam], cams.t[e.cam])
    obs = np.concatenate([ref + np.random.default_rng(ce.SEED).normal(0, 2.0, ref.shape), np.zeros((2, 2))])
    # the observations in another order than the points, each with its own point's camera
    order = np.random.default_rng(ce.SEED + 1).permutation(len(X)).astype(np.int32)
    r = ctx.sba_residuals(rec, obs[order], order, cam[order], X).reshape(-1, 2)
    fin = order < n
    err = np.abs(r[fin] - (ref - obs[:n])[order[fin]]).max(1)
    print('residuals %s: max |gpu - reference| %.2e px over %d observations' % (model, err.max(), fin.sum()))
    assert err.max() <= PX_TOL
    assert fin.sum() == n and not np.isfinite(r[~fin]).any()           # the plane
    bad = cam[order].copy()
    bad[0] = cams.n
    assert np.isnan(ctx.sba_residuals(rec, obs[order], order, bad, X)[:2]).all()


@pytest.mark.parametrize('n', BLOCK_EDGE)
def test_projection_block_edge(ctx, cams, n):
    """n points around the 256-thread block, the last of them on the axis exactly (r = 0)."""
    e = ce.edge_points(cams)
    fill = np.flatnonzero(e.cls == 'seam')
    last = np.flatnonzero((e.cls == 'axis') & (e.r == 0.0))[0]
    idx = np.concatenate([np.resize(fill, n - 1), [last]]).astype(int)
    uv = ctx.project(_pack(cams), e.X[idx], e.cam[idx])
    ref = fisheye.project(e.X[idx], cams.K[e.cam[idx]], cams.D[e.cam[idx]], cams.R[e.cam[idx]], cams.t[e.cam[idx]])
    assert uv.shape == (n, 2)
    np.testing.assert_allclose(uv, ref, rtol=0, atol=PX_TOL)
    np.testing.assert_array_equal(uv[-1], [cams.K[0, 0, 2], cams.K[0, 1, 2]])


# ---- 2. SBA covariance: the Jacobian of model_project<., true>, directly ------------------------

def _in_front_seam(model):
    """The six scene cameras' seam points that every one of the six sees from the front."""
    c = ce.cameras()
    e = ce.edge_points(c, 'standard' if model != 'fisheye' else 'fisheye')
    sel = np.flatnonzero((e.cls == 'seam') & (e.cam < 6))
    Y2 = np.einsum('cj,nj->nc', c.R[:6, 2], e.X[sel]) + c.t[:6, 2]
    keep = sel[(Y2 > 0.5).all(1)]
    return e.X[keep], e.r[keep]


@pytest.mark.parametrize('layout', ['dense', 'list'])
@pytest.mark.parametrize('model', ['fisheye', 'eight'])
def test_covariance_on_the_axis_and_the_seams(ctx, model, layout):
    """The points themselves as the linearisation point: every `axis` point of axis6 and the seam
    points, seen by all six cameras."""
    prob = ce.axis6(model)
    Xs, rs = _in_front_seam(model)
    assert len(prob.truth) == 96 and len(Xs) >= 6 and (rs <= ce.T_PI8).any() and (rs > ce.T_PI8).any()
    pts = np.concatenate([prob.truth, Xs])
    sc = prob.scene
    std = model != 'fisheye'
    pj = sm.project_jac if std else fisheye.project_jac
    D = sm.pad8(prob.D, 6) if std else prob.D
    n = len(pts)
    pi, ci = np.repeat(np.arange(n), 6), np.tile(np.arange(6), n)
    t = sc.t.reshape(-1, 3)
    uv = pj(pts[pi], sc.K[ci], D[ci], sc.R[ci], t[ci])[0] + np.random.default_rng(ce.SEED + 4).normal(0, 1.0, (6 * n, 2))
    ref = cref.covariance(pj, uv, pi, ci, pts, sc.K, D, sc.R, t)
    rec = _native.pack_cameras_standard(sc.K, prob.D, sc.R, sc.t) if std else _native.pack_cameras(sc.K, prob.D, sc.R, sc.t)
    if layout == 'dense':
        got = ctx.sba_points_dense_covariance(rec, uv.reshape(n, 6, 2), np.ones((n, 6), np.uint8), pts)
    else:
        got = ctx.sba_points_covariance(rec, uv, pi.astype(np.int32), ci.astype(np.int32), pts)
    cov_file._check(got, ref, 'covariance axis + seam, %s %s (%d + %d points)' % (model, layout, 96, len(Xs)))
    assert got[2]['n_ok'] == n


@pytest.mark.parametrize('layout', ['dense', 'list'])
@pytest.mark.parametrize('C', [6, 12])
def test_covariance_at_the_hub(ctx, C, layout):
    prob = ce.hub(C)
    sc, pts = prob.scene, prob.truth
    n = len(pts)
    pi, ci = np.repeat(np.arange(n), C), np.tile(np.arange(C), n)
    t = sc.t.reshape(-1, 3)
    uv = prob.uv.reshape(-1, 2)
    ref = cref.covariance(fisheye.project_jac, uv, pi, ci, pts, sc.K, prob.D, sc.R, t)
    rec = _native.pack_cameras(sc.K, prob.D, sc.R, sc.t)
    if layout == 'dense':
        got = ctx.sba_points_dense_covariance(rec, prob.uv, prob.mask, pts)
    else:
        got = ctx.sba_points_covariance(rec, uv, pi.astype(np.int32), ci.astype(np.int32), pts)
    cov_file._check(got, ref, 'covariance hub(%d) %s' % (C, layout))
    assert got[2]['n_ok'] == n == 4 * C + 1


# ---- 3. points-only SBA: the guard inside k_sba_lm's own linearisation ---------------------------

_solved = {}


def _oracle(name):
    """The oracle's solution of a camera_edges.sba_cases() problem, computed once."""
    if name not in _solved:
        prob, mask, pts0, repeat = ce.sba_cases()[name]
        _solved[name] = (prob, mask, pts0, repeat) + ce.solve_oracle(prob, mask, pts0, repeat=repeat)
    return _solved[name]


def _records(prob):
    sc = prob.scene
    if prob.model == 'fisheye':
        return _native.pack_cameras(sc.K, prob.D, sc.R, sc.t), 'fisheye'
    return _native.pack_cameras_standard(sc.K, prob.D, sc.R, sc.t), 'standard'


def _against_oracle(label, pts, rep, ref, info):
    err = float(np.nanmax(np.abs(pts - ref)))
    print('%s: %d points, max |gpu - oracle| %.3e m, iters_sum %d (oracle %d), nfev_sum %d (oracle %d), %s' % (
        label, len(ref), err, rep['iters_sum'], info['iters'].sum(), rep['nfev_sum'], info['nfev'].sum(),
        {k: v for k, v in rep['status_counts'].items() if v}))
    assert err < 1e-7
    pass_file._check_counts(rep, info, len(ref))


ROW_OF = {'hub(3)': 2, 'hub(4)': 2, 'hub(5)': 3, 'axis6 fisheye': 3, 'axis6 fisheye from the truth': 3,
          'axis6 fisheye mask three': 3, 'axis6 fisheye mask lone': 3, 'hub(8)': 4}


@pytest.mark.parametrize('name', list(ROW_OF))
def test_row_and_butterfly_instances_on_the_axis(ctx, name):
    """Dense problems of 3 .. 8 cameras: the ROW instance the library picks, the register-resident
    butterfly it can be told to take instead, identical bits, and the oracle's decisions."""
    prob, mask, pts0, _, ref, info = _oracle(name)
    rec, _ = _records(prob)
    C, n = mask.shape[1], len(pts0)
    assert (C + 1) // 2 == ROW_OF[name]
    try:
        assert ctx.sba_lm_layout(C, n)[0] == 'row'
        row, rep_row = ctx.sba_points_dense(rec, prob.uv, mask, pts0)
        ctx.sba_set_lm_layout('butterfly')
        assert ctx.sba_lm_layout(C, n)[0] == 'butterfly'
        fly, rep_fly = ctx.sba_points_dense(rec, prob.uv, mask, pts0)
    finally:
        ctx.sba_set_lm_layout('auto')
    _against_oracle('ROW %d instance, %s' % (ROW_OF[name], name), row, rep_row, ref, info)
    _against_oracle('register-resident butterfly, %s' % name, fly, rep_fly, ref, info)
    np.testing.assert_array_equal(_bits(row), _bits(fly))
    assert rep_row == rep_fly
    if name.endswith('lone'):
        # point 0: one observation, inside the guard; point 1: none, untouched
        assert mask[0].sum() == 1 and mask[1].sum() == 0 and rep_row['status_counts']['noobs'] == 1
        np.testing.assert_array_equal(row[1], pts0[1])


@pytest.mark.parametrize('C,family', [(2, 'register-resident butterfly'), (12, 'register-resident butterfly'),
                                      (20, 'LDS-staged, one slot per lane')])
def test_butterfly_widths_at_the_hub(ctx, C, family):
    prob, mask, pts0, _, ref, info = _oracle('hub(%d)' % C)
    assert ctx.sba_lm_layout(C, len(pts0))[0] == 'butterfly'
    pts, rep = ctx.sba_points_dense(_records(prob)[0], prob.uv, mask, pts0)
    _against_oracle('%s, hub(%d)' % (family, C), pts, rep, ref, info)


@pytest.mark.parametrize('name', list(ce.sba_cases()))
def test_list_api_on_the_axis(ctx, name):
    """Every problem as an observation list: the camera-id instances (LDS-staged, one slot per lane;
    four slots per lane for the problem whose observations are repeated past 64 per point), both models."""
    prob, mask, pts0, repeat, ref, info = _oracle(name)
    rec, model = _records(prob)
    uv, pi, ci = ce.obs_list(prob, mask, repeat)
    K = int(np.bincount(pi, minlength=len(pts0)).max())
    assert (K > 64) == (repeat > 1)
    assert ctx.sba_lm_layout(K, len(pts0), cam_ids=True, camera_model=model)[0] == 'butterfly'
    pts, _, _, rep = ctx.sba_points(rec, uv, pi, ci, pts0, residuals=False)
    family = 'four slots per lane' if K > 64 else 'camera ids, one slot per lane'
    _against_oracle('%s (%s model, %d slots), %s' % (family, model, K, name), pts, rep, ref, info)


@pytest.mark.parametrize('name', ['axis6 five', 'axis6 eight', 'axis6 zero', 'axis6 five from the truth',
                                  'axis6 eight from the truth', 'axis6 zero from the truth'])
def test_standard_model_dense_on_the_axis(ctx, name):
    prob, mask, pts0, _, ref, info = _oracle(name)
    rec, model = _records(prob)
    assert model == 'standard' and ctx.sba_lm_layout(6, len(pts0), camera_model='standard')[0] == 'butterfly'
    pts, rep = ctx.sba_points_dense(rec, prob.uv, mask, pts0)
    _against_oracle('standard model (LDS-staged butterfly), %s' % name, pts, rep, ref, info)


def test_three_slots_per_lane_at_the_hub(ctx):
    """12 cameras at the smallest point count above the threshold (more than 4 waves per SIMD): 4 lanes
    x 3 slots. hub(12)'s 49 on-axis points tiled; every copy must have the first copy's bits."""
    prob, mask, pts0, _, ref, info = _oracle('hub(12)')
    n, m = pass_file.N_GRID, len(pts0)
    n_cu = ctx.sba_lm_layout(12, n)[1]
    assert ctx.sba_lm_layout(12, n)[0] == 'butterfly' and (n * 16 + 63) // 64 > 16 * n_cu
    idx = np.arange(n) % m
    pts, rep = ctx.sba_points_dense(_records(prob)[0], np.ascontiguousarray(prob.uv[idx]),
                                    np.ascontiguousarray(mask[idx]), np.ascontiguousarray(pts0[idx]))
    st = rep['status_counts']
    assert st['running'] == st['stalled'] == st['maxiter'] == st['noobs'] == 0, st
    sel = np.sort(np.random.default_rng(9).choice(n, 256, replace=False))
    err = float(np.abs(pts[sel] - ref[idx[sel]]).max())
    print('three slots per lane, hub(12) x %d points: max |gpu - oracle| over the sample %.3e m, iters_sum %d '
          '(oracle %d), nfev_sum %d (oracle %d)' % (n, err, rep['iters_sum'], info['iters'][idx].sum(),
                                                    rep['nfev_sum'], info['nfev'][idx].sum()))
    assert err < 1e-7
    np.testing.assert_array_equal(_bits(pts), _bits(pts[:m][idx]))
    assert rep['iters_sum'] == int(info['iters'][idx].sum()) and rep['nfev_sum'] == int(info['nfev'][idx].sum())
    assert rep['iters_max'] == int(info['iters'].max())
    for name, code in pass_file.STATUS.items():
        assert st[name] == int((info['status'][idx] == code).sum()), name


@pytest.mark.parametrize('api', ['dense row', 'dense butterfly', 'list'])
@pytest.mark.parametrize('what', ['start', 'observation'])
def test_non_finite_point_stays_alone(ctx, what, api):
    """A NaN start point (what acs_triangulate_dense returns for a point without a pair) or a NaN
    observation in a valid slot: the point's matrix is never positive definite, every pass is a
    rejection without a trial until lambda passes 1e16 (STALLED after 20 passes, one evaluation),
    as the oracle has it; every other point of its wave keeps the bits of the run without it."""
    prob, mask, _, _, _, ibase = _oracle('axis6 fisheye')
    k = ce.NAN_POINT
    pts0, uv = prob.pts0.copy(), prob.uv.copy()
    if what == 'start':
        pts0[k] = np.nan
    else:
        uv[k, 2, 0] = np.nan
    _, info = ce.solve_oracle(prob, pts0=pts0, uv=uv)
    assert (info['status'][k], info['iters'][k], info['nfev'][k]) == (osba.STALLED, 20, 1)
    rec, _ = _records(prob)

    def run(u, x):
        if api == 'list':
            pi, ci = np.nonzero(mask)
            out, _, _, rep = ctx.sba_points(rec, u[pi, ci], pi.astype(np.int32), ci.astype(np.int32), x, residuals=False)
            return out, rep
        return ctx.sba_points_dense(rec, u, mask, x)

    try:
        if api != 'list':
            ctx.sba_set_lm_layout(api.split()[1])
        clean, _ = run(prob.uv, prob.pts0)
        got, rep = run(uv, pts0)
    finally:
        ctx.sba_set_lm_layout('auto')
    pass_file._check_counts(rep, info, len(pts0))
    assert rep['status_counts']['stalled'] == 1
    others = np.arange(len(pts0)) != k
    np.testing.assert_array_equal(_bits(got[others]), _bits(clean[others]))
    np.testing.assert_array_equal(_bits(got[k]), _bits(pts0[k]))
    for key in ('status', 'iters', 'nfev'):
        np.testing.assert_array_equal(info[key][others], ibase[key][others])


# ---- 4. extrinsics SBA: fisheye_project<true>'s JY and Y -----------------------------------------

@pytest.mark.parametrize('max_iters', [1, 5])
def test_extrinsics_sba_at_the_hub(ctx, max_iters):
    """hub(6) started at the truth: every point on some camera's axis at the first linearisation."""
    prob = ce.hub(6)
    sc = prob.scene
    uv, pi, ci = ce.obs_list(prob)
    t0 = sc.t.reshape(-1, 3)
    rec = _native.pack_cameras(sc.K, prob.D, sc.R, t0)
    cams_out, X, rb, ra, rep = ctx.sba_extrinsics(rec, uv, pi, ci, prob.truth, ctx.sba_ext_opts(max_iters=max_iters))
    Xo, Ro, to, info = oext.sba_extrinsics(uv, prob.truth, pi.astype(np.int64), ci.astype(np.int64), sc.K, prob.D,
                                           sc.R, t0, max_iters=max_iters)
    print('extrinsics hub(6), max_iters %d: %d passes, max |X - oracle| %.2e m' % (max_iters, rep['iters'],
                                                                                    np.abs(X - Xo).max()))
    r0 = oext.residuals(prob.truth, sc.R, t0, sc.K, prob.D, uv, pi, ci).ravel()
    np.testing.assert_allclose(rb, r0, atol=1e-9)
    assert rep['status_name'] == info['status']
    assert rep['iters'] == info['iters'] and rep['n_accepted'] == info['n_accepted']
    assert abs(rep['lambda_final'] - info['lam']) <= 1e-12 * info['lam']
    assert abs(rep['cost_before'] - info['cost_before']) <= 1e-12 * info['cost_before']
    assert abs(rep['cost_after'] - info['cost_after']) <= 1e-12 * info['cost_after']
    np.testing.assert_allclose(X, Xo, rtol=0, atol=1e-9)
    np.testing.assert_allclose(cams_out[:, 8:17].reshape(-1, 3, 3), Ro, rtol=0, atol=1e-10)
    np.testing.assert_allclose(cams_out[:, 17:20], to.reshape(-1, 3), rtol=0, atol=1e-9)
    ro = oext.residuals(Xo, Ro, to, sc.K, prob.D, uv, pi, ci).ravel()
    np.testing.assert_allclose(ra, ro, atol=1e-8)


# ---- 5. triangulation ---------------------------------------------------------------------------

def _tri_check(label, cls, xyz, ref):
    err = np.abs(xyz - ref).max(1)
    worst = {}
    for c in sorted(set(cls)):
        m = cls == c
        worst[c] = float(err[m].max())
        print('%s %s: %d cases, max |gpu - reference| %.3e m (bound %.1e, |X| up to %.3g m)' % (
            label, c, m.sum(), worst[c], _tri_bound(c), np.abs(ref[m]).max()))
    for c, w in worst.items():
        assert w <= _tri_bound(c), (c, w, _tri_bound(c))
    return worst


def test_fisheye_pairs_at_the_edges(ctx):
    """T1 centre, T2 rim, T3 sentinel (and its converged neighbours), T4 far."""
    cams, cs = ce.tri_pair_cases()
    assert {c: int((cs.cls == c).sum()) for c in set(cs.cls)} == \
        {c: n for c, n in TRI_COUNTS.items() if c not in ('standard', 'dense')}
    ref = ce.tri_pair_reference(cams, cs)
    assert np.isfinite(ref).all()
    rec = _native.pack_cameras(cams.K, cams.D, cams.R, cams.t)
    xyz = ctx.triangulate_pairs(rec, cs.uva, cs.uvb, cs.ca, cs.cb)
    _tri_check('pairs', cs.cls, xyz, ref)
    # a camera id out of range gives NaN, and only there
    ca, cb = cs.ca.copy(), cs.cb.copy()
    ca[0], cb[1], ca[2] = cams.n, -1, 255
    out = ctx.triangulate_pairs(rec, cs.uva, cs.uvb, ca, cb)
    assert np.isnan(out[:3]).all()
    np.testing.assert_array_equal(_bits(out[3:]), _bits(xyz[3:]))


def test_standard_pairs_around_the_put_back(ctx):
    """T6: pixels for which standard_undistort's inverse radial factor turns negative, next to ones
    for which it does not."""
    cams, cs = ce.tri_standard_cases()
    hit = ce.standard_put_back(cams, cs)
    assert len(hit) == TRI_COUNTS['standard'] and hit.any() and not hit.all()
    ref = ce.tri_standard_reference(cams, cs)
    rec = _native.pack_cameras_standard(cams.K, cams.D, cams.R, cams.t)
    xyz = ctx.triangulate_pairs(rec, cs.uva, cs.uvb, cs.ca, cs.cb)
    _tri_check('pairs (%d put back, %d not)' % (hit.sum(), (~hit).sum()), cs.cls, xyz, ref)
    ca = cs.ca.copy()
    ca[0] = 6
    assert np.isnan(ctx.triangulate_pairs(rec, cs.uva, cs.uvb, ca, cs.cb)[0]).all()


@pytest.mark.parametrize('n', BLOCK_EDGE)
@pytest.mark.parametrize('C', [2, 3, 6])
def test_dense_triangulation_bookkeeping(ctx, C, n):
    """T5: the pair count and the mean over the pairs: all cameras, no adjacent pair, only the wrap
    pair (C - 1, 0); with two cameras the pairs (0, 1) and (1, 0) both count."""
    scene, uv, mask, kind = ce.tri_dense_problem(C, n)
    D, t = scene.D.reshape(-1, 4), scene.t.reshape(-1, 3)
    ref, cnt_ref = ce.triangulate_dense_ref(fisheye.triangulate_pair, uv, mask, scene.K, D, scene.R, t)
    xyz, cnt = ctx.triangulate_dense(_native.pack_cameras(scene.K, D, scene.R, t), uv, mask)
    np.testing.assert_array_equal(cnt, cnt_ref)
    want = {'all': C, 'none': 0, 'wrap': 2 if C == 2 else 1}
    for k, v in want.items():
        assert (cnt[kind == k] == v).all(), (k, v)
    assert n < 3 or set(kind) == set(want)
    none = cnt == 0
    assert np.isnan(xyz[none]).all() and np.isfinite(xyz[~none]).all()
    err = float(np.abs(xyz - ref)[~none].max())
    print('dense C = %d, n = %d: max |gpu - oracle| %.3e m' % (C, n, err))
    assert err <= _tri_bound('dense')


def test_dense_triangulation_standard_model(ctx):
    scene, uv, mask, kind = ce.tri_dense_problem(6, 257)
    co = ce.standard_coeffs(6)['five']
    t = scene.t.reshape(-1, 3)
    ref, cnt_ref = ce.triangulate_dense_ref(sm.triangulate_pair, uv, mask, scene.K, co, scene.R, t)
    xyz, cnt = ctx.triangulate_dense(_native.pack_cameras_standard(scene.K, co, scene.R, t), uv, mask)
    np.testing.assert_array_equal(cnt, cnt_ref)
    none = cnt == 0
    assert none.any() and np.isnan(xyz[none]).all()
    err = float(np.abs(xyz - ref)[~none].max())
    print('dense standard model: max |gpu - helper| %.3e m' % err)
    assert err <= _tri_bound('standard')
