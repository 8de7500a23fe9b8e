"""GPU: camera-pose and joint point covariances of the points + extrinsics SBA
(acs_sba_extrinsics_covariance) against the numpy restatement tests/sba_ext_cov_ref.py, evaluated
at the GPU solver's own solution (ctx.sba_extrinsics, 20 iterations, the solver's default
f_scale = 1; observations with 0.5 px noise).

Shapes: C = 2 / n = 12 (one tile, rank 5, lane groups of 2), C = 3 / n = 40 (18 rows cross the
16-row tile edge, groups of 4), the sba_extrinsics golden problem (6 cameras, 80 points, groups of
8), C = 16 / n = 400 (EXT_MAXC, 96 rows, groups of 16), `mixed` (16 cameras, points seen by 2..16
of them, plus one point without observation and two single-view points) and C = 3 with every
observation given 6 / 12 times (groups of 32 / 64).

Measure and bound. cov_cams against the helper's R in the measure max |S - R| / sqrt(diag R (x)
diag R) over the entries whose variances are non-zero (the anchor camera's rows and columns are
exact zeros and are compared as such), bounded by beta = C_BOUND cond2(Ah) 2.2e-16 with C_BOUND =
10, the constant of the FTE and points-only covariance tests; Ah = S + mu Q Q^T scaled to unit
diagonal is the matrix both sides invert. A point's record cov_i = sigma^2 V^-1 + V^-1 B^T cov_cc B
V^-1 is bounded entry by entry by the forward error of its two terms: a camera matrix within beta
s_a s_b of R (s = sqrt(diag R)) moves the second term by at most beta u_j u_k with u = |V^-1| |B^T|
s, and the point's own inverse contributes C_BOUND cond2(V_i) 2.2e-16 d_j d_k, d = sqrt(diag
cov_i):
    |cov_i - R_i|_jk <= C_BOUND 2.2e-16 (cond2(Ah) u_j u_k + cond2(V_i) d_j d_k).
(u_j u_k can exceed d_j d_k by far: B^T cov_cc B is a difference of large terms when the cameras a
point is seen by move together; on the golden problem, cond2(Ah) = 5.6e5 after 20 iterations, the
plain measure reaches 16 (cond2(Ah) + cond2(V)) 2.2e-16 on one point.) The measured maxima of
error / bound are printed by the tests and recorded in DESIGN §3.
"""
import json
import os

import numpy as np
import pytest

import sba_ext_cov_ref as xref
from conftest import golden
from acinoset_amd import _native
from acinoset_amd.lib import sba as lsba, utils as lutils

pytestmark = pytest.mark.gpu

EPS = 2.2e-16
C_BOUND = 10.0
NAME = 'acs_sba_extrinsics_covariance'
_cache = {}


def _noisy(n, C, seed=7, sizes=None):
    """xref.synthetic with 0.5 px noise and a perturbed start; `sizes`: cameras per point."""
    K, D, R, t, X, uv, pi, ci = xref.synthetic(n, C, seed)
    rng = np.random.default_rng(seed + 1)
    if sizes is not None:
        pi = np.repeat(np.arange(n), sizes).astype(np.int32)
        ci = np.concatenate([rng.choice(C, size=s, replace=False) for s in sizes]).astype(np.int32)
        uv = xref.oext.residuals(X, R, t, K, D.reshape(-1, 4), np.zeros((len(pi), 2)), pi, ci)
    uv = uv + rng.normal(0, 0.5, uv.shape)
    R0 = R.copy()
    t0 = t.copy()
    for c in range(1, C):
        R0[c] = xref.oext.rodrigues(rng.normal(0, 2e-3, 3)) @ R0[c]
        t0[c] += rng.normal(0, 5e-3, 3)
    return K, D, R0, t0, X + rng.normal(0, 5e-3, X.shape), uv, pi, ci


def _build(name):
    if name == 'golden':
        g = golden('sba_extrinsics')
        return (g['K'], g['D'].reshape(-1, 4), g['R0'], g['t0'].reshape(-1, 3), g['points_3d'], g['points_2d'],
                g['point_indices'].astype(np.int32), g['camera_indices'].astype(np.int32))
    if name == 'mixed':
        K, D, R, t, X, uv, pi, ci = _noisy(60, 16, 21, sizes=2 + np.arange(60) % 15)
        # point 60 has no observation, points 61 and 62 one each
        X = np.vstack([X, [[0.1, 0.2, 0.3]], X[:2] + 0.05])
        uv = np.vstack([uv, uv[pi == 0][:1], uv[pi == 1][:1]])
        ci = np.concatenate([ci, ci[pi == 0][:1], ci[pi == 1][:1]]).astype(np.int32)
        pi = np.concatenate([pi, [61, 62]]).astype(np.int32)
        return K, D, R, t, X, uv, pi, ci
    if name.startswith('dup'):
        K, D, R, t, X, uv, pi, ci = _noisy(40, 3)
        k = int(name[3:])
        rng = np.random.default_rng(5)
        uv = np.concatenate([uv + rng.normal(0, 0.2, uv.shape) for _ in range(k)])
        return K, D, R, t, X, uv, np.tile(pi, k), np.tile(ci, k)
    C, n = {'c2': (2, 12), 'c3': (3, 40), 'c16': (16, 400)}[name]
    return _noisy(n, C)


def _problem(ctx, name):
    """The problem solved once on the GPU: dict with cams (solution records), K, D, R, t, X, uv, pi, ci."""
    if name not in _cache:
        K, D, R0, t0, X0, uv, pi, ci = _build(name)
        cams0 = _native.pack_cameras(K, D, R0, t0)
        cams, X, _, _, rep = ctx.sba_extrinsics(cams0, uv, pi, ci, X0, ctx.sba_ext_opts(max_iters=20), residuals=False)
        _cache[name] = dict(cams=cams, K=K, D=D, R=cams[:, 8:17].reshape(-1, 3, 3).copy(), t=cams[:, 17:20].copy(),
                            X=X, uv=np.asarray(uv, np.float64), pi=pi, ci=ci, ref={})
    return _cache[name]


def _ref(p, gauge, anchor, sigma_px=1.0, f_scale=1.0):
    key = (gauge, anchor, sigma_px, f_scale)
    if key not in p['ref']:
        p['ref'][key] = xref.covariance(p['X'], p['R'], p['t'], p['K'], p['D'], p['uv'], p['pi'], p['ci'], f_scale,
                                        sigma_px, gauge, anchor)
    return p['ref'][key]


def _gpu(ctx, p, gauge, anchor, sigma_px=1.0, f_scale=1.0, **kw):
    return ctx.sba_extrinsics_covariance(p['cams'], kw.get('uv', p['uv']), kw.get('pi', p['pi']), kw.get('ci', p['ci']),
                                         p['X'], f_scale=f_scale, sigma_px=sigma_px, gauge=gauge, anchor=anchor)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _points_worst(cp, ref, cond, other=None):
    """max over the OK points and entries of |cp - R_i| / (2.2e-16 (cond2(Ah) u_j u_k + cond2(V_i) d_j d_k))
    (the module docstring's bound with C_BOUND = 1); R_i = `other` or the helper's records."""
    s = np.sqrt(ref['cov_cams'].diagonal())
    worst = 0.0
    for i in np.flatnonzero(ref['status'] == xref.OK):
        Vi = np.linalg.inv(ref['V'][i])
        u = np.abs(Vi) @ np.abs(ref['B'][i].T) @ s
        d = np.sqrt(ref['cov_points'][i].diagonal())
        unit = EPS * (cond * np.outer(u, u) + np.linalg.cond(ref['V'][i]) * np.outer(d, d))
        tgt = ref['cov_points'][i] if other is None else other[i]
        worst = max(worst, float((np.abs(cp[i] - tgt) / unit).max()))
    return worst


def _check(got, ref, gauge, anchor, label):
    cc, cp, st, rep = got
    r = ref['report']
    assert rep['status'] == r['status'] == 0
    np.testing.assert_array_equal(st, ref['status'])
    for k in ('n_points', 'n_ok', 'n_noobs', 'n_degenerate', 'dof'):
        assert rep[k] == r[k], k
    # exactly symmetric, the anchor camera exactly zero
    np.testing.assert_array_equal(_bits(cc), _bits(cc.T))
    np.testing.assert_array_equal(_bits(cp), _bits(np.swapaxes(cp, 1, 2)))
    if gauge == 'anchor':
        a = anchor[0]
        assert not cc[6 * a:6 * a + 6].any() and not cc[:, 6 * a:6 * a + 6].any()
        assert not ref['cov_cams'][6 * a:6 * a + 6].any()
    cond = np.linalg.cond(ref['Ah'])
    err = xref.rel_error(cc, ref['cov_cams'])
    ok = st == xref.OK
    assert np.isnan(cp[~ok]).all() and np.isfinite(cp[ok]).all() and np.isfinite(cc).all()
    worst_p = _points_worst(cp, ref, cond)
    print('%s %s %s: cond(Ah) %.4g, cameras error %.3g = %.3f cond eps; points worst %.3f of the unit bound; '
          'min pivot %.4g' % (label, gauge, anchor, cond, err, err / (cond * EPS), worst_p, rep['min_pivot']))
    assert err <= C_BOUND * cond * EPS
    assert worst_p <= C_BOUND
    np.testing.assert_allclose(rep['min_pivot'], r['min_pivot'], rtol=1e-6)
    np.testing.assert_allclose(rep['sigma_hat_px'], r['sigma_hat_px'], rtol=1e-9)
    np.testing.assert_allclose(rep['rot_sd_max'], r['rot_sd_max'], rtol=1e-9)
    np.testing.assert_allclose(rep['trans_sd_max'], r['trans_sd_max'], rtol=1e-9)
    sd = np.sqrt(cc.diagonal()).reshape(-1, 6)
    assert rep['rot_sd_max'] == sd[:, :3].max() and rep['trans_sd_max'] == sd[:, 3:].max()


CASES = [('c2', 'free', None), ('c2', 'anchor', (0, 1)), ('c2', 'anchor', (1, 0)),
         ('c3', 'free', None), ('c3', 'anchor', (0, 1)), ('c3', 'anchor', (2, 0)),
         ('golden', 'free', None), ('golden', 'anchor', (0, 3)), ('golden', 'anchor', (4, 1)),
         ('c16', 'free', None), ('c16', 'anchor', (0, 8)), ('c16', 'anchor', (15, 6)),
         ('mixed', 'free', None), ('mixed', 'anchor', (3, 11)),
         ('dup6', 'free', None), ('dup12', 'anchor', (1, 2))]


@pytest.mark.parametrize('name,gauge,anchor', CASES)
def test_matches_helper(ctx, name, gauge, anchor):
    p = _problem(ctx, name)
    anchor = anchor or (0, 1)
    _check(_gpu(ctx, p, gauge, anchor), _ref(p, gauge, anchor), gauge, anchor, name)


def test_sigma_px_and_f_scale(ctx):
    p = _problem(ctx, 'c3')
    got = _gpu(ctx, p, 'anchor', (0, 1), sigma_px=0.7, f_scale=50.0)
    _check(got, _ref(p, 'anchor', (0, 1), 0.7, 50.0), 'anchor', (0, 1), 'c3 sigma 0.7 f 50')


def test_mixed_statuses_and_s_unchanged_by_points_left_out(ctx):
    p = _problem(ctx, 'mixed')
    cc, cp, st, rep = _gpu(ctx, p, 'anchor', (3, 11))
    assert (rep['n_ok'], rep['n_noobs'], rep['n_degenerate']) == (60, 1, 2)
    np.testing.assert_array_equal(st[60:], [xref.NOOBS, xref.DEGENERATE, xref.DEGENERATE])
    assert np.isnan(cp[60:]).all() and np.isfinite(cp[:60]).all()
    keep = p['pi'] < 60
    q = dict(p, X=p['X'][:60])
    cc2, cp2, st2, rep2 = _gpu(ctx, q, 'anchor', (3, 11), uv=p['uv'][keep], pi=p['pi'][keep], ci=p['ci'][keep])
    np.testing.assert_array_equal(_bits(cc2), _bits(cc))
    np.testing.assert_array_equal(_bits(cp2), _bits(cp[:60]))
    assert rep2['sigma_hat_px'] == rep['sigma_hat_px'] and rep2['min_pivot'] == rep['min_pivot']


def _starved(p, cam, k):
    """Camera `cam` keeps only k observations, all of points two other cameras see."""
    pi, ci = p['pi'], p['ci']
    others = np.bincount(pi[ci != cam], minlength=len(p['X']))
    last = np.flatnonzero((ci == cam) & (others[pi] >= 2))
    keep = ci != cam
    keep[last[:k]] = True
    return dict(uv=p['uv'][keep], pi=pi[keep], ci=ci[keep])


@pytest.mark.parametrize('k', [3, 2, 0])
def test_degenerate_problem(ctx, k):
    p = _problem(ctx, 'golden')
    sub = _starved(p, 5, k)
    cc, cp, st, rep = _gpu(ctx, p, 'anchor', (0, 3), **sub)
    ref = xref.covariance(p['X'], p['R'], p['t'], p['K'], p['D'], sub['uv'], sub['pi'], sub['ci'], 1.0, 1.0, 'anchor',
                          (0, 3))
    print('k = %d: min pivot %.3g (helper %.3g)' % (k, rep['min_pivot'], ref['report']['min_pivot']))
    np.testing.assert_array_equal(st, ref['status'])
    assert rep['status'] == ref['report']['status'] == int(k < 3)
    if k < 3:
        assert rep['status_name'] == 'degenerate' and not rep['min_pivot'] > 1e-9
        assert np.isnan(cc).all() and np.isnan(cp).all()
        assert np.isnan(rep['rot_sd_max']) and np.isnan(rep['trans_sd_max'])
    else:
        assert rep['min_pivot'] > 1e-9 and np.isfinite(cc).all()
        np.testing.assert_allclose(rep['min_pivot'], ref['report']['min_pivot'], rtol=1e-6)


def test_one_camera_is_degenerate_not_an_error(ctx):
    p = _problem(ctx, 'c2')
    one = p['ci'] == 0
    for gauge in ('free', 'anchor'):
        cc, cp, st, rep = ctx.sba_extrinsics_covariance(p['cams'][:1], p['uv'][one], p['pi'][one], p['ci'][one], p['X'],
                                                        gauge=gauge, anchor=(0, 1))
        assert rep['status'] == 1 and cc.shape == (6, 6)
        assert np.isnan(cc).all() and np.isnan(cp).all()
        assert (st == xref.DEGENERATE).all() and rep['n_degenerate'] == 12


def test_validation_errors_stage_nothing(ctx):
    p = _problem(ctx, 'c3')
    _gpu(ctx, p, 'anchor', (0, 1))
    same = p['cams'].copy()
    same[1, 8:20] = same[0, 8:20]   # coincident centres
    std = np.zeros((3, _native.ACS_CAM_STRIDE_STD))
    big = _native.pack_cameras(*xref.synthetic(4, 16, 1)[:4])
    bad = [dict(f_scale=0.0), dict(f_scale=-1.0), dict(sigma_px=0.0), dict(anchor=(1, 1)), dict(anchor=(0, 3)),
           dict(anchor=(-1, 1)), dict(cams=same), dict(cams=std), dict(cams=np.vstack([big, big[:1]]))]
    before = _native.alloc_events()
    for kw in bad:
        args = dict(cams=p['cams'], f_scale=1.0, sigma_px=1.0, anchor=(0, 1))
        args.update(kw)
        with pytest.raises(RuntimeError, match=NAME):
            ctx.sba_extrinsics_covariance(args['cams'], p['uv'], p['pi'], p['ci'], p['X'], f_scale=args['f_scale'],
                                          sigma_px=args['sigma_px'], gauge='anchor', anchor=args['anchor'])
    assert _native.alloc_events() == before
    with pytest.raises(ValueError):
        _gpu(ctx, p, 'fixed', (0, 1))
    # a point index out of range is refused by name as well
    pi = p['pi'].copy()
    pi[0] = 10_000
    with pytest.raises(RuntimeError, match=NAME):
        _gpu(ctx, p, 'free', (0, 1), pi=pi)


def test_second_call_allocates_nothing(ctx):
    p = _problem(ctx, 'c16')
    first = _gpu(ctx, p, 'anchor', (0, 8))
    before = _native.alloc_events()
    again = _gpu(ctx, p, 'anchor', (0, 8))
    assert _native.alloc_events() == before
    np.testing.assert_array_equal(_bits(again[0]), _bits(first[0]))
    np.testing.assert_array_equal(_bits(again[1]), _bits(first[1]))


@pytest.mark.parametrize('name,anchor', [('c3', (0, 1)), ('c16', (0, 8)), ('golden', (0, 3))])
def test_observation_order_invariance(ctx, name, anchor):
    """Observations are regrouped per point, so a permutation of the list changes only the slot order
    inside a point: the summation order of S and of B^T cov_cc B. That moves cov_cams by about
    cond2(Ah) 2.2e-16 (2.8e-12 on c3, 4.4e-12 on c16) and a point's record by that times its
    cancellation factor u u^T / d d^T: 1e-9 relative holds with room on c3 and c16. On the golden
    problem cond2(Ah) 2.2e-16 is 1.2e-10 and the points reach 1.3e-9 (measured), so there the
    cameras are held to 1e-9 and the points to twice the helper comparison's bound."""
    p = _problem(ctx, name)
    base = _gpu(ctx, p, 'anchor', anchor)
    perm = np.random.default_rng(1).permutation(len(p['pi']))
    got = _gpu(ctx, p, 'anchor', anchor, uv=p['uv'][perm], pi=p['pi'][perm], ci=p['ci'][perm])
    ec = xref.rel_error(got[0], base[0])
    ep = max(xref.rel_error(got[1][i], base[1][i]) for i in range(len(p['X'])))
    ref = _ref(p, 'anchor', anchor)
    worst = _points_worst(got[1], ref, np.linalg.cond(ref['Ah']), other=base[1])
    print('%s: cameras %.3g, points %.3g relative (%.3f of the unit bound)' % (name, ec, ep, worst))
    np.testing.assert_array_equal(got[2], base[2])
    assert ec <= 1e-9
    if name == 'golden':
        assert worst <= 2 * C_BOUND
    else:
        assert ep <= 1e-9


def test_lib_default_is_byte_equal_and_covariance_adds_keys(ctx):
    g = golden('sba_extrinsics')
    args = (g['points_2d'], g['points_3d'], g['point_indices'], g['camera_indices'], g['K'], g['D'], g['R0'], g['t0'],
            None)
    plain = lsba.bundle_adjust_points_and_extrinsics(*args)
    off = lsba.bundle_adjust_points_and_extrinsics(*args, covariance=False)
    on = lsba.bundle_adjust_points_and_extrinsics(*args, covariance=True, sigma_px=0.5)
    assert set(plain[3]) == set(off[3]) == {'before', 'after'}
    for other in (off, on):
        for a, b in zip(plain[:3], other[:3]):
            assert a.tobytes() == b.tobytes()
        for k in ('before', 'after'):
            assert plain[3][k].tobytes() == other[3][k].tobytes()
    res = on[3]
    assert res['cov_cams'].shape == (36, 36) and res['cov_cam_blocks'].shape == (6, 6, 6)
    assert res['cov_points'].shape == (80, 3, 3) and res['cov_status'].shape == (80,)
    pair = lsba.default_anchor(on[1], on[2])
    assert res['cov_report']['gauge'] == 'anchor' and res['cov_report']['anchor'] == pair and pair[0] == 0
    np.testing.assert_array_equal(res['cov_cam_blocks'][2], res['cov_cams'][12:18, 12:18])
    assert not res['cov_cam_blocks'][0].any()
    ref = xref.covariance(on[0], on[1], on[2].reshape(-1, 3), g['K'], g['D'].reshape(-1, 4), g['points_2d'],
                          g['point_indices'], g['camera_indices'], 1.0, 0.5, 'anchor', pair)
    assert xref.rel_error(res['cov_cams'], ref['cov_cams']) <= C_BOUND * np.linalg.cond(ref['Ah']) * EPS
    free = lsba.bundle_adjust_points_and_extrinsics(*args, covariance=True, gauge='free')[3]
    assert free['cov_report']['anchor'] is None and free['cov_cam_blocks'][0].any()


def test_board_dropin_writes_cov_json_and_the_same_scene(ctx, tmp_path, monkeypatch):
    from acinoset_amd.lib import app

    class _Clock:   # save_scene stamps the wall clock into the scene JSON: hold it still
        @staticmethod
        def now():
            return '2000-01-01 00:00:00'
    monkeypatch.setattr(lutils, 'datetime', _Clock)
    G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'board.npz'))
    C = len(G['K'])
    pfs = []
    for c in range(C):
        f = tmp_path / f'points_cam{c}.json'
        f.write_text(str(G[f'points_cam{c}']))
        pfs.append(str(f))
    mf = tmp_path / 'manual_points.json'
    mf.write_text(str(G['manual_points_json']))
    scene = str(tmp_path / 'scene.json')
    lutils.save_scene(scene, G['K'], G['D'], G['R0'], G['t0'], tuple(int(v) for v in G['res']))
    out_a, out_b = str(tmp_path / 'a' / 'scene_sba.json'), str(tmp_path / 'b' / 'scene_sba.json')
    os.makedirs(os.path.dirname(out_a))
    os.makedirs(os.path.dirname(out_b))
    app.sba_board_points_fisheye(scene, pfs, out_a, manual_points_fpath=str(mf))
    res = app.sba_board_points_fisheye(scene, pfs, out_b, manual_points_fpath=str(mf), covariance=True, sigma_px=1.0)
    assert open(out_a, 'rb').read() == open(out_b, 'rb').read()
    assert os.listdir(os.path.dirname(out_a)) == ['scene_sba.json']
    with open(os.path.join(os.path.dirname(out_b), 'scene_sba_cov.json')) as f:
        cov = json.load(f)
    assert cov['status'] == 'ok' and cov['gauge'] == 'anchor' and cov['anchor'][0] == 0
    assert len(cov['cameras']) == C and cov['sigma_hat_px'] > 0
    _, _, R, t, _ = lutils.load_scene(out_b, verbose=False)
    for c, cam in enumerate(cov['cameras']):
        blk = np.array(cam['cov'])
        np.testing.assert_array_equal(blk, res['cov_cam_blocks'][c])
        np.testing.assert_allclose(cam['rotation_sd'], np.sqrt(blk.diagonal()[:3]))
        np.testing.assert_allclose(cam['translation_sd'], np.sqrt(blk.diagonal()[3:]))
        np.testing.assert_allclose(cam['centre_cov'], lsba.camera_centre_covariance(blk, R[c], t[c]), rtol=1e-6,
                                   atol=1e-18)
    assert not np.array(cov['cameras'][0]['cov']).any()
