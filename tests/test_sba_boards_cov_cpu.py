"""CPU: the definition of the rigid-board SBA's covariances (tests/sba_boards_cov_ref.py, restating
DESIGN §3 / include/acinoset_hip.h) checked against the dense normal matrix of
sba_boards_ref.dense_jacobian and against the real scatter of the numpy solver, and the Python entry
points' new arguments.

Bounds. Identities between two formulations of one inverse are bounded by 10 cond2(Ah) 2.2e-16 in
the measure max |A - B| / sqrt(diag B (x) diag B), Ah the unit-diagonal matrix that is inverted (the
constant of the GPU covariance tests). The Monte-Carlo band is the sampling error of a variance from
N draws, 4 sqrt(2 / (N - 1)), plus the linearisation bias measured once at 8000 draws.
"""
import inspect
import os
import re

import numpy as np
import pytest

import sba_boards_cov_ref as cref
import sba_boards_ref as bref
import sba_ext_cov_ref as xref
from conftest import REPO

EPS = 2.2e-16
# the shapes of tests/test_gpu_sba_boards.py
SHAPES = {
    'c2_b2_nc4': (2, 2, (2, 2), None),
    'c3_b5_nc12': (3, 5, (4, 3), None),
    'c16_b40_nc54': (16, 40, (9, 6), (2, 16)),
    'nc70': (3, 4, (10, 7), (2, 3)),
    'nc256': (2, 3, (16, 16), None),
}
_RIGS = {}


def _rig(name):
    if name not in _RIGS:
        C, B, shape, views = SHAPES[name]
        _RIGS[name] = bref.make_rig(C, B, shape=shape, views=views)
    return _RIGS[name]


def _cov(rig, f_scale=1.0, sigma_px=1.0, gauge='anchor', anchor=0, **kw):
    a = {k: kw.get(k, rig[k]) for k in ('R', 't', 'K', 'D', 'obj', 'bR', 'bt', 'uv', 'mask')}
    return cref.covariance(a['R'], a['t'], a['K'], a['D'], a['obj'], a['bR'], a['bt'], a['uv'], a['mask'], f_scale,
                           sigma_px, gauge, anchor)


@pytest.mark.parametrize('name', list(SHAPES))
def test_generators_annihilate_the_dense_normal_matrix(name):
    rig = _rig(name)
    J = bref.dense_jacobian(rig['R'], rig['t'], rig['K'], rig['D'], rig['obj'], rig['bR'], rig['bt'], rig['mask'])
    H = J.T @ J
    G = np.vstack([cref.gauge_generators(rig['R']), cref.board_generators(rig['bt'])])
    assert np.linalg.matrix_rank(G) == 6
    assert np.linalg.norm(H @ G) <= 1e-14 * np.linalg.norm(H) * np.linalg.norm(G)
    w = np.sort(np.abs(np.linalg.eigvalsh(H)))
    print('%s: eigenvalue 6 %.3g, 7 %.3g of the largest' % (name, w[5] / w[-1], w[6] / w[-1]))
    assert w[5] <= 1e-12 * w[-1] and w[6] >= 1e-7 * w[-1]
    # ... and the cameras' parts alone annihilate the reduced system
    r = _cov(rig)
    assert np.abs(r['S'] @ r['G']).max() <= 1e-13 * np.abs(r['S']).max()


@pytest.mark.parametrize('name', list(SHAPES))
def test_free_gauge_is_the_pseudo_inverse(name):
    rig = _rig(name)
    r = _cov(rig, gauge='free')
    assert r['report']['status'] == 0
    err = xref.rel_error(r['cov_cams'], np.linalg.pinv(r['S']))
    bound = 10 * np.linalg.cond(r['Ah']) * EPS
    print('%s: |free - pinv| %.3g, bound %.3g' % (name, err, bound))
    assert err <= bound
    r2 = _cov(rig, gauge='free', sigma_px=2.0)
    np.testing.assert_allclose(r2['cov_cams'], 4.0 * r['cov_cams'], rtol=1e-14)
    np.testing.assert_allclose(r2['cov_boards'], 4.0 * r['cov_boards'], rtol=1e-14)


@pytest.mark.parametrize('name,a', [('c2_b2_nc4', 0), ('c2_b2_nc4', 1), ('c3_b5_nc12', 0), ('c3_b5_nc12', 2),
                                    ('c16_b40_nc54', 0), ('c16_b40_nc54', 11), ('nc70', 1), ('nc256', 1)])
def test_anchored_covariances_are_blocks_of_the_dense_inverse(name, a):
    """At the true poses the residuals vanish, so the Triggs weights are 1 and the helper's S is the
    Schur complement of the unweighted dense J^T J."""
    rig = _rig(name)
    C, B = rig['mask'].shape[1], rig['mask'].shape[0]
    r = _cov(rig, anchor=a)
    full, _ = cref.dense_anchor_inverse(rig['R'], rig['t'], rig['K'], rig['D'], rig['obj'], rig['bR'], rig['bt'],
                                        rig['mask'], a)
    bound = 10 * np.linalg.cond(r['Ah']) * EPS
    ec = xref.rel_error(r['cov_cams'], full[:6 * C, :6 * C])
    eb = max(xref.rel_error(r['cov_boards'][b], full[6 * (C + b):6 * (C + b) + 6, 6 * (C + b):6 * (C + b) + 6])
             for b in range(B))
    print('%s anchor %d: cameras %.3g, boards %.3g, bound %.3g, min pivot %.3g' % (name, a, ec, eb, bound,
                                                                                     r['report']['min_pivot']))
    assert ec <= bound and eb <= bound
    assert not r['cov_cams'][6 * a:6 * a + 6].any() and not r['cov_cams'][:, 6 * a:6 * a + 6].any()
    np.testing.assert_array_equal(r['cov_cams'], r['cov_cams'].T)
    np.testing.assert_array_equal(r['cov_boards'], np.swapaxes(r['cov_boards'], 1, 2))
    rep = r['report']
    assert rep['n_ok'] == B and rep['dof'] == 2 * len(rig['obj']) * int(rig['mask'].sum()) - 6 * B - (6 * C - 6)


def test_single_view_board_is_ok():
    rig = _rig('c3_b5_nc12')
    mask = rig['mask'].copy()
    mask[2] = [0, 1, 0]
    r = _cov(rig, mask=mask)
    assert (r['status'] == cref.OK).all() and r['report']['status'] == 0
    assert np.isfinite(r['cov_boards']).all()
    # ... and carries no information about the cameras: S is that of the other four boards
    keep = [0, 1, 3, 4]
    r4 = _cov(rig, mask=mask[keep], uv=rig['uv'][keep], bR=rig['bR'][keep], bt=rig['bt'][keep])
    np.testing.assert_allclose(r['S'], r4['S'], rtol=0, atol=1e-9 * np.abs(r4['S']).max())


def test_collinear_target_is_degenerate():
    obj = np.array([[0.0, 0, 0], [0.1, 0, 0], [0.2, 0, 0]])
    rig = bref.make_rig(3, 4, obj=obj)
    r = _cov(rig)
    assert (r['status'] == cref.DEGENERATE).all()
    rep = r['report']
    assert rep['status'] == 1 and rep['n_degenerate'] == 4 and rep['n_ok'] == 0
    assert np.isnan(r['cov_cams']).all() and np.isnan(r['cov_boards']).all()
    assert np.isnan(rep['rot_sd_max']) and np.isnan(rep['board_trans_sd_max']) and np.isnan(rep['sigma_hat_px'])
    assert not r['S'].any()


# the third point eps off the line of the first two: the smallest pivot of the boards' unit-diagonal
# V falls with eps^2 (measured: 2.3e-9 .. 2.2e-8 at 1e-5, 2.0e-9 / 5.0e-10 / 2.1e-10 / 2.7e-10 at 3e-6,
# <= 8.8e-10 at 2e-6)
@pytest.mark.parametrize('eps,expect', [(1e-5, [0, 0, 0, 0]), (3e-6, [0, 2, 2, 2]), (2e-6, [2, 2, 2, 2])])
def test_board_pivot_on_its_side_of_the_threshold(eps, expect):
    obj = np.array([[0.0, 0, 0], [0.1, 0, 0], [0.2, eps, 0]])
    rig = bref.make_rig(3, 4, obj=obj)
    sys_ = cref.reduced_system(rig['R'], rig['t'], rig['K'], rig['D'], rig['obj'], rig['bR'], rig['bt'], rig['uv'],
                               rig['mask'], 1.0)
    piv = np.array([xref.ldl_pivots(cref.unit_diagonal(v)[0]).min() for v in sys_['V']])
    print('eps %g: smallest pivots %s' % (eps, piv))
    np.testing.assert_array_equal(sys_['status'], expect)
    np.testing.assert_array_equal(piv > cref.PIVOT_TOL, np.array(expect) == cref.OK)
    assert ((piv > 5e-11) & (piv < 3e-8)).all()   # every one within a decade and a half of the threshold on its side
    r = _cov(rig)
    # one OK board alone leaves the cameras undetermined
    assert r['report']['status'] == int(sum(e == 0 for e in expect) < 2)


def test_camera_seen_by_no_ok_board_is_degenerate():
    rig = _rig('c3_b5_nc12')
    mask = rig['mask'].copy()
    mask[:, 2] = 0
    r = _cov(rig, mask=mask)
    assert (r['status'] == cref.OK).all()
    rep = r['report']
    assert rep['status'] == 1 and not rep['min_pivot'] > 1e-9
    assert np.isnan(r['cov_cams']).all() and np.isnan(r['cov_boards']).all()


@pytest.mark.parametrize('gauge', ['free', 'anchor'])
def test_one_camera(gauge):
    rig = _rig('c3_b5_nc12')
    one = dict(R=rig['R'][:1], t=rig['t'][:1], K=rig['K'][:1], D=rig['D'][:1], uv=rig['uv'][:, :1],
               mask=rig['mask'][:, :1])
    r = _cov(rig, sigma_px=0.5, gauge=gauge, **one)
    rep = r['report']
    assert rep['status'] == 0 and r['cov_cams'].shape == (6, 6) and not r['cov_cams'].any()
    assert rep['rot_sd_max'] == 0.0 and rep['trans_sd_max'] == 0.0 and np.isnan(rep['min_pivot'])
    assert rep['dof'] == 2 * 12 * 5 - 6 * 5
    for b in range(5):
        vi = 0.25 * np.linalg.inv(r['V'][b])
        np.testing.assert_allclose(r['cov_boards'][b], 0.5 * (vi + vi.T), rtol=1e-13)


def test_boards_that_are_not_ok_leave_s_unchanged():
    rig = _rig('c3_b5_nc12')
    base = _cov(rig)
    # board 5 unseen; board 6 a copy of board 0 with NaN corners in its one view
    mask = np.concatenate([rig['mask'], [[0, 0, 0], [1, 0, 0]]]).astype(np.uint8)
    uv = np.concatenate([rig['uv'], np.zeros_like(rig['uv'][:1]), rig['uv'][:1]])
    uv[6, 0, 0] = np.nan
    bR = np.concatenate([rig['bR'], rig['bR'][:2]])
    bt = np.concatenate([rig['bt'], rig['bt'][:2]])
    r = _cov(rig, mask=mask, uv=uv, bR=bR, bt=bt)
    np.testing.assert_array_equal(r['status'], [0, 0, 0, 0, 0, cref.NOOBS, cref.DEGENERATE])
    np.testing.assert_array_equal(r['S'], base['S'])
    np.testing.assert_array_equal(r['cov_cams'], base['cov_cams'])
    np.testing.assert_array_equal(r['cov_boards'][:5], base['cov_boards'])
    assert np.isnan(r['cov_boards'][5:]).all()
    rep = r['report']
    assert (rep['n_boards'], rep['n_ok'], rep['n_noobs'], rep['n_degenerate']) == (7, 5, 1, 1)
    assert rep['sigma_hat_px'] == base['report']['sigma_hat_px'] and rep['dof'] == base['report']['dof']


def _log_so3(R):
    c = np.clip((np.trace(R) - 1) * 0.5, -1.0, 1.0)
    th = np.arccos(c)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * 0.5
    return v if th < 1e-12 else v * (th / np.sin(th))


MC_DRAWS = 2000
MC_LIN_BIAS = 0.04   # measured at 8000 draws, see the test's docstring


def test_monte_carlo_scatter_of_the_numpy_solver():
    """MC_DRAWS noise draws (sigma = 1 px, f_scale = 50, seeds 1000 + k, started at the truth) of
    sba_boards_ref.sba_boards on the 3-camera / 5-board / 4 x 3 rig, each solution moved by the rigid
    motion that puts camera 0 on its true pose. Along every camera axis (12) and board axis (30) the
    sample variance over the anchored prediction lies within 1 +- (4 sqrt(2 / (N - 1)) + MC_LIN_BIAS).
    MC_LIN_BIAS: at 8000 draws (sampling sd of a ratio 0.016) the ratios lay in 0.979 .. 1.019 over the
    camera axes and 0.967 .. 1.039 over the board axes, which 42 axes reach by sampling alone (2.5 sd);
    at 300 draws the same seeds with sigma = 0.3 px move the extreme ratios by at most 0.0012, so the
    part that grows with the noise is of that order. The linearisation bias is not resolved at 8000
    draws; its allowance is the largest deviation seen there, 0.04."""
    rig = _rig('c3_b5_nc12')
    R, t, K, D, obj, bR, bt, uv0, mask = (rig[k] for k in ('R', 't', 'K', 'D', 'obj', 'bR', 'bt', 'uv', 'mask'))
    pred = _cov(rig, f_scale=50.0, sigma_px=1.0, anchor=0)
    assert pred['report']['status'] == 0
    N = MC_DRAWS
    dc, db = np.empty((N, 18)), np.empty((N, 30))
    ct = -R[0].T @ t[0]
    for k in range(N):
        uv = uv0 + np.random.default_rng(1000 + k).normal(0, 1.0, uv0.shape)
        Rs, ts, bRs, bts, _ = bref.sba_boards(R, t, K, D, obj, bR, bt, uv, mask, f_scale=50.0)
        # X' = Q X + tau: R' = R Q^T, t' = t - R' tau; boards R_b' = Q R_b, t_b' = Q t_b + tau
        Q = R[0].T @ Rs[0]
        tau = ct - Q @ (-Rs[0].T @ ts[0])
        Ra = Rs @ Q.T
        ta = ts - np.einsum('cij,j->ci', Ra, tau)
        bRa = np.einsum('ij,bjk->bik', Q, bRs)
        bta = bts @ Q.T + tau
        for c in range(3):
            dc[k, 6 * c:6 * c + 3] = _log_so3(Ra[c] @ R[c].T)
            dc[k, 6 * c + 3:6 * c + 6] = ta[c] - t[c]
        for b in range(5):
            db[k, 6 * b:6 * b + 3] = _log_so3(bRa[b] @ bR[b].T)
            db[k, 6 * b + 3:6 * b + 6] = bta[b] - bt[b]
    assert np.abs(dc[:, :6]).max() <= 1e-9   # the anchor camera did not move
    vc = pred['cov_cams'].diagonal()[6:]
    vb = np.concatenate([c.diagonal() for c in pred['cov_boards']])
    rc = dc[:, 6:].var(0, ddof=1) / vc
    rb = db.var(0, ddof=1) / vb
    band = 4 * np.sqrt(2.0 / (N - 1)) + MC_LIN_BIAS
    print('cameras: variance ratios %.3f..%.3f; boards %.3f..%.3f; band %.3f' % (rc.min(), rc.max(), rb.min(),
                                                                                  rb.max(), band))
    assert np.abs(rc - 1).max() <= band and np.abs(rb - 1).max() <= band


def test_header_and_symbols_carry_the_new_names():
    from acinoset_amd import _native
    with open(os.path.join(REPO, 'include', 'acinoset_hip.h')) as f:
        text = f.read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    m = re.search(r'int acs_sba_boards_covariance\(([^;]*)\);', code)
    assert m, 'acs_sba_boards_covariance prototype missing from include/acinoset_hip.h'
    args = [a.strip().split()[-1].lstrip('*') for a in m.group(1).replace('\n', ' ').split(',')]
    assert args == ['ctx', 'cams', 'n_cams', 'obj_pts', 'n_corners', 'uv', 'mask', 'n_boards', 'board_poses', 'opts',
                    'cov_cams', 'cov_boards', 'board_status', 'report', 'flags']
    assert 'acs_sba_boards_cov_report' in code and re.search(r'^#define ACS_ABI_VERSION 5$', text, re.M)
    assert 'acs_sba_boards_covariance' in _native.SYMBOLS
    fn = _native.load_library().acs_sba_boards_covariance
    assert fn.argtypes is not None and len(fn.argtypes) == 15
    assert _native.C.sizeof(_native.SbaBoardsCovReport) == 8 + 5 * 8 + 6 * 8
    assert set(_native.SbaBoardsCovReport().as_dict()) >= {'status_name', 'n_boards', 'board_rot_sd_max', 'dof'}


def test_python_entry_points_carry_the_new_arguments(monkeypatch):
    from acinoset_amd import _native
    from acinoset_amd.lib import app, sba as lsba
    p = inspect.signature(_native.Context.sba_boards_covariance).parameters
    assert list(p)[1:7] == ['cams', 'obj_pts', 'uv', 'mask', 'board_r', 'board_t']
    assert (p['f_scale'].default, p['sigma_px'].default, p['gauge'].default, p['anchor'].default) == (1.0, 1.0,
                                                                                                      'anchor', 0)
    p = inspect.signature(lsba.bundle_adjust_boards_and_extrinsics).parameters
    assert p['covariance'].default is False and p['sigma_px'].default == 1.0
    assert p['gauge'].default == 'anchor' and p['anchor'].default is None
    for fn in (lsba._sba_board_poses, app.sba_board_poses_fisheye):
        p = inspect.signature(fn).parameters
        assert p['covariance'].default is False and p['sigma_px'].default == 1.0

    # without covariance the new binding is never reached; with it, once, at the solver's answer
    rig = _rig('c2_b2_nc4')
    calls = []

    class _Ctx:
        def sba_ext_opts(self, **kw):
            return kw

        def sba_boards(self, cams, obj, uv, mask, br, bt, o):
            rep = dict(iters=0, cost_before=0.0, cost_after=0.0, status_name='gtol')
            return np.asarray(cams), np.asarray(br) + 0.0, np.asarray(bt) + 1.0, np.zeros(1), np.zeros(1), rep

        def sba_boards_covariance(self, cams, obj, uv, mask, br, bt, **kw):
            calls.append((np.asarray(bt).copy(), kw))
            rep = dict(status=0, status_name='ok', rot_sd_max=0.0, trans_sd_max=0.0, sigma_hat_px=1.0)
            return np.zeros((12, 12)), np.zeros((2, 6, 6)), np.zeros(2, np.int32), rep

    monkeypatch.setattr(_native, 'default_context', lambda: _Ctx())
    args = (rig['uv'], rig['mask'], rig['obj'], rig['bR'], rig['bt'], rig['K'], rig['D'], rig['R'], rig['t'])
    out = lsba.bundle_adjust_boards_and_extrinsics(*args)
    assert not calls and set(out[4]) == {'before', 'after', 'report'}
    out = lsba.bundle_adjust_boards_and_extrinsics(*args, covariance=False)
    assert not calls and set(out[4]) == {'before', 'after', 'report'}
    out = lsba.bundle_adjust_boards_and_extrinsics(*args, f_scale=3.0, covariance=True, sigma_px=0.5)
    assert len(calls) == 1
    np.testing.assert_array_equal(calls[0][0], rig['bt'] + 1.0)
    assert calls[0][1] == dict(f_scale=3.0, sigma_px=0.5, gauge='anchor', anchor=0)
    assert set(out[4]) == {'before', 'after', 'report', 'cov_cams', 'cov_cam_blocks', 'cov_boards', 'cov_status',
                           'cov_report'}
    assert out[4]['cov_cam_blocks'].shape == (2, 6, 6) and out[4]['cov_report']['anchor'] == 0
    out = lsba.bundle_adjust_boards_and_extrinsics(*args, covariance=True, gauge='free', anchor=1)
    assert out[4]['cov_report']['gauge'] == 'free' and out[4]['cov_report']['anchor'] is None
