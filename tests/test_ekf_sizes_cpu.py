"""CPU: what tests/test_gpu_ekf_sizes.py rests on, from the oracle alone (tests/ekf_sizes.py).

* kinematics.build_table after its split into table_from_tree: the blobs of all five modes are
  byte-identical to the ones recorded before the split (tests/golden/skeleton_tables.npz).
* oracle.ekf.filter_step / rts_step chained reproduce oracle.ekf.ekf bit for bit; the information
  form and the solving RTS step agree with them to rounding.
* The truncated skeletons: the tables' shapes, and h / H equal to the embedded default_nolure
  oracle's.
* The conditions of the GPU cases: every P_pred a gain inverts (frames >= 1) of a regular clip is
  positive definite, so no gain is flagged to the pivoted kernel; every one of an "indefinite"
  clip (Q[5,5] = -1) has a negative eigenvalue, so every gain is. The tolerance rule gives finite,
  small, non-zero numbers.
"""
import numpy as np
import pytest

import ekf_sizes as es
from conftest import golden
from acinoset_amd import kinematics as pkin
from oracle import ekf as oekf, kinematics as okin

INDEFINITE = ('neck10', 'upper_body', 'front18', 'default_nolure')


def test_build_table_blobs_unchanged_by_the_split():
    g = golden('skeleton_tables')
    assert sorted(g.files) == sorted(f'{m}_{k}' for m in pkin.FK_MODES for k in ('ints', 'reals'))
    for m in pkin.FK_MODES:
        t = pkin.build_table(m)
        assert t.mode == m
        assert t.ints.dtype == g[f'{m}_ints'].dtype and t.ints.tobytes() == g[f'{m}_ints'].tobytes()
        assert t.reals.dtype == g[f'{m}_reals'].dtype and t.reals.tobytes() == g[f'{m}_reals'].tobytes()


def test_truncated_tables_shapes():
    n10, f18 = es.case('neck10').table, es.case('front18').table
    assert (n10.P, n10.L, n10.n_joints, n10.n_nodes) == (10, 4, 2, 5)
    assert n10.params == ['x_0', 'y_0', 'z_0', 'phi_0', 'theta_0', 'psi_0', 'l_1', 'phi_1', 'theta_1', 'psi_1']
    assert n10.markers == ['nose', 'r_eye', 'l_eye', 'neck_base']
    assert (f18.P, f18.L, f18.n_joints, f18.n_nodes) == (18, 14, 8, 15)
    gone = {'theta_4', 'psi_4', 'theta_5', 'psi_5', 'theta_10', 'theta_11', 'theta_12', 'theta_13'}
    assert f18.params == [p for p in pkin.get_pose_params('default_nolure') if p not in gone]
    assert f18.markers == [m for m in pkin.get_markers('default_nolure')
                           if m not in ('tail1', 'tail2', 'r_back_knee', 'r_back_ankle', 'l_back_knee',
                                        'l_back_ankle')]
    for t in (n10, f18):   # the blob sizes acs_ekf_run checks
        assert len(t.ints) == pkin.INT_HDR + 9 * t.n_joints + 4 * t.n_nodes + t.L + 4 * t.P + t.n_nodes * t.P
        assert len(t.reals) == 3 * t.n_nodes


@pytest.mark.parametrize('name', ['neck10', 'front18'])
def test_truncated_measurement_model_is_the_embedded_default_nolure(name):
    """The kept markers do not depend on the dropped parameters: positions, h and H of the
    truncated model are those of default_nolure at the embedded pose, whatever the dropped
    parameters' derivative columns hold; the dropped columns of the kept rows are zero."""
    c = es.case(name)
    m = c.model
    rng = np.random.default_rng(5)
    x = c.s0[:c.P] + rng.normal(0, 0.2, c.P)
    full = m.embed(x)
    np.testing.assert_array_equal(m.positions(x)[0], okin.marker_positions(es.FULL, full[None])[0][m.kept])
    cam = tuple(v[3] for v in c.cams)
    hf, Hf = oekf.analytic_jacobian(full, es.FULL, *cam)
    rows = np.stack([2 * m.kept, 2 * m.kept + 1], 1).ravel()
    np.testing.assert_allclose(m.h(x, cam), hf[rows], rtol=0, atol=1e-10)
    np.testing.assert_allclose(m.H(x, cam, 'analytic'), Hf[np.ix_(rows, m.cols)], rtol=0, atol=1e-9)
    dropped = np.setdiff1d(np.arange(m.Pfull), m.cols)
    assert np.abs(Hf[np.ix_(rows, dropped)]).max() == 0.0
    _, Hd = oekf.fd_jacobian(full, es.FULL, *cam, ref_numerics=False)
    np.testing.assert_allclose(m.H(x, cam, 'fd'), Hd[np.ix_(rows, m.cols)], rtol=0, atol=1e-9)
    # a shipped mode through the same Model class: oracle.ekf's own functions
    u = es.case('upper_body')
    xu = u.s0[:u.P]
    hu, Hu = oekf.analytic_jacobian(xu, 'upper_body', *cam)
    np.testing.assert_allclose(u.model.h(xu, cam), hu, rtol=0, atol=1e-10)
    np.testing.assert_allclose(u.model.H(xu, cam, 'analytic'), Hu, rtol=0, atol=1e-9)


@pytest.mark.parametrize('mode,jacobian', [('head', 'fd'), ('head', 'analytic'), ('upper_body', 'fd'),
                                           ('default', 'analytic')])
def test_chained_steps_are_ekf_bit_for_bit(mode, jacobian):
    """oracle.ekf.ekf on a mode name, against filter_step and rts_step chained by hand."""
    c = es.case(mode)
    N = 5
    K, D, R, t = c.cams
    covs = [oekf.CAL_COVS[k % 6] for k in range(es.N_CAMS)]
    for ref_numerics in ((True, False) if jacobian == 'fd' else (False,)):
        o = oekf.ekf(c.meas[:N], c.lik[:N], K, D, R, t, mode, es.FPS, c.s0, 0.5, c.max_pixel_err,
                     ref_numerics=ref_numerics, cal_covs=covs, jacobian=jacobian, Q=c.Q, P0=c.P0)
        s, Pm, outl = c.s0, c.P0, 0
        est = []
        for i in range(N):
            xp, Pp, s, Pm, k = oekf.filter_step(mode, c.cams, s, Pm, c.meas[i], c.lik[i], c.F, c.Q, es.ST, c.base,
                                                0.5, c.max_pixel_err, ref_numerics, jacobian)
            est.append((xp, Pp, s, Pm))
            outl += k
            for key, v in zip(('x_pred', 'P_pred', 'x_est', 'P_est'), est[-1]):
                np.testing.assert_array_equal(o[key][i], v)
        assert outl == o['outliers']
        xs, Ps = est[-1][2], est[-1][3]
        np.testing.assert_array_equal(o['x_smooth'][-1], xs)
        for i in range(N - 2, -1, -1):
            xs, Ps = oekf.rts_step(est[i][2], est[i][3], est[i + 1][0], est[i + 1][1], xs, Ps, c.F)
            np.testing.assert_array_equal(o['x_smooth'][i], xs)
            np.testing.assert_array_equal(o['P_smooth'][i], Ps)
            np.testing.assert_array_equal(oekf.rts_step(est[i][2], est[i][3], est[i + 1][0], est[i + 1][1],
                                                        o['x_smooth'][i + 1], None, c.F)[0], xs)


@pytest.mark.parametrize('name', es.SIZES)
def test_tolerance_rule_and_regular_clip_conditions(name):
    """Per size (analytic H; the forward-difference numbers are in test_gpu_ekf_sizes' docstring):
    the rule's two numbers are finite and far below the trajectory tolerances of test_gpu_ekf.py,
    the two forms count the same outliers, and every P_pred a gain inverts is positive definite."""
    c = es.case(name)
    o = es.oracle_run(name, 'analytic')
    forms, ulp = es.bound_parts(name, 'analytic')
    d = es.bounds(name, 'analytic')
    assert set(d) == {'xp', 'dxp', 'ddxp', 'x', 'dx', 'ddx', 'P_est', 'x_smooth', 'P_smooth'}
    for k, v in d.items():
        assert np.isfinite(v) and v == max(forms[k], ulp[k])
        assert 0 < es.MARGIN * v < {'xp': 1e-12, 'dxp': 1e-12, 'ddxp': 1e-10, 'x': 5e-8, 'dx': 5e-8, 'ddx': 5e-7,
                                    'P_est': 1e-8, 'x_smooth': 1e-6, 'P_smooth': 1e-8}[k], (k, v)
    assert forms['xp'] == forms['dxp'] == forms['ddxp'] == 0.0      # one prediction, both forms
    outl = 0
    for i in range(es.N_FRAMES):
        s_prev, P_prev = (c.s0, c.P0) if i == 0 else (o['x_est'][i - 1], o['P_est'][i - 1])
        a = es.filter_step(c, 'analytic', s_prev, P_prev, i)
        b = es.filter_step(c, 'analytic', s_prev, P_prev, i, oekf.filter_step_information)
        np.testing.assert_array_equal(a[2], o['x_est'][i])
        assert a[4] == b[4]
        outl += a[4]
    assert outl == o['outliers']
    for i in range(1, es.N_FRAMES):
        Pp = o['P_pred'][i]
        assert np.linalg.eigvalsh((Pp + Pp.T) / 2).min() > 1e-7, i     # measured >= 4e-7 on every size
    assert np.isfinite(o['x_smooth']).all() and np.isfinite(o['P_smooth']).all()


@pytest.mark.parametrize('name', INDEFINITE)
def test_indefinite_clip_conditions(name):
    """Q[5,5] = -1: every P_pred a gain inverts has a negative eigenvalue (so the tiled gain
    kernels, which take positive scalar pivots, must flag every gain), the oracle stays finite
    and its rule's numbers stay small."""
    c = es.case(name, es.N_FRAMES, True)
    assert c.Q[5, 5] == -1.0 and es.case(name).Q[5, 5] > 0
    o = es.oracle_run(name, 'analytic', es.N_FRAMES, True)
    for i in range(1, es.N_FRAMES):
        Pp = o['P_pred'][i]
        assert np.linalg.eigvalsh((Pp + Pp.T) / 2).min() < -0.5, i
    assert all(np.isfinite(o[k]).all() for k in ('x_est', 'P_est', 'x_smooth', 'P_smooth'))
    d = es.bounds(name, 'analytic', es.N_FRAMES, True)
    assert all(np.isfinite(v) and es.MARGIN * v < 1e-5 for v in d.values()), d


def _step_with_one_wrong_schur_entry(model, cams, s_prev, P_prev, meas_i, lik_i, F, Q, sT, base, thresh,
                                     max_pixel_err, ref_numerics, jacobian):
    """oracle.ekf.filter_step_information with A[1, 2] off by 1e-7 relative."""
    P = oekf.model_P(model)
    s = oekf.predict(np.asarray(s_prev, np.float64), sT, P, ref_numerics)
    Pm = F @ P_prev @ F.T + Q
    h, H = oekf.measurement_model(model, s[:P], cams, jacobian, ref_numerics)
    Hx = H[:, :P]
    w = 1.0 / oekf.measurement_std(base, lik_i, thresh, max_pixel_err) ** 2
    resid = np.nan_to_num(np.asarray(meas_i).reshape(-1) - h)
    A = Hx.T @ (w[:, None] * Hx)
    A[1, 2] *= 1 + 1e-7
    V = np.linalg.inv(np.eye(P) + A @ Pm[:P, :P])
    return s, Pm, s + Pm[:, :P] @ (V @ (Hx.T @ (w * resid))), Pm - Pm[:, :P] @ (V @ A) @ Pm[:P, :], 0


@pytest.mark.parametrize('name', es.SIZES)
def test_rule_sees_a_1e7_error_in_one_schur_entry(name):
    """What the step check buys: one entry of A = Hx^T R^-1 Hx off by 1e-7 relative, which the
    trajectory tolerances of test_gpu_ekf.py cannot see, passes MARGIN x d_q in every analytic-H
    case (by 1.4 .. 9 x). The forward-difference cases are less sharp, because an ulp of the pose
    already moves their H by 1e-13: there the same error is 0.02 .. 0.1 of the tolerance."""
    c = es.case(name)
    o = es.oracle_run(name, 'analytic')
    d = es.bounds(name, 'analytic')
    worst = {}
    for i in range(es.N_FRAMES):
        s_prev, P_prev = (c.s0, c.P0) if i == 0 else (o['x_est'][i - 1], o['P_est'][i - 1])
        ref = es.filter_step(c, 'analytic', s_prev, P_prev, i)
        es._worst(worst, es.filter_diffs(c, es.filter_step(c, 'analytic', s_prev, P_prev, i,
                                                           _step_with_one_wrong_schur_entry), ref))
    assert max(worst[k] / (es.MARGIN * d[k]) for k in ('x', 'dx', 'ddx', 'P_est')) > 1.0, (worst, d)
