"""GPU: the EKF + RTS smoother (acs_ekf_run) frame by frame, at every state size its kernels
select on: head 6, neck10 10, upper_body 11, head_stabilize 11, front18 18, default_nolure 26,
default 29 (tests/ekf_sizes.py; tests/test_ekf_plan.py shows these cases launch every filter,
gain and smoother instance of csrc/ekf.hip). 12-camera ring, 8 frames, float64 forward-difference
and analytic H.

Nothing is compared along a trajectory. Frame i's x_pred, x_est and P_est are compared with
oracle.ekf.filter_step started from the GPU's own x_est[i-1], P_est[i-1] (frame 0: s0, P0);
x_smooth[i] and P_smooth[i] with oracle.ekf.rts_step fed the GPU's own filter output, its own
x_smooth[i+1], P_smooth[i+1] and P_pred = F P_est F^T + Q; the x_smooth of the run without
covariances (the parallel gains and the state recursion) the same way. The tolerance of a
quantity q is MARGIN (100) x d_q, d_q from the oracle alone (the rule of tests/ekf_sizes.py).
Vectors absolutely, matrices relative to their largest entry.

MEASURED (MI355X; this module's `-s` output, lines `EKF_SIZES ...`, kept whole in
profiles/r19/ekf_sizes_gpu.log and as a table in DESIGN.md's EKF section, round 19). Worst frame
of the clip, measured / d_q; "par." is the x_smooth of the run without covariances:

  case            H         x            dx           ddx          P_est        x_smooth     P_smooth     par.
  head            fd        2e-12/4e-12  2e-11/2e-11  4e-11/3e-11  4e-12/6e-12  1e-14/3e-12  1e-13/4e-14  2e-11/3e-12
  head            analytic  7e-12/7e-12  1e-12/1e-12  3e-13/3e-12  3e-12/4e-12  4e-14/3e-12  7e-14/9e-14  2e-11/3e-12
  neck10          fd        6e-11/5e-11  1e-10/1e-10  8e-10/3e-10  1e-12/3e-12  2e-13/3e-12  3e-14/3e-14  2e-13/3e-12
  neck10          analytic  4e-12/4e-12  5e-13/5e-13  3e-13/2e-12  8e-13/9e-13  2e-13/3e-12  5e-14/6e-14  2e-13/3e-12
  upper_body      fd        5e-12/2e-11  4e-11/2e-10  3e-10/6e-10  3e-13/4e-13  2e-12/4e-12  1e-13/1e-13  2e-12/4e-12
  upper_body      analytic  1e-11/1e-11  7e-12/9e-12  7e-13/3e-12  2e-13/6e-13  1e-12/4e-12  7e-14/1e-13  1e-12/4e-12
  head_stabilize  fd        3e-11/6e-11  1e-10/2e-10  1e-9/5e-9    8e-13/1e-12  2e-12/3e-12  6e-14/7e-14  2e-12/3e-12
  head_stabilize  analytic  5e-12/1e-11  1e-12/2e-12  8e-13/4e-12  2e-13/4e-13  3e-12/3e-12  4e-14/1e-13  3e-12/3e-12
  front18         fd        2e-11/2e-11  2e-10/1e-10  3e-9/2e-9    4e-13/8e-13  1e-11/4e-11  2e-13/3e-13  1e-11/4e-11
  front18         analytic  2e-11/3e-11  8e-12/8e-12  1e-11/1e-11  9e-14/3e-13  2e-11/1e-10  1e-13/3e-13  2e-11/1e-10
  default_nolure  fd        3e-11/2e-11  1e-10/7e-11  4e-9/3e-9    1e-12/7e-13  1e-10/3e-9   2e-12/2e-12  1e-10/3e-9
  default_nolure  analytic  9e-12/3e-11  2e-12/3e-12  1e-10/1e-10  3e-14/3e-14  2e-10/1e-9   5e-13/1e-12  2e-10/1e-9
  default         fd        2e-11/2e-11  3e-10/3e-10  9e-9/8e-9    8e-13/8e-13  1e-10/2e-9   1e-12/1e-12  1e-10/2e-9
  default         analytic  2e-11/3e-11  3e-12/5e-12  1e-10/1e-10  2e-14/2e-14  1e-10/1e-9   1e-12/2e-12  1e-10/1e-9

The predicted states differ by at most 2e-15 (d_q 9e-16 .. 1e-13). The worst measured / d_q of any
quantity in any case of this module (the Q[5,5] = -1 and the 1- and 2-frame clips included, whose
rows are in DESIGN.md) is 7.2, the head model's parallel-gain x_smooth; the margin is 100. The
outlier counts are equal in every case.
"""
import numpy as np
import pytest

import ekf_sizes as es
from acinoset_amd import _native
from oracle import ekf as oekf

pytestmark = pytest.mark.gpu

FILTER_KEYS = ('xp', 'dxp', 'ddxp', 'x', 'dx', 'ddx', 'P_est')
INDEFINITE = ('neck10', 'upper_body', 'front18', 'default_nolure')


def _run(ctx, c, jacobian, covariances, meas=None, lik=None, s0=None):
    cams = _native.pack_cameras(*c.cams)
    return ctx.ekf_run(c.table, cams, c.meas if meas is None else meas, c.lik if lik is None else lik, es.FPS, 0.5,
                       c.max_pixel_err, c.rstd, c.Q, c.P0, c.s0 if s0 is None else s0, ref_numerics=False,
                       covariances=covariances, jacobian=jacobian)


def _measure_steps(c, jacobian, a, b):
    """Worst per-frame differences of the run without (a) and with (b) covariances from the
    oracle steps on the GPU's own previous values, and the oracle's outlier count."""
    N = len(b['x_est'])
    got = dict.fromkeys(FILTER_KEYS + ('x_smooth', 'P_smooth', 'xs_only'), 0.0)
    outliers = 0
    for i in range(N):
        s_prev, P_prev = (c.s0, c.P0) if i == 0 else (b['x_est'][i - 1], b['P_est'][i - 1])
        ref = es.filter_step(c, jacobian, s_prev, P_prev, i)
        es._worst(got, es.filter_diffs(c, (b['x_pred'][i], None, b['x_est'][i], b['P_est'][i]), ref))
        outliers += ref[4]
    for i in range(N - 2, -1, -1):
        Pp = c.F @ b['P_est'][i] @ c.F.T + c.Q
        xs, Ps = oekf.rts_step(b['x_est'][i], b['P_est'][i], b['x_pred'][i + 1], Pp, b['x_smooth'][i + 1],
                               b['P_smooth'][i + 1], c.F)
        xo, _ = oekf.rts_step(b['x_est'][i], b['P_est'][i], b['x_pred'][i + 1], Pp, a['x_smooth'][i + 1], None, c.F)
        es._worst(got, {'x_smooth': float(np.abs(b['x_smooth'][i] - xs).max()),
                        'P_smooth': es.mat_diff(b['P_smooth'][i], Ps),
                        'xs_only': float(np.abs(a['x_smooth'][i] - xo).max())})
    return got, outliers


def _check_steps(label, c, jacobian, a, b, d):
    """The step checks of the module docstring; prints every figure before it asserts."""
    np.testing.assert_array_equal(a['x_est'], b['x_est'])
    np.testing.assert_array_equal(a['x_pred'], b['x_pred'])
    np.testing.assert_array_equal(a['x_smooth'][-1], a['x_est'][-1])
    np.testing.assert_array_equal(b['x_smooth'][-1], b['x_est'][-1])
    np.testing.assert_array_equal(b['P_smooth'][-1], b['P_est'][-1])
    for out in (a, b):
        assert all(np.isfinite(v).all() for v in out.values())
    got, outliers = _measure_steps(c, jacobian, a, b)
    d = dict(d, xs_only=d['x_smooth'])
    for k, v in got.items():
        print(f'EKF_SIZES {label} {jacobian} {k} measured {v:.2e} d_q {d[k]:.2e} ratio {v / d[k] if d[k] else 0:.2f}')
    print(f'EKF_SIZES {label} {jacobian} outliers gpu {int(a["outliers"])} oracle {outliers}')
    bad = {k: (v, d[k]) for k, v in got.items() if not v <= es.MARGIN * d[k]}
    assert not bad, bad
    assert abs(int(a['outliers']) - outliers) <= 1 and int(a['outliers']) == int(b['outliers'])


@pytest.mark.parametrize('jacobian', ['fd', 'analytic'])
@pytest.mark.parametrize('name', es.SIZES)
def test_ekf_every_size_matches_the_oracle_step_by_step(ctx, name, jacobian):
    c = es.case(name)
    a, b = _run(ctx, c, jacobian, False), _run(ctx, c, jacobian, True)
    _check_steps(name, c, jacobian, a, b, es.bounds(name, jacobian))


@pytest.mark.parametrize('name', ['neck10', 'front18'])
def test_truncated_tables_fk_matches_the_embedded_oracle(ctx, name):
    """The tables kinematics.table_from_tree builds for the two test skeletons, run by the FK
    kernel, against default_nolure's oracle at the embedded pose (which never sees a table)."""
    c = es.case(name)
    x = c.s0[:c.P] + np.random.default_rng(8).normal(0, 0.3, (5, c.P))
    assert np.abs(ctx.fk(c.table, x) - c.model.positions(x)).max() < 1e-12


@pytest.mark.parametrize('name', ['upper_body', 'default_nolure'])
def test_ekf_batch_of_three_equals_single_runs(ctx, name):
    """The gain grids and the per-gain flag array are indexed by (sequence, frame): three
    different sequences in one call equal the three single calls bit for bit, with and without
    the smoothed covariances."""
    c = es.case(name)
    rng = np.random.default_rng(3)
    meas = np.stack([c.meas + 0.5 * k * rng.normal(0, 1, c.meas.shape) for k in range(3)])
    lik = np.stack([c.lik] * 3)
    s0 = np.stack([c.s0, c.s0 * 1.001, c.s0 + 0.002])
    for cov in (False, True):
        batch = _run(ctx, c, 'analytic', cov, meas, lik, s0)
        assert not np.array_equal(batch['x_est'][0], batch['x_est'][1])
        for k in range(3):
            one = _run(ctx, c, 'analytic', cov, meas[k], lik[k], s0[k])
            for key in one:
                np.testing.assert_array_equal(batch[key][k], one[key], err_msg=f'{key} of sequence {k}')


@pytest.mark.parametrize('name', INDEFINITE)
def test_ekf_pivoted_gains_away_from_87_states(ctx, name):
    """Q[5,5] = -1: every P_pred a gain inverts has a negative eigenvalue (the oracle's own run,
    tests/test_ekf_sizes_cpu.py), so k_ekf_gain_t flags every gain to k_ekf_gain_piv (neck10:
    k_ekf_gain, the unpivoted blocked Gauss-Jordan of the sequential smoother, which takes any
    non-zero pivot). Two sequences. The parallel path against the sequential smoother at
    1e-9 x scale, everything finite, sequence 0 step by step against the oracle (np.linalg.inv:
    pivoted LU) at the rule's tolerance for this clip, sequence 1 equal to its single run."""
    c = es.case(name, es.N_FRAMES, True)
    s0 = np.stack([c.s0, c.s0 + 0.002])
    meas = np.stack([c.meas, c.meas + 0.25])
    lik = np.stack([c.lik] * 2)
    a = _run(ctx, c, 'analytic', False, meas, lik, s0)
    b = _run(ctx, c, 'analytic', True, meas, lik, s0)
    np.testing.assert_array_equal(a['x_est'], b['x_est'])
    assert all(np.isfinite(v).all() for out in (a, b) for v in out.values())
    sc = max(1.0, float(np.abs(b['x_smooth']).max()))
    print(f'EKF_SIZES {name}-indefinite parallel-vs-sequential {np.abs(a["x_smooth"] - b["x_smooth"]).max() / sc:.2e}')
    np.testing.assert_allclose(a['x_smooth'], b['x_smooth'], atol=1e-9 * sc, rtol=0)
    _check_steps(name + '-indefinite', c, 'analytic', {k: v[0] for k, v in a.items()}, {k: v[0] for k, v in b.items()},
                 es.bounds(name, 'analytic', es.N_FRAMES, True))
    one = _run(ctx, c, 'analytic', False, meas[1], lik[1], s0[1])
    for key in one:
        np.testing.assert_array_equal(a[key][1], one[key], err_msg=key)


@pytest.mark.parametrize('N', [1, 2])
@pytest.mark.parametrize('name', INDEFINITE)
def test_ekf_shortest_clips_every_size(ctx, name, N):
    """One frame (no gain) and two frames (one gain), with and without covariances, by the same
    step checks; the last smoothed state is the last filtered one."""
    c = es.case(name, N)
    a, b = _run(ctx, c, 'analytic', False), _run(ctx, c, 'analytic', True)
    assert a['x_est'].shape == (N, c.n) and b['P_smooth'].shape == (N, c.n, c.n)
    _check_steps(f'{name}-N{N}', c, 'analytic', a, b, es.bounds(name, 'analytic', N))
