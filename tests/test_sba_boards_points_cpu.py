"""The rigid-board bundle adjustment with free points without a GPU: the numpy restatement
(sba_boards_points_ref.py) against central differences and a dense solve, against sba_boards_ref with no
points, on the split rig the feature exists for, against scipy; the rule that picks the GPU parity
problems; the header and the binding. Every measured quantity is in DESIGN §3 "Rigid-board SBA with
free points" and asserted at ten times the measured value."""
import os
import re

import numpy as np

import sba_boards_points_ref as ref
import sba_boards_ref as bref
import sba_ext_shapes as sh
from acinoset_amd import _native

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'acinoset_hip.h')


def _apply(start, x, C, B):
    R0, t0, bR0, bt0, X0 = start
    return (bref.apply(R0, t0, x[:6 * C].reshape(C, 6)) + bref.apply(bR0, bt0, x[6 * C:6 * C + 6 * B].reshape(B, 6))
            + (X0 + x[6 * C + 6 * B:].reshape(-1, 3),))


def _resid(rig, state):
    R, t, bR, bt, X = state
    return ref.residuals(R, t, rig['K'], rig['D'], rig['obj'], bR, bt, rig['uv'], rig['mask'], X, rig['pt_uv'],
                         rig['pt_mask'])


def _jac(rig, state):
    R, t, bR, bt, X = state
    return ref.dense_jacobian(R, t, rig['K'], rig['D'], rig['obj'], bR, bt, rig['mask'], X, rig['pt_mask'])


def test_schur_step_equals_the_dense_step():
    """(J^T W J + lam diag) d = -J^T w r over all 6 C + 6 B + 3 n parameters, the dense Jacobian checked
    against central differences, against the step of the Schur complement. Measured at lam = 1e-3
    on the (3, 5, (4, 3)) rig with 7 points seen by 2-3 cameras: relative difference 3.7e-13 of the
    largest entry of the step."""
    rig, start = ref.problem('c3_b5_nc12_n7')
    C, B, n = 3, 5, 7
    N = 6 * C + 6 * B + 3 * n
    J = _jac(rig, start)
    h = 1e-6
    Jn = np.zeros_like(J)
    for k in range(N):
        d = np.zeros(N)
        d[k] = h
        Jn[:, k] = (_resid(rig, _apply(start, d, C, B)) - _resid(rig, _apply(start, -d, C, B))) / (2 * h)
    # central differences of step 1e-6 (as test_sba_boards_cpu.py): below 1e-6 of the largest entry
    assert np.abs(J - Jn).max() <= 1e-6 * np.abs(J).max()
    assert np.abs(J[:, 6 * C + 6 * B:]).max() > 1.0 and J.shape == (2 * (12 * 15 + int(rig['pt_mask'].sum())), N)
    r = _resid(rig, start)
    z = r * r
    w = 1.0 / (1.0 + z)
    wh = np.maximum((1.0 - z) * w * w, 0.1 * w)
    H = J.T @ (wh[:, None] * J)
    g = J.T @ (w * r)
    lam = 1e-3
    dg = np.diag(H).copy()
    dg[:6 * C] = np.maximum(dg[:6 * C], 1e-12)  # the camera diagonal's floor (k_ext_solve)
    Hd = H + lam * np.diag(dg) + 1e-300 * np.diag(np.arange(N) >= 6 * C)
    dense = np.linalg.solve(Hd, -g)
    R0, t0, bR0, bt0, X0 = start
    lin = ref.linearize(R0, t0, rig['K'], rig['D'], rig['obj'], bR0, bt0, rig['uv'], rig['mask'], X0, rig['pt_uv'],
                        rig['pt_mask'], 1.0)
    dc, db, dX = ref.step(*lin[1:], rig['mask'] != 0, rig['pt_mask'], lam)
    schur = np.concatenate([dc.ravel(), db.ravel(), dX.ravel()])
    rel = np.abs(schur - dense).max() / np.abs(dense).max()
    print('Schur step against the dense step: relative difference %.3e' % rel)
    assert rel <= 3.7e-12


def test_no_points_is_the_boards_helper_exactly():
    rig = bref.make_rig(3, 5, seed=0, noise=0.5)
    R0, t0, bR0, bt0 = bref.perturb(rig, 100)
    K, D, obj, uv, mask = (rig[k] for k in ('K', 'D', 'obj', 'uv', 'mask'))
    for kw in (dict(max_iters=8), dict(ftol=1e-10)):
        a = bref.sba_boards(R0, t0, K, D, obj, bR0, bt0, uv, mask, **kw)
        b = ref.sba_boards_points(R0, t0, K, D, obj, bR0, bt0, uv, mask, np.zeros((0, 3)), np.zeros((0, 3, 2)),
                                  np.zeros((0, 3), np.uint8), **kw)
        for x, y in zip(a[:4], b[:4]):
            np.testing.assert_array_equal(x.view(np.uint64), y.view(np.uint64))
        assert b[4].shape == (0, 3) and a[4] == b[5]


def _spectrum(rig, with_points):
    R, t, bR, bt, X = (rig[k] for k in ('R', 't', 'bR', 'bt', 'X'))
    if with_points:
        J = ref.dense_jacobian(R, t, rig['K'], rig['D'], rig['obj'], bR, bt, rig['mask'], X, rig['pt_mask'])
    else:
        J = bref.dense_jacobian(R, t, rig['K'], rig['D'], rig['obj'], bR, bt, rig['mask'])
    return np.linalg.eigvalsh(J.T @ J)


def test_split_rig_is_tied_together_by_the_points():
    """4 ring cameras; boards 0-2 seen only by cameras {0, 1}, boards 3-5 only by {2, 3}; (4, 3) corners,
    0.5 px noise; 6 non-coplanar points seen by all four cameras.
    J^T J at the truth. Boards alone: 12 eigenvalues at rounding level (measured: the 12 smallest at
    most 8.9e-17 of the largest, the 13th 1.64e-6 of it). With the points: 6 (at most 1.04e-16), the 7th
    2.12e-6 of the largest.
    The start: perturb()'s, and cameras {2, 3} moved together by 2 cm and 5 mrad. Measured, largest error
    of the four cross-group centre distances: 1.77e-2 m at the start; boards alone 3.43e-2 m after the
    solve (the displacement stays, and each group drifts along its own free gauge); with the points
    1.50e-2 m. That is the noise level of this rig: sigma^2 pinv(J^T J) at 0.5 px propagated to the four
    distances gives standard deviations of 1.16e-2 to 1.31e-2 m (six points in a 1.6 m box seen from
    4 to 5 m tie the two pairs no tighter). Asserted: boards alone above a tenth of its measured value,
    mixed below ten times its measured value.
    Without noise the same start separates the two cleanly, so that is asserted too. Measured: boards
    alone 2.26e-2 m at a cost of 9e-23 (the data cannot see the displacement), asserted above a tenth of
    it; with the points 1.3e-13 m, asserted below 1e-9 m (the translation tolerance of the GPU parity
    tests: an exact fit has no noise floor, what is left is rounding)."""
    rig = ref.split_rig()
    wb, wp = _spectrum(rig, False), _spectrum(rig, True)
    print('boards alone: 12 smallest <= %.2e, 13th %.2e of the largest' % (np.abs(wb[:12]).max() / wb[-1], wb[12] / wb[-1]))
    print('with points:   6 smallest <= %.2e,  7th %.2e of the largest' % (np.abs(wp[:6]).max() / wp[-1], wp[6] / wp[-1]))
    assert np.all(np.abs(wb[:12]) < 1e-12 * wb[-1]) and wb[12] > 1e-7 * wb[-1]
    assert np.all(np.abs(wp[:6]) < 1e-12 * wp[-1]) and wp[6] > 1e-8 * wp[-1]
    start = ref.split_start(rig)
    truth = ref.cross_distances(rig['R'], rig['t'])
    e0 = np.abs(ref.cross_distances(start[0], start[1]) - truth).max()
    K, D, obj, uv, mask = (rig[k] for k in ('K', 'D', 'obj', 'uv', 'mask'))
    Rb, tb, _, _, ib = bref.sba_boards(*start[:2], K, D, obj, *start[2:4], uv, mask)
    eb = np.abs(ref.cross_distances(Rb, tb) - truth).max()
    Rm, tm, _, _, _, im = ref.solve(rig, start)
    em = np.abs(ref.cross_distances(Rm, tm) - truth).max()
    print('cross-group centre distances, largest error: start %.3e, boards alone %.3e, with points %.3e m' % (e0, eb, em))
    print(ib, im)
    assert eb >= 3.43e-3
    assert em <= 1.50e-1
    rig0 = ref.split_rig(noise=0.0)
    start0 = ref.split_start(rig0)
    Rb, tb = bref.sba_boards(*start0[:2], K, D, obj, *start0[2:4], rig0['uv'], mask)[:2]
    Rm, tm = ref.solve(rig0, start0)[:2]
    eb0, em0 = (np.abs(ref.cross_distances(a, b) - truth).max() for a, b in ((Rb, tb), (Rm, tm)))
    print('without noise: boards alone %.3e, with points %.3e m' % (eb0, em0))
    assert eb0 >= 2.26e-3
    assert em0 <= 1e-9


def test_matches_scipy_on_noisy_data():
    """The (3, 5, (4, 3)) rig with 7 points, 0.5 px noise, a perturbed start; scipy TRF with the Cauchy
    loss at tolerances 1e-15 over the same 6 C + 6 B + 3 n parameters (3-point differences). Measured,
    helper against scipy: final cost +9.7e-13 (33.10446522809664 against ...09567; the same with
    scipy's state put through the helper's cost function) and 9.7e-11 m on the pairwise camera-centre
    distances; the distances asserted at ten times that. "Not higher" is read at the helper's own stop:
    it ends on a relative decrease of ftol = 1e-12 or less, so it may stand ftol F = 3.3e-11 above the
    minimum that scipy, run to 1e-15, reaches."""
    from scipy.optimize import least_squares
    rig, start = ref.problem('c3_b5_nc12_n7')
    C, B = 3, 5

    def fun(x):
        return _resid(rig, _apply(start, x, C, B))

    s = least_squares(fun, np.zeros(6 * C + 6 * B + 21), jac='3-point', method='trf', loss='cauchy', x_scale='jac',
                      ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=2000)
    Rh, th, _, _, _, info = ref.solve(rig, start)
    Rs, ts = _apply(start, s.x, C, B)[:2]
    dd = np.abs(bref.centre_distances(Rh, th) - bref.centre_distances(Rs, ts)).max()
    print('helper - scipy: cost %.3e, distances %.3e' % (info['cost_after'] - s.cost, dd), info)
    assert info['cost_after'] < 0.2 * info['cost_before']
    assert info['status'] == 'ftol' and info['cost_after'] <= s.cost + 1e-12 * s.cost
    assert dd <= 9.7e-10


# ---- the condition for every fixed-iteration GPU parity problem ----------------------------------
def test_every_compared_decision_is_far_from_a_tie():
    for name in ref.PROBLEMS:
        trace = []
        ref.solve(*ref.problem(name), trace=trace, max_iters=ref.FIXED_ITERS)
        m = min(sh.margin(e) for e in trace)
        print(name, 'smallest margin %.2e over %d decisions' % (m, len(trace)))
        assert len(trace) == ref.FIXED_ITERS and m >= sh.TIE, name
    trace = []
    ref.solve(ref.split_rig(), ref.split_start(ref.split_rig()), trace=trace, max_iters=ref.FIXED_ITERS)
    assert min(sh.margin(e) for e in trace) >= sh.TIE


def test_the_stop_of_the_run_to_convergence():
    """The run to convergence on the C = 3 rig stops on ftol; the tolerance is choose_stop's on the trace
    of a run without tolerances (ref.CONVERGED records it)."""
    trace = []
    ref.solve(*ref.problem('c3_b5_nc12_n7'), trace=trace, **dict(sh.FREE, max_iters=ref.FREE_ITERS))
    stop = sh.choose_stop(trace, 'ftol')
    print(stop)
    assert stop is not None
    assert abs(stop.tol / ref.CONVERGED.tol - 1) < 5e-3 and stop.iters == ref.CONVERGED.iters
    assert all(sh.margin(e) >= sh.TIE for e in trace[:stop.iters - 1])


def test_header_and_binding():
    with open(HEADER) as f:
        text = f.read()
    assert re.search(r'^#define ACS_ABI_VERSION 5$', text, re.M)
    assert _native.ABI_VERSION == 5
    m = re.search(r'int acs_sba_boards_points\(([^;]*)\);', text)
    assert m, 'acs_sba_boards_points prototype missing from include/acinoset_hip.h'
    args = [a.strip() for a in m.group(1).replace('\n', ' ').split(',')]
    assert [a.split()[-1].lstrip('*') for a in args] == [
        'ctx', 'cams', 'n_cams', 'obj_pts', 'n_corners', 'uv', 'mask', 'n_boards', 'board_poses', 'pt_uv', 'pt_mask',
        'n_pts', 'pts', 'opts', 'resid_before', 'resid_after', 'report', 'flags']
    assert 'const acs_sba_ext_opts* opts' in m.group(1) and 'acs_sba_ext_report* report' in m.group(1)
    assert 'acs_sba_boards_points' in _native.SYMBOLS
    assert hasattr(_native.Context, 'sba_boards_points') and hasattr(_native.Context, 'sba_boards_points_dev')
    # acs_sba_boards keeps its prototype
    assert re.search(r'int acs_sba_boards\(acs_ctx\* ctx, double\* cams, int32_t n_cams, const double\* obj_pts,', text)
