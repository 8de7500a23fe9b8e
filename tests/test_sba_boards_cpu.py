"""The rigid-board bundle adjustment without a GPU: the numpy restatement (sba_boards_ref.py) against
central differences, the gauge count, scale recovery and scipy; the host-side initialisation; the
header and symbol table.

The scene of tests 2 to 4: 3 cameras on a 4 m ring, 5 boards of 4 x 3 corners, 0.1 m squares, every
board seen by every camera (sba_boards_ref.make_rig(3, 5, seed=0))."""
import os
import re

import numpy as np

import sba_boards_ref as ref
from acinoset_amd import _native
from acinoset_amd.lib import sba as lsba

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'acinoset_hip.h')


def _state(rig):
    return tuple(rig[k] for k in ('R', 't', 'K', 'D', 'obj', 'bR', 'bt'))


def test_jacobians_match_central_differences():
    rig = ref.make_rig(3, 4, seed=2, views=(1, 3))
    R, t, K, D, obj, bR, bt = _state(rig)
    mask, uv = rig['mask'], rig['uv']
    B, C = mask.shape
    J = ref.dense_jacobian(R, t, K, D, obj, bR, bt, mask)
    h = 1e-6
    Jn = np.zeros_like(J)
    for k in range(6 * C + 6 * B):
        r = []
        for s in (+h, -h):
            d = np.zeros(6 * C + 6 * B)
            d[k] = s
            Rn, tn = ref.apply(R, t, d[:6 * C].reshape(C, 6))
            bRn, btn = ref.apply(bR, bt, d[6 * C:].reshape(B, 6))
            r.append(ref.residuals(Rn, tn, K, D, obj, bRn, btn, uv, mask))
        Jn[:, k] = (r[0] - r[1]) / (2 * h)
    # central differences of step 1e-6 on entries up to ~1e4 px/rad: truncation ~h^2 |J'''| and
    # rounding ~1e-16 |r| / h, both below 1e-6 of the largest entry
    assert np.abs(J - Jn).max() <= 1e-6 * np.abs(J).max()
    assert np.abs(J[:, :6 * C]).max() > 1.0 and np.abs(J[:, 6 * C:]).max() > 1.0


def test_gauge_is_six_dimensional_where_free_corners_have_seven():
    """Measured: the six smallest eigenvalues of J^T J at most 1.0e-16 of the largest, the seventh
    8.5e-6 of it; free corners: seven at most 2.0e-16, the eighth 5.4e-6."""
    rig = ref.make_rig(3, 5, seed=0)
    R, t, K, D, obj, bR, bt = _state(rig)
    J = ref.dense_jacobian(R, t, K, D, obj, bR, bt, rig['mask'])
    w = np.linalg.eigvalsh(J.T @ J)
    assert np.all(np.abs(w[:6]) < 1e-12 * w[-1])
    assert w[6] > 1e-6 * w[-1]
    Jf = ref.free_corner_jacobian(R, t, K, D, obj, bR, bt, rig['mask'])
    wf = np.linalg.eigvalsh(Jf.T @ Jf)
    assert np.all(np.abs(wf[:7]) < 1e-12 * wf[-1])
    assert wf[7] > 1e-12 * wf[-1]


def test_scale_recovered_from_a_scaled_start():
    """Noiseless data, every camera and board translation of the start multiplied by 1.05: the solve
    returns every pairwise camera-centre distance. Measured: 3.3e-16 relative (18 iterations, xtol)."""
    rig = ref.make_rig(3, 5, seed=0)
    R, t, K, D, obj, bR, bt = _state(rig)
    truth = ref.centre_distances(R, t)
    assert np.abs(ref.centre_distances(R, 1.05 * t) / truth - 1).min() > 0.049
    Rs, ts, _, _, info = ref.sba_boards(R, 1.05 * t, K, D, obj, bR, 1.05 * bt, rig['uv'], rig['mask'])
    err = np.abs(ref.centre_distances(Rs, ts) / truth - 1).max()
    print('scale recovery: max relative baseline error', err, info)
    assert err <= 1e-6


def test_matches_scipy_on_noisy_data():
    """0.5 px noise, a perturbed start; scipy TRF with the Cauchy loss at tolerances 1e-15 over the same
    6 C + 6 B perturbation parameters (3-point differences). Measured, helper against scipy: final
    cost -1.35e-13 (the helper's is lower; 32.4533142191985 against ...9859) and 9.4e-10 m on the
    pairwise camera-centre distances; asserted at ten times those."""
    from scipy.optimize import least_squares
    rig = ref.make_rig(3, 5, seed=0, noise=0.5)
    K, D, obj, mask, uv = (rig[k] for k in ('K', 'D', 'obj', 'mask', 'uv'))
    R0, t0, bR0, bt0 = ref.perturb(rig, 7)
    B, C = mask.shape

    def unpack(x):
        return ref.apply(R0, t0, x[:6 * C].reshape(C, 6)) + ref.apply(bR0, bt0, x[6 * C:].reshape(B, 6))

    def fun(x):
        R, t, bR, bt = unpack(x)
        return ref.residuals(R, t, K, D, obj, bR, bt, uv, mask)

    s = least_squares(fun, np.zeros(6 * C + 6 * B), jac='3-point', method='trf', loss='cauchy', x_scale='jac',
                      ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=2000)
    Rh, th, _, _, info = ref.sba_boards(R0, t0, K, D, obj, bR0, bt0, uv, mask)
    Rs, ts, _, _ = unpack(s.x)
    dd = np.abs(ref.centre_distances(Rh, th) - ref.centre_distances(Rs, ts)).max()
    print('helper - scipy: cost', info['cost_after'] - s.cost, 'distances', dd, info)
    assert info['cost_after'] < 0.2 * info['cost_before']
    assert info['cost_after'] <= s.cost + 1.4e-12
    assert dd <= 9.4e-9


def test_board_poses_from_points():
    rng = np.random.default_rng(3)
    obj = ref.board_object_pts((4, 3), 0.1)
    bR = np.array([ref.rodrigues(rng.normal(0, 1.5, 3)) for _ in range(6)])
    bt = rng.normal(0, 2.0, (6, 3))
    X = np.einsum('bij,nj->bni', bR, obj) + bt[:, None, :]
    r, t = lsba.board_poses_from_points(obj, X)
    np.testing.assert_allclose(r, bR, atol=1e-12)
    np.testing.assert_allclose(t, bt, atol=1e-12)
    # a mirrored point set has no rigid fit: the answer is still a proper rotation
    r, t = lsba.board_poses_from_points(obj, X * [1.0, 1.0, -1.0])
    np.testing.assert_allclose(np.linalg.det(r), 1.0, atol=1e-12)
    np.testing.assert_allclose(r @ np.swapaxes(r, 1, 2), np.broadcast_to(np.eye(3), r.shape), atol=1e-12)
    r1, t1 = lsba.board_poses_from_points(obj, X[0])
    np.testing.assert_array_equal(r1[0], lsba.board_poses_from_points(obj, X)[0][0])


def test_header_and_symbols():
    with open(HEADER) as f:
        text = f.read()
    assert re.search(r'^#define ACS_ABI_VERSION 5$', text, re.M)
    assert _native.ABI_VERSION == 5
    m = re.search(r'int acs_sba_boards\(([^;]*)\);', text)
    assert m, 'acs_sba_boards prototype missing from include/acinoset_hip.h'
    args = [a.strip() for a in m.group(1).replace('\n', ' ').split(',')]
    assert [a.split()[-1].lstrip('*') for a in args] == [
        'ctx', 'cams', 'n_cams', 'obj_pts', 'n_corners', 'uv', 'mask', 'n_boards', 'board_poses', 'opts',
        'resid_before', 'resid_after', 'report', 'flags']
    assert 'const acs_sba_ext_opts* opts' in m.group(1) and 'acs_sba_ext_report* report' in m.group(1)
    assert 'acs_sba_boards' in _native.SYMBOLS
    assert hasattr(_native.Context, 'sba_boards')
