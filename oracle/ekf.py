"""Oracle: extended Kalman filter + Rauch-Tung-Striebel smoother of src/core/ekf.py.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

Restates `core.ekf.ekf` (src/core/ekf.py:26-347) as plain numpy, pinned by the reference's
own run on synthetic data (tests/golden/ekf_*.npz, tests/golden/make_golden.py):

* state s = [x (P), dx (P), ddx (P)]; constant-acceleration prediction (:73-79) whose
  result is cast to float32 (`.astype(np.float32)`, :79) — the reference's measurement
  model then runs on float32 pose values: FK trig in float32 (numpy float32 cos/sin of the
  float32 angles, matrices and sums in float64), and the forward-difference Jacobian (:81-96,
  eps = 1e-3) perturbs x_i in float32 (x_i + 1e-3 rounded to float32) while dividing by
  1e-3. This module reproduces those roundings;
* P0 (:159-186, including the reference's negative neck-length variance -0.28), Q from
  the qb list (:188-207), F (:219-224), R = diag((2 cov_c / min cov)^2) with cal_covs of
  :210-213 and max_pixel_err = cam_res[0] for points below the likelihood threshold
  (:244-253); residual = nan_to_num(z - h) (:256-257); K = P H^T S^-1 (:267),
  P = (I - K H) P (:274);
* initial state from linear fits of the pairwise-triangulated nose and lure (:121-157);
* RTS smoother (:280-287).
"""
import numpy as np
from scipy.stats import linregress

from .fisheye import project
from .kinematics import POSE, marker_positions

CAL_COVS = [0.137, 0.236, 0.176, 0.298, 0.087, 0.116]                      # src/core/ekf.py:210
QB = [5.0, 5.0, 5.0, 10.0, 10.0, 10.0, 5.0, 5.0, 25.0, 5.0, 50.0, 5.0, 50.0, 25.0, 100.0, 30.0, 140.0, 40.0,
      350.0, 200.0, 350.0, 200.0, 450.0, 400.0, 450.0, 400.0, 5.0, 5.0, 5.0]  # src/core/ekf.py:188-203
SIGMA_BOUND = 3


def n_angular(mode):
    return len([k for k in POSE[mode] if 'phi' in k or 'theta' in k or 'psi' in k])


def initial_covariance(mode):
    """P0 (src/core/ekf.py:159-186)."""
    na = n_angular(mode)
    p_lin_pos, p_ang_pos = np.ones(3) * 9.0, np.ones(na) * (np.pi / 4) ** 2
    p_lin_vel, p_ang_vel = np.ones(3) * 25.0, np.ones(na) * 9.0
    p_lin_acc, p_ang_acc = np.ones(3) * 9.0, np.ones(na) * 9.0
    p_ang_acc[10:] = 25.0
    if mode == 'default':
        d = np.concatenate([p_lin_pos, p_ang_pos[:3], [-0.28], p_ang_pos[3:], np.ones(3) * 9.0,
                            p_lin_vel, p_ang_vel[:3], [0.0], p_ang_vel[3:], np.ones(3) * 25.0,
                            p_lin_acc, p_ang_acc[:3], [0.0], p_ang_acc[3:], np.ones(3) * 9.0])
    elif mode == 'head':
        d = np.concatenate([p_lin_pos, p_ang_pos[:3], p_ang_pos[3:], p_lin_vel, p_ang_vel[:3], p_ang_vel[3:],
                            p_lin_acc, p_ang_acc[:3], p_ang_acc[3:]])
    else:
        raise ValueError(f'the reference EKF defines P0 for default / head only, not {mode!r}')
    return np.diag(d)


def process_noise(P, sT):
    qb = np.diag(QB[:P]) ** 2
    return np.block([[sT ** 4 / 4 * qb, sT ** 3 / 2 * qb, sT ** 2 / 2 * qb],
                     [sT ** 3 / 2 * qb, sT ** 2 * qb, sT * qb],
                     [sT ** 2 / 2 * qb, sT * qb, qb]])


def transition(P, sT):
    n = 3 * P
    F = np.eye(n)
    r = np.arange(n - P)
    F[r, r + P] = sT
    r2 = np.arange(n - 2 * P)
    F[r2, r2 + 2 * P] = sT ** 2 / 2
    return F


def predict(s, sT, P, ref_numerics=True):
    acc = s[2 * P:]
    vel = s[P:2 * P] + sT * acc
    pos = s[:P] + sT * vel + (0.5 * sT ** 2) * acc
    out = np.concatenate([pos, vel, acc])
    return out.astype(np.float32).astype(np.float64) if ref_numerics else out


def h_function(x, mode, K, D, R, t, ref_numerics=True):
    """(L, 2) pixels of the pose x (reference numerics: float32 values, FK trig in float32)."""
    x = np.asarray(x, np.float64)[None]
    pos = marker_positions(mode, x, f32_trig=ref_numerics)[0]
    return project(pos, K, D, R, t)


def fd_jacobian(x, mode, K, D, R, t, eps=1e-3, ref_numerics=True):
    """src/core/ekf.py:81-96; reference numerics perturb x_i in float32."""
    x = np.asarray(x, np.float64)
    fx = h_function(x, mode, K, D, R, t, ref_numerics).ravel()
    J = np.empty((fx.size, x.size))
    for i in range(x.size):
        xp = x.copy()
        xp[i] = float(np.float32(xp[i]) + np.float32(eps)) if ref_numerics else xp[i] + eps
        J[:, i] = (h_function(xp, mode, K, D, R, t, ref_numerics).ravel() - fx) / eps
    return fx, J


def initial_state(mode, frames, markers_idx, xyz, start_frame, sT):
    """src/core/ekf.py:121-157 from pairwise-triangulated points (frame, marker, xyz)."""
    idx = {k: i for i, k in enumerate(POSE[mode])}
    P = len(idx)
    s = np.zeros(3 * P)
    from acinoset_amd.kinematics import get_markers   # marker names (src/lib/misc.py:8-37)
    names = list(get_markers(mode))
    if 'lure' in names:
        sel = markers_idx == names.index('lure')
        if sel.sum() >= 2:
            sx, ix = linregress(frames[sel], xyz[sel, 0])[:2]
            sy, iy = linregress(frames[sel], xyz[sel, 1])[:2]
            s[[idx['x_l'], idx['y_l']]] = [start_frame * sx + ix, start_frame * sy + iy]
            s[[P + idx['x_l'], P + idx['y_l']]] = [sx / sT, sy / sT]
    sel = markers_idx == names.index('nose')
    sx, ix = linregress(frames[sel], xyz[sel, 0])[:2]
    sy, iy = linregress(frames[sel], xyz[sel, 1])[:2]
    s[[idx['x_0'], idx['y_0'], idx['psi_0']]] = [start_frame * sx + ix, start_frame * sy + iy, np.arctan2(sy, sx)]
    s[[P + idx['x_0'], P + idx['y_0']]] = [sx / sT, sy / sT]
    return s


def analytic_jacobian(x, mode, K, D, R, t):
    """The analytic measurement Jacobian (replacing :81-96): h(x) and
    H = d proj / d X (oracle.fisheye.project_jac) times d pos / d x (the exact FK Jacobian,
    oracle.kinematics.marker_jacobian), float64. Returns (h (2L,), H (2L, P))."""
    from .fisheye import project_jac
    from .kinematics import marker_jacobian
    x = np.asarray(x, np.float64)
    pos = marker_positions(mode, x[None])[0]                       # (L, 3)
    Jfk = marker_jacobian(mode, x[None])[0]                        # (L, 3, P)
    uv, Jp = project_jac(pos, K, D, R, t)                          # (L, 2), (L, 2, 3)
    return uv.ravel(), np.einsum('lik,lkp->lip', Jp, Jfk).reshape(-1, x.size)


def model_P(model):
    """Pose parameters of `model`: a mode name, or an object with `P`, `h(x, cam)` -> (2L,) pixels
    and `H(x, cam, jacobian)` -> (2L, P) (cam = (K, D, R, t) of one camera; float64 only)."""
    return len(POSE[model]) if isinstance(model, str) else int(model.P)


def measurement_model(model, x, cams, jacobian='fd', ref_numerics=True):
    """h (2 C L,) and H (2 C L, 3P; zero past the pose columns) of every camera at pose x."""
    K, D, R, t = cams
    C, P = len(K), model_P(model)
    rows = []
    for c in range(C):
        if not isinstance(model, str):
            assert not ref_numerics, 'a model object runs in float64'
            cam = (K[c], D[c], R[c], t[c])
            hc, Hc = np.asarray(model.h(x, cam)).ravel(), np.asarray(model.H(x, cam, jacobian))
        elif jacobian == 'analytic':
            hc, Hc = analytic_jacobian(x, model, K[c], D[c], R[c], t[c])
        else:
            hc, Hc = fd_jacobian(x, model, K[c], D[c], R[c], t[c], ref_numerics=ref_numerics)
        rows.append((hc, Hc))
    m = len(rows[0][0])
    H = np.zeros((C * m, 3 * P))
    h = np.zeros(C * m)
    for c, (hc, Hc) in enumerate(rows):
        h[c * m:(c + 1) * m], H[c * m:(c + 1) * m, :P] = hc, Hc
    return h, H


def measurement_std(base, lik_i, thresh, max_pixel_err):
    """Per-row measurement standard deviations of one frame (:244-253): `base` (2 C L,) with
    max_pixel_err on both rows of a point whose likelihood is below the threshold."""
    r_std = np.array(base, np.float64)
    r_std[np.repeat(np.asarray(lik_i).ravel() < thresh, 2)] = max_pixel_err
    return r_std


def _count_outliers(resid, S_diag):
    with np.errstate(invalid='ignore'):  # a negative diag(S) gives NaN: no outlier, as the reference
        tmp = SIGMA_BOUND * np.sqrt(S_diag)
    return int(np.sum((np.abs(resid[0::2]) > tmp[0::2]) | (np.abs(resid[1::2]) > tmp[1::2])))


def filter_step(model, cams, s_prev, P_prev, meas_i, lik_i, F, Q, sT, base, thresh=0.5, max_pixel_err=2704.0,
                ref_numerics=True, jacobian='fd'):
    """One frame of the filter in the reference's covariance form (:226-274): predict from
    (s_prev, P_prev), K = P H^T S^-1, P = (I - K H) P. cams = (K, D, R, t); meas_i (C, L, 2),
    lik_i (C, L); base (2 C L,) the per-row standard deviations before the likelihood
    threshold. Returns x_pred, P_pred, x_est, P_est, outliers."""
    P = model_P(model)
    n = 3 * P
    s = predict(np.asarray(s_prev, np.float64), sT, P, ref_numerics)
    Pm = F @ P_prev @ F.T + Q
    h, H = measurement_model(model, s[:P], cams, jacobian, ref_numerics)
    r_std = measurement_std(base, lik_i, thresh, max_pixel_err)
    Rm = np.diag(r_std ** 2)
    resid = np.nan_to_num(np.asarray(meas_i).reshape(-1) - h)
    S = H @ Pm @ H.T + Rm
    outliers = _count_outliers(resid, np.diag(S))
    Kg = Pm @ H.T @ np.linalg.inv(S)
    x_est = s + Kg @ resid
    P_est = (np.eye(n) - Kg @ H) @ Pm
    return s, Pm, x_est, P_est, outliers


def filter_step_information(model, cams, s_prev, P_prev, meas_i, lik_i, F, Q, sT, base, thresh=0.5,
                            max_pixel_err=2704.0, ref_numerics=True, jacobian='fd'):
    """The step of filter_step through A = Hx^T R^-1 Hx, b = Hx^T R^-1 r and (I + A P_xx)^-1
    (H^T S^-1 = (I + A P)^-1 H^T R^-1, H zero past the pose columns): x = s + P[:, x] V b,
    P_est = P - P[:, x] V A P[x, :], V = (I + A P_xx)^-1 by np.linalg.inv (as the covariance form
    inverts S). The same returns."""
    P = model_P(model)
    s = predict(np.asarray(s_prev, np.float64), sT, P, ref_numerics)
    Pm = F @ P_prev @ F.T + Q
    h, H = measurement_model(model, s[:P], cams, jacobian, ref_numerics)
    Hx = H[:, :P]
    r_std = measurement_std(base, lik_i, thresh, max_pixel_err)
    w = 1.0 / r_std ** 2
    resid = np.nan_to_num(np.asarray(meas_i).reshape(-1) - h)
    A = Hx.T @ (w[:, None] * Hx)
    b = Hx.T @ (w * resid)
    Pxx, Pcx = Pm[:P, :P], Pm[:, :P]
    outliers = _count_outliers(resid, np.einsum('ij,jk,ik->i', Hx, Pxx, Hx) + r_std ** 2)
    V = np.linalg.inv(np.eye(P) + A @ Pxx)
    x_est = s + Pcx @ (V @ b)
    P_est = Pm - Pcx @ (V @ A) @ Pm[:P, :]
    return s, Pm, x_est, P_est, outliers


def rts_step(x_est_i, P_est_i, x_pred_next, P_pred_next, xs_next, Ps_next, F):
    """One backward step of the RTS smoother (:280-287) with the gain by np.linalg.inv, as the
    reference. Ps_next None: the smoothed state only. Returns xs_i, Ps_i."""
    A = P_est_i @ F.T @ np.linalg.inv(P_pred_next)
    xs = x_est_i + A @ (xs_next - x_pred_next)
    Ps = None if Ps_next is None else P_est_i + A @ (Ps_next - P_pred_next) @ A.T
    return xs, Ps


def rts_step_solve(x_est_i, P_est_i, x_pred_next, P_pred_next, xs_next, Ps_next, F):
    """rts_step with the gain from a solve, A^T = P_pred^-T (F P_est^T), instead of an inverse."""
    A = np.linalg.solve(P_pred_next.T, F @ P_est_i.T).T
    xs = x_est_i + A @ (xs_next - x_pred_next)
    Ps = None if Ps_next is None else P_est_i + A @ (Ps_next - P_pred_next) @ A.T
    return xs, Ps


def measurement_std_base(n_cams, L, cal_covs=None):
    """(2 C L,) standard deviations 2 cov_c / min cov per row (:210-213)."""
    covs = CAL_COVS if cal_covs is None else list(cal_covs)
    assert n_cams == len(covs), (n_cams, len(covs))
    return np.repeat([2 * c / min(covs) for c in covs], 2 * L)


def ekf(meas, likelihood, K, D, R, t, mode, fps, s0, thresh=0.5, max_pixel_err=2704.0, ref_numerics=True,
        cal_covs=None, jacobian='fd', Q=None, P0=None):
    """meas (N, C, L, 2) pixels (NaN = missing), likelihood (N, C, L). Returns a dict with
    the filtered / predicted / smoothed states and covariances and the outlier count.
    `mode`: a mode name or a model object (model_P). `cal_covs`: per-camera calibration
    covariances (default: the reference's six, :210; the reference asserts six cameras, :213,
    other rigs pass their own). `jacobian`: 'fd' (the reference's forward differences) or
    'analytic' (float64 only). `Q`, `P0` (test extension): the process noise and initial
    covariance instead of the reference's (:154-208). filter_step and rts_step, chained."""
    assert jacobian == 'fd' or not ref_numerics, 'the analytic H runs in float64'
    N, C, L, _ = meas.shape
    P = model_P(mode)
    n = 3 * P
    sT = 1.0 / fps
    F = transition(P, sT)
    Q = process_noise(P, sT) if Q is None else np.asarray(Q, np.float64)
    Pm = initial_covariance(mode) if P0 is None else np.asarray(P0, np.float64)
    base = measurement_std_base(C, L, cal_covs)
    s = np.asarray(s0, np.float64)
    out = dict(x_est=np.zeros((N, n)), x_pred=np.zeros((N, n)), P_est=np.zeros((N, n, n)), P_pred=np.zeros((N, n, n)))
    outliers = 0
    for i in range(N):
        out['x_pred'][i], out['P_pred'][i], s, Pm, k = filter_step(
            mode, (K, D, R, t), s, Pm, meas[i], likelihood[i], F, Q, sT, base, thresh, max_pixel_err, ref_numerics,
            jacobian)
        out['x_est'][i], out['P_est'][i] = s, Pm
        outliers += k
    xs = out['x_est'].copy()
    Ps = out['P_est'].copy()
    for i in range(N - 2, -1, -1):
        xs[i], Ps[i] = rts_step(out['x_est'][i], out['P_est'][i], out['x_pred'][i + 1], out['P_pred'][i + 1],
                                xs[i + 1], Ps[i + 1], F)
    out.update(x_smooth=xs, P_smooth=Ps, outliers=outliers)
    return out
