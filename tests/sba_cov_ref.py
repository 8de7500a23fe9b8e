"""CPU reference of the points-only SBA's per-point covariance for the tests: a numpy
restatement of the definition in DESIGN §3 / include/acinoset_hip.h (not a conftest).

For point i with observations o, residuals r_od (pixels) at the points passed in,
z = r^2 / f_scale^2 and w = 1 / (1 + z):

    H_i   = sum_o sum_d wh_od J_od^T J_od,  wh = max((1 - z) w^2, 0.1 w)   (oracle/sba.py:90)
    cov_i = sigma_px^2 H_i^-1, by LDL^T without pivoting (pivots d0, d1, d2)
    status: NOOBS (1) without observations, else DEGENERATE (2) when a pivot fails
            d > 1e-9 max(H00, H11, H22) (a NaN fails), else OK (0); cov is NaN unless OK
    sigma_hat^2 = sum w r^2 / (m - 3 n_ok) over the observations of the OK points, m their number
            of scalar residuals; NaN when m <= 3 n_ok

`project_jac(X, K, D, R, t) -> (uv (n, 2), J (n, 2, 3))` is `oracle.fisheye.project_jac` or
`tests/standard_model.project_jac`, with per-observation camera parameters.
"""
import numpy as np

OK, NOOBS, DEGENERATE = 0, 1, 2
PIVOT_RATIO = 1e-9


def normal_matrices(project_jac, uv, pt_idx, cam_idx, pts, K, D, R, t, f_scale=50.0):
    """-> H (n, 3, 3), sum w r^2 (n,), number of scalar residuals (n,)."""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    n = len(pts)
    pi = np.asarray(pt_idx, np.int64)
    ci = np.asarray(cam_idx, np.int64)
    H = np.zeros((n, 3, 3))
    swr2 = np.zeros(n)
    m = np.zeros(n, np.int64)
    if len(pi) == 0:
        return H, swr2, m
    with np.errstate(invalid='ignore', divide='ignore'):
        prj, J = project_jac(pts[pi], K[ci], D[ci], R[ci], t[ci])
        r = prj - np.asarray(uv, np.float64).reshape(-1, 2)
        z = r * r / (f_scale * f_scale)
        w = 1.0 / (1.0 + z)
        wh = np.maximum((1.0 - z) * w * w, 0.1 * w)     # propagates a NaN
        np.add.at(H, pi, np.einsum('od,odi,odj->oij', wh, J, J))
        np.add.at(swr2, pi, (w * r * r).sum(1))
    np.add.at(m, pi, 2)
    return H, swr2, m


def ldl_inverse(H):
    """(n, 3, 3) symmetric -> (inverse (n, 3, 3) by LDL^T without pivoting, pivots (n, 3))."""
    H = np.asarray(H, np.float64).reshape(-1, 3, 3)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        d0 = H[:, 0, 0]
        l10, l20 = H[:, 0, 1] / d0, H[:, 0, 2] / d0
        d1 = H[:, 1, 1] - l10 * H[:, 0, 1]
        tt = H[:, 1, 2] - l20 * H[:, 0, 1]
        l21 = tt / d1
        d2 = H[:, 2, 2] - l20 * H[:, 0, 2] - l21 * tt
        i0, i1, i2 = 1.0 / d0, 1.0 / d1, 1.0 / d2
        m20 = l10 * l21 - l20
        c = np.empty_like(H)
        c[:, 2, 2] = i2
        c[:, 1, 2] = c[:, 2, 1] = -l21 * i2
        c[:, 0, 2] = c[:, 2, 0] = m20 * i2
        c[:, 1, 1] = i1 + l21 * l21 * i2
        c[:, 0, 1] = c[:, 1, 0] = -l10 * i1 - l21 * c[:, 0, 2]
        c[:, 0, 0] = i0 + l10 * l10 * i1 + m20 * c[:, 0, 2]
    return c, np.stack([d0, d1, d2], -1)


def pivot_ratio(H):
    """min pivot / max diagonal entry per point (NaN where undefined)."""
    _, d = ldl_inverse(H)
    with np.errstate(invalid='ignore', divide='ignore'):
        return d.min(1) / np.max(np.diagonal(H, axis1=1, axis2=2), 1)


def classify(H, m):
    _, d = ldl_inverse(H)
    with np.errstate(invalid='ignore'):
        thr = PIVOT_RATIO * np.fmax.reduce(np.diagonal(H, axis1=1, axis2=2), 1)
        good = (d > thr[:, None]).all(1)
    return np.where(m == 0, NOOBS, np.where(good, OK, DEGENERATE)).astype(np.int32)


def covariance(project_jac, uv, pt_idx, cam_idx, pts, K, D, R, t, f_scale=50.0, sigma_px=1.0):
    """-> dict(cov (n, 3, 3), status (n,), report, H (n, 3, 3))."""
    H, swr2, m = normal_matrices(project_jac, uv, pt_idx, cam_idx, pts, K, D, R, t, f_scale)
    status = classify(H, m)
    inv, _ = ldl_inverse(H)
    ok = status == OK
    cov = np.where(ok[:, None, None], sigma_px * sigma_px * inv, np.nan)
    n_ok = int(ok.sum())
    dof = int(m[ok].sum()) - 3 * n_ok
    var = np.diagonal(cov[ok], axis1=1, axis2=2)
    report = dict(n_points=len(H), n_ok=n_ok, n_noobs=int((status == NOOBS).sum()),
                  n_degenerate=int((status == DEGENERATE).sum()),
                  var_min=float(var.min()) if n_ok else np.nan, var_max=float(var.max()) if n_ok else np.nan,
                  sigma_hat_px=float(np.sqrt(swr2[ok].sum() / dof)) if dof > 0 else np.nan)
    return dict(cov=cov, status=status, report=report, H=H)


def rel_error(S, Rf):
    """max |S - R| / sqrt(diag R (x) diag R) per point."""
    d = np.sqrt(np.einsum('nii->ni', Rf))
    return (np.abs(S - Rf) / (d[:, :, None] * d[:, None, :])).reshape(len(S), -1).max(1)
