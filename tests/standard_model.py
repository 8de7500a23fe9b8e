"""CPU reference of the standard (pinhole) camera model for the tests: a numpy restatement of
the formulas in include/acinoset_hip.h (ACS_CAMS_STANDARD), not a conftest.

    a = Y0/Y2, b = Y1/Y2, r2 = a^2 + b^2,  Y = R X + t
    cd = (1 + k1 r2 + k2 r2^2 + k3 r2^3) / (1 + k4 r2 + k5 r2^2 + k6 r2^3)
    xd = a cd + 2 p1 a b + p2 (r2 + 2 a^2),  yd = b cd + p1 (r2 + 2 b^2) + 2 p2 a b
    u = fx xd + cx, v = fy yd + cy

with d = (k1, k2, p1, p2, k3, k4, k5, k6), a shorter d zero-padded. `undistort` is
cv::undistortPoints with its default criteria (5 fixed-point iterations, no convergence test,
the `icdist < 0` guard), `triangulate_pair` the homogeneous DLT of cv::triangulatePoints.

The LM reference is `oracle.sba.sba_points` with its module-level `project` / `project_jac`
replaced (`patch_oracle`): the oracle reshapes its distortion argument to 4 columns, so it is
handed a (C, 4) stand-in whose column 0 is the camera index, and the replacements look the 8
coefficients up by it. oracle/ itself is untouched.
"""
import numpy as np

# the test scenes' coefficients (k1, k2, p1, p2, k3, k4, k5, k6), jittered per camera
BASE_COEFFS = np.array([-0.12, 0.03, 8e-4, -5e-4, -0.004, 0.05, -0.01, 0.002])


def jittered_coeffs(n_cams, seed, rel=0.05):
    """(n_cams, 8): BASE_COEFFS times (1 + N(0, rel)) per camera and coefficient."""
    rng = np.random.default_rng(seed)
    return BASE_COEFFS * (1.0 + rng.normal(0.0, rel, (n_cams, 8)))


def pad8(d, n=None):
    """Distortion coefficients in any of the scene-file shapes -> (n, 8), zero-padded."""
    d = np.asarray(d, np.float64)
    d = d.reshape(1, -1) if n is None and d.ndim < 2 else d.reshape(len(d) if n is None else n, -1)
    out = np.zeros((len(d), 8))
    out[:, :d.shape[1]] = d
    return out


def _normalised(X, R, t):
    Y = np.einsum('nij,nj->ni', R, X) + t.reshape(-1, 3)
    return Y, Y[:, 0] / Y[:, 2], Y[:, 1] / Y[:, 2]


def _distort(a, b, d, jac=False):
    k1, k2, p1, p2, k3, k4, k5, k6 = d.T
    r2 = a * a + b * b
    num = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    den = 1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3
    cd = num / den
    xd = a * cd + 2 * p1 * a * b + p2 * (r2 + 2 * a * a)
    yd = b * cd + p1 * (r2 + 2 * b * b) + 2 * p2 * a * b
    if not jac:
        return xd, yd
    dnum = k1 + 2 * k2 * r2 + 3 * k3 * r2 ** 2
    dden = k4 + 2 * k5 * r2 + 3 * k6 * r2 ** 2
    cp = (dnum - cd * dden) / den
    xa = cd + 2 * a * a * cp + 2 * p1 * b + 6 * p2 * a
    xb = 2 * a * b * cp + 2 * p1 * a + 2 * p2 * b
    yb = cd + 2 * b * b * cp + 6 * p1 * b + 2 * p2 * a
    return xd, yd, xa, xb, yb


def _batch(X, K, d, R, t):
    X = np.asarray(X, np.float64).reshape(-1, 3)
    n = len(X)
    K = np.broadcast_to(np.asarray(K, np.float64).reshape(-1, 3, 3), (n, 3, 3))
    R = np.broadcast_to(np.asarray(R, np.float64).reshape(-1, 3, 3), (n, 3, 3))
    t = np.broadcast_to(np.asarray(t, np.float64).reshape(-1, 3), (n, 3))
    d = np.asarray(d, np.float64)
    d = np.broadcast_to(pad8(d.reshape(-1, d.shape[-1]) if d.ndim > 1 else d), (n, 8))
    return X, K, d, R, t


def project(X, K, d, R, t):
    """(n, 3) points through one camera or per-point cameras (K (n,3,3), d (n, <= 8), R, t) -> (n, 2)."""
    X, K, d, R, t = _batch(X, K, d, R, t)
    _, a, b = _normalised(X, R, t)
    xd, yd = _distort(a, b, d)
    return np.stack([K[:, 0, 0] * xd + K[:, 0, 2], K[:, 1, 1] * yd + K[:, 1, 2]], -1)


def project_jac(X, K, d, R, t):
    """-> (uv (n, 2), J (n, 2, 3) = d uv / d X), analytic."""
    X, K, d, R, t = _batch(X, K, d, R, t)
    Y, a, b = _normalised(X, R, t)
    xd, yd, xa, xb, yb = _distort(a, b, d, jac=True)
    uv = np.stack([K[:, 0, 0] * xd + K[:, 0, 2], K[:, 1, 1] * yd + K[:, 1, 2]], -1)
    iz = 1.0 / Y[:, 2]
    # d(a, b)/dY = iz [[1, 0, -a], [0, 1, -b]]
    dab = np.zeros((len(X), 2, 3))
    dab[:, 0, 0] = dab[:, 1, 1] = iz
    dab[:, 0, 2] = -a * iz
    dab[:, 1, 2] = -b * iz
    duv = np.empty((len(X), 2, 2))
    duv[:, 0, 0] = K[:, 0, 0] * xa
    duv[:, 0, 1] = K[:, 0, 0] * xb
    duv[:, 1, 0] = K[:, 1, 1] * xb
    duv[:, 1, 1] = K[:, 1, 1] * yb
    return uv, duv @ dab @ R


def undistort(uv, K, d, iters=5):
    """cv::undistortPoints, default criteria: (n, 2) pixels -> (n, 2) normalised coordinates."""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    K = np.asarray(K, np.float64).reshape(3, 3)
    k1, k2, p1, p2, k3, k4, k5, k6 = pad8(np.asarray(d, np.float64).ravel())[0]
    x0 = (uv[:, 0] - K[0, 2]) / K[0, 0]
    y0 = (uv[:, 1] - K[1, 2]) / K[1, 1]
    x, y = x0.copy(), y0.copy()
    live = np.ones(len(uv), bool)
    for _ in range(iters):
        r2 = x * x + y * y
        ic = (1 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        bad = live & (ic < 0)
        x[bad], y[bad] = x0[bad], y0[bad]
        live &= ~bad
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x = np.where(live, (x0 - dx) * ic, x)
        y = np.where(live, (y0 - dy) * ic, y)
    return np.stack([x, y], -1)


def triangulate_pair(uva, uvb, Ka, da, Ra, ta, Kb, db, Rb, tb):
    """triangulate_points (src/lib/calib.py:53-62): undistort both views, homogeneous DLT."""
    xa, xb = undistort(uva, Ka, da), undistort(uvb, Kb, db)
    Pa = np.hstack([np.asarray(Ra).reshape(3, 3), np.asarray(ta).reshape(3, 1)])
    Pb = np.hstack([np.asarray(Rb).reshape(3, 3), np.asarray(tb).reshape(3, 1)])
    out = np.empty((len(xa), 3))
    for i in range(len(xa)):
        A = np.stack([xa[i, 0] * Pa[2] - Pa[0], xa[i, 1] * Pa[2] - Pa[1],
                      xb[i, 0] * Pb[2] - Pb[0], xb[i, 1] * Pb[2] - Pb[1]])
        h = np.linalg.svd(A)[2][-1]
        out[i] = h[:3] / h[3]
    return out


def triangulate_dense(uv, mask, K, D, R, t):
    """get_pairwise_3d_points_from_df on a dense (n, C, 2) tensor: the mean over the adjacent
    pairs (c, c + 1 mod C) both cameras saw, in pair order -> (xyz (n, 3), NaN without a pair; n_pairs)."""
    n, C = mask.shape
    D = pad8(D, C)
    s = np.zeros((n, 3))
    cnt = np.zeros(n, np.int32)
    for c in range(C):
        c2 = (c + 1) % C
        both = np.flatnonzero((mask[:, c] != 0) & (mask[:, c2] != 0))
        if len(both):
            s[both] += triangulate_pair(uv[both, c], uv[both, c2], K[c], D[c], R[c], t[c], K[c2], D[c2], R[c2], t[c2])
            cnt[both] += 1
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(cnt[:, None] > 0, s / cnt[:, None], np.nan), cnt


def oracle_stand_in(n_cams):
    """The (C, 4) `D` handed to the patched oracle: column 0 is the camera index."""
    D = np.zeros((n_cams, 4))
    D[:, 0] = np.arange(n_cams)
    return D


def patch_oracle(monkeypatch, coeffs):
    """Replace oracle.sba's projection by the standard model with `coeffs` (C, <= 8) per camera,
    for the duration of the test (or of a `pytest.MonkeyPatch.context()`)."""
    from oracle import sba as osba
    table = pad8(coeffs, len(coeffs))

    def look(D):
        return table[np.rint(np.asarray(D).reshape(-1, 4)[:, 0]).astype(int)]

    monkeypatch.setattr(osba, 'project', lambda X, K, D, R, t: project(X, K, look(D), R, t))
    monkeypatch.setattr(osba, 'project_jac', lambda X, K, D, R, t: project_jac(X, K, look(D), R, t))
    return osba
