"""numpy restatement of acs_sba_extrinsics_covariance (include/acinoset_hip.h): the
covariance of the camera poses and the joint covariance of the points of the points + extrinsics
SBA, in a chosen gauge. TEST INFRASTRUCTURE ONLY; builds on oracle.sba_ext.linearize.

Definition (everything evaluated at the state passed in; nothing is solved):
  camera parameters per camera (dw, dt): R <- exp([dw]x) R, t <- t + dt; Triggs weights
  wh = max((1 - z) w^2, 0.1 w), w = 1 / (1 + z), z = r^2 / f_scale^2 (oracle.sba_ext.linearize).
  Point status from its own V = sum wh J_pt^T J_pt: NOOBS without a usable observation,
  DEGENERATE when an LDL^T pivot fails d > 1e-9 max(V00, V11, V22), else OK. A point that is not
  OK is left out entirely (its U, W and V terms).
  S = sum U - sum_OK W V^-1 W^T (6C x 6C, symmetrised).
  Gauge generators G (6C x 7), per camera c: rotation theta: dw = -R_c theta; translation tau:
  dt = -R_c tau; scale: dt = t_c.  S G = 0.
  FREE:   cov = sigma^2 [(S + mu Q Q^T)^-1 - Q Q^T / mu] = sigma^2 pinv(S), Q = orth(G),
          mu = max diag S.
  ANCHOR(a, b): camera a's pose and the distance of the centres of a and b held:
          Cm (7 x 6C) = [I_6 on camera a ; e^T dc_b/d(dw_b, dt_b)], c = -R^T t,
          dc/d(dw, dt) = [-R^T [t]x | -R^T], e the unit baseline; P = I - G (Cm G)^-1 Cm,
          cov = P cov_free P^T, camera a's rows and columns exact zeros.
          Independent form: sigma^2 N (N^T S N)^-1 N^T, N a null-space basis of Cm.
  Degenerate problem: with A = S + mu Q Q^T and Ah = A scaled to unit diagonal (a diagonal entry
  that is not > 0 scales its row and column to zero), a pivot of the unpivoted LDL^T of Ah in
  natural order fails d > 1e-9 (a NaN fails), or G has rank < 7. min_pivot = the smallest pivot
  up to and including the first that fails. Then every covariance is NaN.
  Point i (OK): cov_i = sigma^2 V_i^-1 + V_i^-1 B_i^T cov_cc B_i V_i^-1, B_i the 6C x 3 stack of
  its W blocks.
  sigma_hat^2 = sum w r^2 / (m - 3 n_ok - (6C - 7)) over the OK points' residuals.
"""
import numpy as np

from oracle import sba_ext as oext

OK, NOOBS, DEGENERATE = 0, 1, 2
GAUGE_FREE, GAUGE_ANCHOR = 0, 1
PIVOT_TOL = 1e-9


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], float)


def synthetic(n_pts, C, seed):
    """The scene generator of the extrinsics SBA's GPU tests, unperturbed: a ring of C cameras,
    points in a slab, each seen by 2..C cameras. Returns K, D, R, t (C, 3), X, uv (noiseless),
    pi, ci."""
    from acinoset_amd import synth
    rng = np.random.default_rng(seed)
    sc = synth.ring_scene(C)
    K, D, R, t = sc.K, sc.D, sc.R, sc.t
    X = rng.uniform(-2, 2, (n_pts, 3)) * [1, 1, 0.3] + [1.9, 6.4, 0.5]
    pi, ci = [], []
    for p in range(n_pts):
        cs = rng.choice(C, size=rng.integers(2, C + 1), replace=False)
        pi += [p] * len(cs)
        ci += list(cs)
    pi, ci = np.array(pi, np.int32), np.array(ci, np.int32)
    uv = oext.residuals(X, R, t.reshape(-1, 3), K, D.reshape(-1, 4), np.zeros((len(pi), 2)), pi, ci)
    return K, D, R.copy(), t.copy().reshape(-1, 3), X.copy(), uv, pi, ci


def centre_jacobian(R, t):
    """d c / d(dw, dt) (3 x 6) of the camera centre c = -R^T t under R <- exp([dw]x) R, t <- t + dt."""
    return np.concatenate([-R.T @ skew(t), -R.T], 1)


def centres(R, t):
    return -np.einsum('cji,cj->ci', R, t)


def gauge_generators(R, t):
    C = len(R)
    G = np.zeros((6 * C, 7))
    for c in range(C):
        G[6 * c:6 * c + 3, 0:3] = -R[c]
        G[6 * c + 3:6 * c + 6, 3:6] = -R[c]
        G[6 * c + 3:6 * c + 6, 6] = t[c]
    return G


def ldl_pivots(A, tol=None):
    """Pivots of the unpivoted LDL^T in natural order, stopping after the first that fails
    d > tol (tol None: never stops)."""
    A = np.array(A, float)
    n = len(A)
    piv = []
    for k in range(n):
        d = A[k, k]
        piv.append(d)
        if tol is not None and not d > tol:
            break
        l = A[k + 1:, k] / d
        A[k + 1:, k + 1:] -= np.outer(l, A[k, k + 1:])
    return np.array(piv)


def point_status(V, nobs):
    """Round 13's rule on each point's V (n, 3, 3)."""
    st = np.empty(len(V), np.int32)
    for i, v in enumerate(V):
        if nobs[i] == 0:
            st[i] = NOOBS
            continue
        thr = PIVOT_TOL * max(v[0, 0], v[1, 1], v[2, 2])
        d0 = v[0, 0]
        l10, l20 = v[0, 1] / d0 if d0 else np.nan, v[0, 2] / d0 if d0 else np.nan
        d1 = v[1, 1] - l10 * v[0, 1]
        tt = v[1, 2] - l20 * v[0, 1]
        l21 = tt / d1 if d1 else np.nan
        d2 = v[2, 2] - l20 * v[0, 2] - l21 * tt
        st[i] = OK if (d0 > thr and d1 > thr and d2 > thr) else DEGENERATE
    return st


def reduced_system(X, R, t, K, D, uv, pi, ci, f_scale):
    """-> dict: status (n,), S (6C x 6C, symmetrised), V (n, 3, 3), B (n, 6C, 3) (zero rows of
    points that are not OK), sum w r^2 and residual count over the OK points."""
    n, C = len(X), len(R)
    pi = np.asarray(pi, np.int64)
    ci = np.asarray(ci, np.int64)
    use = (ci >= 0) & (ci < C)
    pi, ci, uv = pi[use], ci[use], np.asarray(uv, float)[use]
    D = np.asarray(D, float).reshape(-1, 4)
    t = np.asarray(t, float).reshape(-1, 3)
    nobs = np.bincount(pi, minlength=n)
    V = np.zeros((n, 3, 3))
    if len(pi):
        V = oext.linearize(X, R, t, K, D, uv, pi, ci, f_scale)[3]
    status = point_status(V, nobs)
    keep = status[pi] == OK
    pk, ck, uvk = pi[keep], ci[keep], uv[keep]
    S = np.zeros((6 * C, 6 * C))
    B = np.zeros((n, 6 * C, 3))
    wr2, m = 0.0, 0
    if len(pk):
        _, U, _, Vk, _, Wm, _, _ = oext.linearize(X, R, t, K, D, uvk, pk, ck, f_scale)
        for c in range(C):
            S[6 * c:6 * c + 6, 6 * c:6 * c + 6] += U[c]
        for o in range(len(pk)):
            B[pk[o], 6 * ck[o]:6 * ck[o] + 6] += Wm[o]
        for i in np.flatnonzero(status == OK):
            S -= B[i] @ np.linalg.solve(V[i], B[i].T)
        r = oext.residuals(X, R, t, K, D, uvk, pk, ck)
        z = r * r / (f_scale * f_scale)
        wr2 = float((r * r / (1.0 + z)).sum())
        m = 2 * len(pk)
    S = 0.5 * (S + S.T)
    return dict(status=status, S=S, V=V, B=B, wr2=wr2, m=m)


def gauge_basis(G):
    """Orthonormal basis of span G (6C x 7) and whether G has full rank 7."""
    Gn = G / np.maximum(np.linalg.norm(G, axis=0), 1e-300)
    U, s, _ = np.linalg.svd(Gn, full_matrices=False)
    full = G.shape[0] >= 7 and s[-1] > 1e-8 * s[0]
    return U, bool(full)


def free_covariance(S, G):
    """(S + mu Q Q^T)^-1 - Q Q^T / mu (sigma = 1), Ah, min_pivot, degenerate."""
    Q, full = gauge_basis(G)
    mu = S.diagonal().max()
    if not mu > 0:
        mu = 1.0
    if not full:
        return np.full_like(S, np.nan), None, 0.0, True
    QQ = Q @ Q.T
    A = S + mu * QQ
    d = A.diagonal()
    s = np.where(d > 0, 1.0 / np.sqrt(np.where(d > 0, d, 1.0)), 0.0)
    Ah = A * np.outer(s, s)
    piv = ldl_pivots(Ah, PIVOT_TOL)
    bad = bool(not (piv > PIVOT_TOL).all())
    if bad:
        return np.full_like(S, np.nan), Ah, float(np.nanmin(piv)) if not np.isnan(piv).all() else np.nan, True
    M = np.linalg.inv(Ah) * np.outer(s, s) - QQ / mu
    return 0.5 * (M + M.T), Ah, float(piv.min()), False


def constraint_matrix(R, t, a, b):
    C = len(R)
    Cm = np.zeros((7, 6 * C))
    Cm[:6, 6 * a:6 * a + 6] = np.eye(6)
    c = centres(R, t)
    e = c[b] - c[a]
    e = e / np.linalg.norm(e)
    Cm[6, 6 * b:6 * b + 6] = e @ centre_jacobian(R[b], t[b])
    return Cm


def anchor_transform(M, G, Cm):
    """The S-transform P M P^T, P = I - G (Cm G)^-1 Cm."""
    P = np.eye(len(M)) - G @ np.linalg.solve(Cm @ G, Cm)
    return P @ M @ P.T


def anchor_nullspace(S, Cm):
    """N (N^T S N)^-1 N^T, N an orthonormal null-space basis of Cm."""
    _, _, Vt = np.linalg.svd(Cm)
    N = Vt[7:].T
    return N @ np.linalg.solve(N.T @ S @ N, N.T)


def default_anchor(R, t):
    """Camera 0 and the camera whose centre is farthest from it (lowest index on ties)."""
    c = centres(np.asarray(R, float), np.asarray(t, float).reshape(-1, 3))
    d = np.linalg.norm(c - c[0], axis=1)
    return 0, int(np.argmax(d))


def covariance(X, R, t, K, D, uv, pi, ci, f_scale, sigma_px=1.0, gauge='anchor', anchor=(0, 1)):
    """The whole definition -> dict: cov_cams (6C, 6C), cov_points (n, 3, 3), status (n,), report
    (status, n_points, n_ok, n_noobs, n_degenerate, min_pivot, sigma_hat_px, dof, rot_sd_max,
    trans_sd_max), S, Ah."""
    R = np.asarray(R, float).reshape(-1, 3, 3)
    t = np.asarray(t, float).reshape(-1, 3)
    X = np.asarray(X, float).reshape(-1, 3)
    n, C = len(X), len(R)
    sys_ = reduced_system(X, R, t, K, D, uv, pi, ci, f_scale)
    st, S = sys_['status'], sys_['S']
    G = gauge_generators(R, t)
    M, Ah, min_pivot, degenerate = free_covariance(S, G)
    if not degenerate and gauge == 'anchor':
        a, b = anchor
        M = anchor_transform(M, G, constraint_matrix(R, t, a, b))
        M = 0.5 * (M + M.T)
        M[6 * a:6 * a + 6] = 0.0
        M[:, 6 * a:6 * a + 6] = 0.0
    s2 = sigma_px * sigma_px
    cov_cams = s2 * M
    cov_pts = np.full((n, 3, 3), np.nan)
    if not degenerate:
        for i in np.flatnonzero(st == OK):
            Vi = np.linalg.inv(sys_['V'][i])
            c = s2 * Vi + Vi @ sys_['B'][i].T @ cov_cams @ sys_['B'][i] @ Vi
            cov_pts[i] = 0.5 * (c + c.T)
    n_ok = int((st == OK).sum())
    dof = sys_['m'] - 3 * n_ok - (6 * C - 7)
    sd = np.sqrt(cov_cams.diagonal()).reshape(C, 6) if not degenerate else np.full((C, 6), np.nan)
    report = dict(status=int(degenerate), n_points=n, n_ok=n_ok, n_noobs=int((st == NOOBS).sum()),
                  n_degenerate=int((st == DEGENERATE).sum()), min_pivot=min_pivot,
                  sigma_hat_px=float(np.sqrt(sys_['wr2'] / dof)) if dof > 0 else np.nan, dof=int(dof),
                  rot_sd_max=float(sd[:, :3].max()), trans_sd_max=float(sd[:, 3:].max()))
    return dict(cov_cams=cov_cams, cov_points=cov_pts, status=st, report=report, S=S, Ah=Ah, V=sys_['V'],
                B=sys_['B'], G=G)


def rel_error(got, ref):
    """max |got - ref| / sqrt(diag ref (x) diag ref) over the entries whose variances are non-zero."""
    d = np.sqrt(np.abs(np.diagonal(ref, axis1=-2, axis2=-1)))
    den = d[..., :, None] * d[..., None, :]
    ok = den > 0
    return float((np.abs(got - ref)[ok] / den[ok]).max()) if ok.any() else 0.0
