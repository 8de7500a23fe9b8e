"""numpy restatement of acs_sba_boards_covariance (include/acinoset_hip.h): the
covariance of the camera poses and of every board pose of the rigid-board bundle adjustment, in a
chosen gauge. TEST INFRASTRUCTURE ONLY; builds on sba_boards_ref.linearize and sba_ext_cov_ref.

Definition (everything evaluated at the cameras and board poses passed in; nothing is solved):
  the problem and linearisation of acs_sba_boards: fisheye, 1 <= C <= 16, 3 <= nc <= 256, B >= 1,
  uv (B, C, nc, 2), mask (B, C); left perturbations R <- exp([dw]x) R, t <- t + dt for cameras and
  boards; J_cam = J_Y [-[R_c X]x | I], J_pt = J_Y R_c, J_brd = J_pt [-[R_b p_j]x | I]; Triggs
  weights wh = max((1 - z) w^2, 0.1 w), w = 1 / (1 + z), z = r^2 / f_scale^2; per seen view U_bc
  and W_bc (6 x 6), per board V_b = sum_views sum wh J_brd^T J_brd, all undamped.
  Board status: NOOBS without a view; DEGENERATE when an entry of diag V_b is not > 0, or a pivot
  of the unpivoted LDL^T of V_b scaled to unit diagonal fails d > 1e-9 (a NaN fails); OK
  otherwise. A board that is not OK is left out entirely (its U, W and V terms).
  S = sum_OK U_bc - sum_OK W_b V_b^-1 W_b^T (6C x 6C, symmetrised), W_b the 6C x 6 stack.
  Gauge generators G (6C x 6), per camera c: rotation theta: dw_c = -R_c theta, dt_c = 0;
  translation tau: dw_c = 0, dt_c = -R_c tau; the boards' parts dw_b = theta,
  dt_b = -[t_b]x theta + tau (board_generators) make the full normal matrix annihilate them.
  FREE:   cov_cc = sigma^2 [(S + mu Q Q^T)^-1 - Q Q^T / mu] (= sigma^2 pinv(S)), Q = orth(G),
          mu = max diag S.
  ANCHOR: camera a's pose held: Cm (6 x 6C) the identity on camera a, cov_cc = P cov_free P^T,
          P = I - G (Cm G)^-1 Cm, camera a's rows and columns exact zeros.
  Degenerate problem: with Ah = S + mu Q Q^T scaled to unit diagonal, a diagonal entry is not > 0,
  a pivot of the unpivoted LDL^T of Ah in natural order fails d > 1e-9, or G has rank < 6. Then
  every covariance is NaN. min_pivot as sba_ext_cov_ref.
  One camera: decided before S is formed; cov_cams exact zeros, status OK, min_pivot NaN, the
  boards get sigma^2 V_b^-1.
  Board b (OK): cov_b = sigma^2 V_b^-1 + V_b^-1 W_b^T cov_cc W_b V_b^-1; NaN for the others.
  sigma_hat^2 = sum w r^2 / dof over the OK boards' views, dof = m - 6 n_ok - (6C - 6); NaN when
  dof <= 0.
"""
import numpy as np

import sba_boards_ref as bref
import sba_ext_cov_ref as xref
from sba_ext_cov_ref import DEGENERATE, NOOBS, OK, PIVOT_TOL, skew  # noqa: F401


def gauge_generators(R):
    """G (6C x 6): the cameras' parts of the six rigid motions of the world frame."""
    C = len(R)
    G = np.zeros((6 * C, 6))
    for c in range(C):
        G[6 * c:6 * c + 3, 0:3] = -R[c]
        G[6 * c + 3:6 * c + 6, 3:6] = -R[c]
    return G


def board_generators(bt):
    """(6B x 6): the boards' parts, dw_b = theta, dt_b = -[t_b]x theta + tau."""
    B = len(bt)
    G = np.zeros((6 * B, 6))
    for b in range(B):
        G[6 * b:6 * b + 3, 0:3] = np.eye(3)
        G[6 * b + 3:6 * b + 6, 0:3] = -skew(bt[b])
        G[6 * b + 3:6 * b + 6, 3:6] = np.eye(3)
    return G


def unit_diagonal(V):
    """V scaled to unit diagonal (a diagonal entry that is not > 0 scales its row and column to zero)
    and whether every diagonal entry is > 0."""
    d = np.diagonal(V)
    pos = d > 0
    s = np.where(pos, 1.0 / np.sqrt(np.where(pos, d, 1.0)), 0.0)
    return V * np.outer(s, s), bool(pos.all())


def board_status(V, n_views):
    """The status rule on each board's V (B, 6, 6)."""
    st = np.empty(len(V), np.int32)
    for b, v in enumerate(V):
        if n_views[b] == 0:
            st[b] = NOOBS
            continue
        vh, pos = unit_diagonal(v)
        piv = xref.ldl_pivots(vh, PIVOT_TOL) if pos else np.array([0.0])
        st[b] = OK if pos and len(piv) == 6 and (piv > PIVOT_TOL).all() else DEGENERATE
    return st


def reduced_system(R, t, K, D, obj, bR, bt, uv, mask, f_scale):
    """-> dict: status (B,), S (6C x 6C, symmetrised), V (B, 6, 6), W (B, 6C, 6) (zero for the boards
    that are not OK and the unseen views), sum w r^2 and the residual count over the OK boards."""
    mask = np.asarray(mask) != 0
    B, C = mask.shape
    _, _, _, Wv, V, _ = bref.linearize(R, t, K, D, obj, bR, bt, uv, mask, f_scale)
    status = board_status(V, mask.sum(1))
    ok = status == OK
    km = mask & ok[:, None]
    S = np.zeros((6 * C, 6 * C))
    W = np.zeros((B, 6 * C, 6))
    wr2, m = 0.0, 0
    if km.any():
        _, U, _, Wk, _, _ = bref.linearize(R, t, K, D, obj, bR, bt, uv, km, f_scale)
        for c in range(C):
            S[6 * c:6 * c + 6, 6 * c:6 * c + 6] += U[c]
        for b in np.flatnonzero(ok):
            W[b] = Wk[b].reshape(6 * C, 6)
            S -= W[b] @ np.linalg.solve(V[b], W[b].T)
        r = bref.residuals(R, t, K, D, obj, bR, bt, uv, km)
        z = r * r / (f_scale * f_scale)
        wr2 = float((r * r / (1.0 + z)).sum())
        m = len(r)
    S = 0.5 * (S + S.T)
    return dict(status=status, S=S, V=V, W=W, wr2=wr2, m=m)


def gauge_basis(G):
    """Orthonormal basis of span G (6C x 6) and whether G has full rank 6."""
    Gn = G / np.maximum(np.linalg.norm(G, axis=0), 1e-300)
    U, s, _ = np.linalg.svd(Gn, full_matrices=False)
    return U, bool(G.shape[0] >= 6 and s[-1] > 1e-8 * s[0])


def free_covariance(S, G):
    """(S + mu Q Q^T)^-1 - Q Q^T / mu (sigma = 1), Ah, min_pivot, degenerate: sba_ext_cov_ref's with
    six generators."""
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
    piv = xref.ldl_pivots(Ah, PIVOT_TOL)
    if not (piv > PIVOT_TOL).all():
        return np.full_like(S, np.nan), Ah, float(np.nanmin(piv)) if not np.isnan(piv).all() else np.nan, True
    M = np.linalg.inv(Ah) * np.outer(s, s) - QQ / mu
    return 0.5 * (M + M.T), Ah, float(piv.min()), False


def constraint_matrix(C, a):
    Cm = np.zeros((6, 6 * C))
    Cm[:, 6 * a:6 * a + 6] = np.eye(6)
    return Cm


def covariance(R, t, K, D, obj, bR, bt, uv, mask, f_scale=1.0, sigma_px=1.0, gauge='anchor', anchor=0):
    """The whole definition -> dict: cov_cams (6C, 6C), cov_boards (B, 6, 6), status (B,), report
    (status, n_boards, n_ok, n_noobs, n_degenerate, dof, min_pivot, sigma_hat_px, rot_sd_max,
    trans_sd_max, board_rot_sd_max, board_trans_sd_max), S, Ah, G, V (B, 6, 6), W (B, 6C, 6)."""
    R = np.asarray(R, float).reshape(-1, 3, 3)
    t = np.asarray(t, float).reshape(-1, 3)
    bR = np.asarray(bR, float).reshape(-1, 3, 3)
    bt = np.asarray(bt, float).reshape(-1, 3)
    D = np.asarray(D, float).reshape(-1, 4)
    obj = np.asarray(obj, float).reshape(-1, 3)
    C, B = len(R), len(bR)
    sys_ = reduced_system(R, t, K, D, obj, bR, bt, uv, mask, f_scale)
    st, S = sys_['status'], sys_['S']
    G = gauge_generators(R)
    if C == 1:
        M, Ah, min_pivot, degenerate = np.zeros((6, 6)), None, np.nan, False
    else:
        M, Ah, min_pivot, degenerate = free_covariance(S, G)
        if not degenerate and gauge == 'anchor':
            M = xref.anchor_transform(M, G, constraint_matrix(C, anchor))
            M = 0.5 * (M + M.T)
            M[6 * anchor:6 * anchor + 6] = 0.0
            M[:, 6 * anchor:6 * anchor + 6] = 0.0
    s2 = sigma_px * sigma_px
    cov_cams = s2 * M
    cov_b = np.full((B, 6, 6), np.nan)
    if not degenerate:
        for b in np.flatnonzero(st == OK):
            Vi = np.linalg.inv(sys_['V'][b])
            c = s2 * Vi + Vi @ sys_['W'][b].T @ cov_cams @ sys_['W'][b] @ Vi
            cov_b[b] = 0.5 * (c + c.T)
    n_ok = int((st == OK).sum())
    dof = sys_['m'] - 6 * n_ok - (6 * C - 6)
    nan = float('nan')
    sd = np.sqrt(cov_cams.diagonal()).reshape(C, 6) if not degenerate else np.full((C, 6), np.nan)
    bsd = np.sqrt(np.diagonal(cov_b[st == OK], axis1=1, axis2=2)) if n_ok and not degenerate else None
    report = dict(status=int(degenerate), n_boards=B, n_ok=n_ok, n_noobs=int((st == NOOBS).sum()),
                  n_degenerate=int((st == DEGENERATE).sum()), dof=int(dof), min_pivot=min_pivot,
                  sigma_hat_px=float(np.sqrt(sys_['wr2'] / dof)) if dof > 0 else nan,
                  rot_sd_max=float(sd[:, :3].max()), trans_sd_max=float(sd[:, 3:].max()),
                  board_rot_sd_max=float(bsd[:, :3].max()) if bsd is not None else nan,
                  board_trans_sd_max=float(bsd[:, 3:].max()) if bsd is not None else nan)
    return dict(cov_cams=cov_cams, cov_boards=cov_b, status=st, report=report, S=S, Ah=Ah, G=G, V=sys_['V'],
                W=sys_['W'])


def dense_anchor_inverse(R, t, K, D, obj, bR, bt, mask, a, weights=None):
    """The inverse of the dense normal matrix J^T diag(weights) J of sba_boards_ref.dense_jacobian with
    camera a's six columns removed, put back as zero rows and columns: (6C + 6B, 6C + 6B), cameras
    first. The independent form of the anchored covariances."""
    J = bref.dense_jacobian(R, t, K, D, obj, bR, bt, mask)
    H = J.T @ (J if weights is None else J * np.asarray(weights)[:, None])
    keep = np.ones(len(H), bool)
    keep[6 * a:6 * a + 6] = False
    full = np.zeros_like(H)
    full[np.ix_(keep, keep)] = np.linalg.inv(H[np.ix_(keep, keep)])
    return full, H


rel_error = xref.rel_error
