"""Numpy restatement of the rigid-board bundle adjustment (acs_sba_boards), for the tests.

The problem (the one definition; also in include/acinoset_hip.h and acinoset_amd/csrc/sba_boards.hip):
  cameras c = 0..C-1: fisheye, intrinsics fixed; boards b = 0..B-1 with a pose (R_b, t_b) from
  board to world coordinates; object points p_j (nc, 3), any rigid target;
  world point X_bj = R_b p_j + t_b; observations uv (B, C, nc, 2) and mask (B, C): a camera sees
  a board image with all its corners or not at all;
  residual r = project(R_c X_bj + t_c) - uv, cost F = 1/2 f^2 sum log1p(r^2 / f^2),
  w = 1 / (1 + z), wh = max((1 - z) w^2, 0.1 w), z = r^2 / f^2;
  left perturbations R <- exp([dw]x) R, t <- t + dt for cameras and boards;
  J_cam = J_Y [-[R_c X]x | I], J_pt = J_Y R_c, J_brd = J_pt [-[R_b p_j]x | I];
  per seen view U_bc = sum wh J_cam^T J_cam, W_bc = sum wh J_cam^T J_brd, g_c += sum w r J_cam;
  per board V_b = sum wh J_brd^T J_brd, g_b = sum w r J_brd.
LM: oracle/sba_ext.py's with "point" read as "board": Marquardt damping on every diagonal,
  M_b = (V_b + lam diag V_b + 1e-300 I)^-1, S = sum U + lam D - sum W M W^T, b = -g_c + sum W M g_b,
  db = -M_b (g_b + sum_c W_bc^T dc); accept iff F_new < F (lam /= 10, floor LAM_MIN), else lam *= 10;
  stop on gtol, ftol, xtol, lam > 1e16, max_iters; |d|^2 = sum dc^2 + sum db^2,
  |x|^2 = sum |t_c|^2 + sum |t_b|^2.
A board whose damped V_b is not positive definite (no view, a NaN, a pivot not > 0) takes no step in
that iteration (M_b = 0); its views still count in U and g_c. The rigid gauge is left free.

The projection and J_Y are oracle.sba_ext's, by import.
"""
import numpy as np

from oracle.sba_ext import LAM_MIN, _project_jy, _skew, rodrigues


def _views(mask):
    vb, vc = np.nonzero(np.asarray(mask))
    return vb, vc


def _project_views(R, t, K, D, obj, bR, bt, vb, vc):
    """Per seen view and corner: R_b p_j, X, R_c X, the projection and J_Y; flattened (nv * nc)."""
    nc = len(obj)
    Rp = np.einsum('vij,nj->vni', bR[vb], obj)                     # (nv, nc, 3)
    X = Rp + bt[vb][:, None, :]
    ci = np.repeat(vc, nc)
    RX = np.einsum('mij,mj->mi', R[ci], X.reshape(-1, 3))
    Y = RX + t[ci]
    p, JY = _project_jy(Y, K[ci], D[ci])
    return Rp.reshape(-1, 3), RX, p, JY, ci


def residuals(R, t, K, D, obj, bR, bt, uv, mask):
    """Residuals of the seen views in (board, camera, corner, row) order, flat."""
    vb, vc = _views(mask)
    p = _project_views(R, t, K, D, obj, bR, bt, vb, vc)[2]
    return (p - uv[vb, vc].reshape(-1, 2)).ravel()


def cost(R, t, K, D, obj, bR, bt, uv, mask, f):
    r = residuals(R, t, K, D, obj, bR, bt, uv, mask)
    return 0.5 * f * f * np.log1p(r * r / (f * f)).sum()


def jacobians(R, t, K, D, obj, bR, bt, mask):
    """J_cam and J_brd (m, 2, 6) per seen view and corner, with the view's board and camera (m,)."""
    vb, vc = _views(mask)
    Rp, RX, _, JY, ci = _project_views(R, t, K, D, obj, bR, bt, vb, vc)
    Jp = JY @ R[ci]
    Jc = np.concatenate([-JY @ _skew(RX), JY], -1)
    Jb = np.concatenate([-Jp @ _skew(Rp), Jp], -1)
    return Jc, Jb, np.repeat(vb, len(obj)), ci


def linearize(R, t, K, D, obj, bR, bt, uv, mask, f_scale):
    """F, U (C,6,6), g_c (C,6), W (B,C,6,6) per view, V (B,6,6), g_b (B,6)."""
    B, C = np.asarray(mask).shape
    f2 = f_scale * f_scale
    vb, vc = _views(mask)
    Jc, Jb, bi, ci = jacobians(R, t, K, D, obj, bR, bt, mask)
    r = residuals(R, t, K, D, obj, bR, bt, uv, mask).reshape(-1, 2)
    z = r * r / f2
    w = 1.0 / (1.0 + z)
    wh = np.maximum((1.0 - z) * w * w, 0.1 * w)
    F = 0.5 * f2 * np.log1p(z).sum()
    U = np.zeros((C, 6, 6))
    gc = np.zeros((C, 6))
    V = np.zeros((B, 6, 6))
    gb = np.zeros((B, 6))
    W = np.zeros((B, C, 6, 6))
    np.add.at(U, ci, np.einsum('md,mdi,mdj->mij', wh, Jc, Jc))
    np.add.at(gc, ci, np.einsum('md,md,mdi->mi', w, r, Jc))
    np.add.at(V, bi, np.einsum('md,mdi,mdj->mij', wh, Jb, Jb))
    np.add.at(gb, bi, np.einsum('md,md,mdi->mi', w, r, Jb))
    np.add.at(W, (bi, ci), np.einsum('md,mdi,mdj->mij', wh, Jc, Jb))
    return F, U, gc, W, V, gb


def board_minv(V, lam, n_views):
    """M_b (B,6,6) and whether each board steps: the damped block by Cholesky, zero where the board
    has no view, a NaN or a pivot that is not > 0."""
    M = np.zeros_like(V)
    ok = np.zeros(len(V), bool)
    for b in range(len(V)):
        Vd = V[b].copy()
        Vd[range(6), range(6)] = Vd[range(6), range(6)] * (1.0 + lam) + 1e-300
        if n_views[b] == 0 or not np.all(np.isfinite(Vd)):
            continue
        try:
            L = np.linalg.cholesky(Vd)
        except np.linalg.LinAlgError:
            continue
        Li = np.linalg.inv(L)
        M[b] = Li.T @ Li
        ok[b] = True
    return M, ok


def step(U, gc, W, V, gb, mask, lam):
    """The LM step (dc (C,6), db (B,6)) of the system at damping lam."""
    B, C = mask.shape
    M, ok = board_minv(V, lam, mask.sum(1))
    S = np.zeros((6 * C, 6 * C))
    for c in range(C):
        Ud = U[c].copy()
        Ud[range(6), range(6)] += lam * np.maximum(np.diag(U[c]), 1e-12)
        S[6 * c:6 * c + 6, 6 * c:6 * c + 6] += Ud
    rhs = -gc.reshape(-1).copy()
    for b in range(B):
        cs = np.nonzero(mask[b])[0]
        for c1 in cs:
            Z = W[b, c1] @ M[b]
            rhs[6 * c1:6 * c1 + 6] += Z @ gb[b]
            for c2 in cs:
                S[6 * c1:6 * c1 + 6, 6 * c2:6 * c2 + 6] -= Z @ W[b, c2].T
    dc = np.linalg.solve(S, rhs).reshape(C, 6)
    acc = gb + np.einsum('bcij,ci->bj', W * mask[:, :, None, None], dc)
    db = -np.einsum('bij,bj->bi', M, acc)
    db[~ok] = 0.0
    return dc, db


def apply(R, t, d):
    """Left perturbation of poses (n,3,3), (n,3) by d (n,6) = (dw, dt)."""
    Rn = np.array([rodrigues(d[i, :3]) @ R[i] for i in range(len(R))]).reshape(-1, 3, 3)
    return Rn, t + d[:, 3:]


def sba_boards(R0, t0, K, D, obj, bR0, bt0, uv, mask, f_scale=1.0, max_iters=500, ftol=1e-12, xtol=1e-12,
               gtol=1e-8, lam0=1e-3):
    """The LM of the kernels, iterate for iterate. Returns (R, t, bR, bt, info)."""
    R = np.array(R0, np.float64).reshape(-1, 3, 3)
    t = np.array(t0, np.float64).reshape(-1, 3)
    bR = np.array(bR0, np.float64).reshape(-1, 3, 3)
    bt = np.array(bt0, np.float64).reshape(-1, 3)
    K = np.asarray(K, np.float64)
    D = np.asarray(D, np.float64).reshape(-1, 4)
    obj = np.asarray(obj, np.float64).reshape(-1, 3)
    mask = np.asarray(mask) != 0
    F, U, gc, W, V, gb = linearize(R, t, K, D, obj, bR, bt, uv, mask, f_scale)
    F0, lam, status, iters, nacc = F, lam0, 'maxiter', 0, 0
    while iters < max_iters:
        gmax = max(np.abs(gc).max(), np.abs(gb).max())
        if gmax <= gtol:
            status = 'gtol'
            break
        dc, db = step(U, gc, W, V, gb, mask, lam)
        Rn, tn = apply(R, t, dc)
        bRn, btn = apply(bR, bt, db)
        Fn = cost(Rn, tn, K, D, obj, bRn, btn, uv, mask, f_scale)
        iters += 1
        dn = np.sqrt((dc ** 2).sum() + (db ** 2).sum())
        xn = np.sqrt((t ** 2).sum() + (bt ** 2).sum())
        if Fn < F:
            nacc += 1
            fconv = (F - Fn) <= ftol * abs(F)
            R, t, bR, bt = Rn, tn, bRn, btn
            lam = max(lam * 0.1, LAM_MIN)
            F, U, gc, W, V, gb = linearize(R, t, K, D, obj, bR, bt, uv, mask, f_scale)
            if fconv:
                status = 'ftol'
                break
            if dn <= xtol * (xtol + xn):
                status = 'xtol'
                break
        else:
            lam *= 10.0
            if lam > 1e16:
                status = 'stalled'
                break
    return R, t, bR, bt, dict(status=status, iters=iters, n_accepted=nacc, cost_before=F0, cost_after=F, lam=lam)


def board_object_pts(shape, square):
    """create_board_object_pts in float64."""
    obj = np.zeros((shape[0] * shape[1], 3))
    obj[:, :2] = np.mgrid[0:shape[0], 0:shape[1]].T.reshape(-1, 2) * square
    return obj


def make_rig(C, B, shape=(4, 3), square=0.1, radius=4.0, seed=0, views=None, noise=0.0, obj=None):
    """A ring of C cameras (synth.ring_scene) looking at its centre and B boards at random poses near
    it. views: per board the number of cameras that see it, an int array (B,) or (lo, hi) for a random
    number in lo..hi; default every camera. Returns a dict: K, D (C,4), R, t (C,3) (the truth), obj,
    bR, bt (the truth), uv (B,C,nc,2) (zero where unseen) and mask (B,C) uint8."""
    from acinoset_amd import synth
    rng = np.random.default_rng(seed)
    sc = synth.ring_scene(C, radius=radius)
    K, D, R, t = sc.K, sc.D.reshape(-1, 4), sc.R, sc.t.reshape(-1, 3)
    obj = board_object_pts(shape, square) if obj is None else np.asarray(obj, np.float64)
    bR = np.array([rodrigues(rng.normal(0, 1.0, 3)) for _ in range(B)])
    bt = rng.uniform(-0.8, 0.8, (B, 3)) * [1, 1, 0.4] + [1.9, 6.4, 0.6]
    if views is None:
        n_views = np.full(B, C)
    elif isinstance(views, tuple):
        n_views = rng.integers(views[0], views[1] + 1, B)
    else:
        n_views = np.broadcast_to(np.asarray(views), (B,))
    mask = np.zeros((B, C), np.uint8)
    for b in range(B):
        mask[b, rng.permutation(C)[:n_views[b]]] = 1
    uv = np.zeros((B, C, len(obj), 2))
    vb, vc = np.nonzero(mask)
    p = _project_views(R, t, K, D, obj, bR, bt, vb, vc)[2]
    uv[vb, vc] = (p + rng.normal(0, noise, p.shape) if noise else p).reshape(len(vb), len(obj), 2)
    return dict(K=K, D=D, R=R, t=t, obj=obj, bR=bR, bt=bt, uv=uv, mask=mask)


def perturb(rig, seed, rot=2e-3, trans=5e-3):
    """A start near the truth: every camera but the first and every board moved a little."""
    rng = np.random.default_rng(seed)
    C, B = len(rig['R']), len(rig['bR'])
    dc = np.concatenate([rng.normal(0, rot, (C, 3)), rng.normal(0, trans, (C, 3))], 1)
    dc[0] = 0.0
    db = np.concatenate([rng.normal(0, rot, (B, 3)), rng.normal(0, trans, (B, 3))], 1)
    R0, t0 = apply(rig['R'], rig['t'], dc)
    bR0, bt0 = apply(rig['bR'], rig['bt'], db)
    return R0, t0, bR0, bt0


def centre_distances(R, t):
    """Pairwise distances of the camera centres c = -R^T t (gauge-invariant), (C (C - 1) / 2,)."""
    c = -np.einsum('cji,cj->ci', np.asarray(R).reshape(-1, 3, 3), np.asarray(t).reshape(-1, 3))
    i, j = np.triu_indices(len(c), 1)
    return np.linalg.norm(c[i] - c[j], axis=1)


def free_corners(rig, bR, bt):
    """The same data posed as free corners for the points + extrinsics SBA: (points_2d, points_3d,
    point_indices, camera_indices) with one 3-D point per board corner."""
    obj, mask, uv = rig['obj'], rig['mask'], rig['uv']
    nc = len(obj)
    X = (np.einsum('bij,nj->bni', bR, obj) + bt[:, None, :]).reshape(-1, 3)
    vb, vc = np.nonzero(mask)
    pi = (vb[:, None] * nc + np.arange(nc)).ravel()
    ci = np.repeat(vc, nc)
    return uv[vb, vc].reshape(-1, 2), X, pi, ci


def dense_jacobian(R, t, K, D, obj, bR, bt, mask):
    """d residuals / d (camera and board perturbations), (2 m, 6 C + 6 B): cameras first."""
    B, C = np.asarray(mask).shape
    Jc, Jb, bi, ci = jacobians(R, t, K, D, obj, bR, bt, mask)
    J = np.zeros((len(Jc), 2, 6 * C + 6 * B))
    for k in range(len(Jc)):
        J[k, :, 6 * ci[k]:6 * ci[k] + 6] = Jc[k]
        J[k, :, 6 * C + 6 * bi[k]:6 * C + 6 * bi[k] + 6] = Jb[k]
    return J.reshape(-1, 6 * C + 6 * B)


def free_corner_jacobian(R, t, K, D, obj, bR, bt, mask):
    """The same data with every corner a free 3-D point: (2 m, 6 C + 3 B nc), J_cam and J_pt."""
    B, C = np.asarray(mask).shape
    nc = len(obj)
    vb, vc = _views(mask)
    _, RX, _, JY, ci = _project_views(R, t, K, D, obj, bR, bt, vb, vc)
    Jp = JY @ R[ci]
    Jc = np.concatenate([-JY @ _skew(RX), JY], -1)
    pi = (vb[:, None] * nc + np.arange(nc)).ravel()
    J = np.zeros((len(Jc), 2, 6 * C + 3 * B * nc))
    for k in range(len(Jc)):
        J[k, :, 6 * ci[k]:6 * ci[k] + 6] = Jc[k]
        J[k, :, 6 * C + 3 * pi[k]:6 * C + 3 * pi[k] + 3] = Jp[k]
    return J.reshape(-1, 6 * C + 3 * B * nc)
