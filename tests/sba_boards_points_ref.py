"""Numpy restatement of the rigid-board bundle adjustment with free points (acs_sba_boards_points), for
the tests, iterate for iterate. Built from sba_boards_ref (linearize, board_minv, apply) and
oracle.sba_ext (linearize), by import.

The problem (the one definition; also in include/acinoset_hip.h and acinoset_amd/csrc/sba_boards.hip):
  everything of sba_boards_ref: fisheye cameras c < C with fixed intrinsics, boards b < B with pose
  (R_b, t_b), object points p_j, uv (B, C, nc, 2), mask (B, C); and
  free points X_p, p < n, stored densely: pt_uv (n, C, 2), pt_mask (n, C); a camera sees a point at
  most once (slot = camera, K = C in the extrinsics SBA's terms);
  the same robust cost and weights for every residual (Cauchy with f_scale, Triggs
  wh = max((1 - z) w^2, 0.1 w)): F = F_boards + F_points; U and g_c of a camera sum over its board
  views and its point observations.
One LM, oracle/sba_ext.py's and sba_boards_ref's joined: Marquardt damping on every diagonal, M_b as
  sba_boards_ref.board_minv, M_p = (V_p + lam diag V_p + 1e-300 I)^-1 (zero where its determinant is
  not > 1e-280: a point without an observation takes no step and contributes nothing),
  S = sum U + lam D - sum_b W M_b W^T - sum_p W M_p W^T, b = -g_c + sum_b W M_b g_b + sum_p W M_p g_p,
  db and dX by back-substitution, gmax = max(|g_c|, |g_b|, |g_p|),
  |d|^2 = sum dc^2 + sum db^2 + sum dX^2, |x|^2 = sum |t_c|^2 + sum |t_b|^2 + sum |X_p|^2;
  accept / reject, the lambda schedule, LAM_MIN, the stop tests and the status names unchanged.
  The 6-DoF rigid gauge stays free.
"""
import numpy as np

import sba_boards_ref as bref
from oracle import sba_ext as oext
from oracle.sba_ext import LAM_MIN, rodrigues


def point_obs(pt_mask):
    """The seen (point, camera) pairs in (point, camera) order."""
    pi, ci = np.nonzero(np.asarray(pt_mask))
    return pi.astype(np.int64), ci.astype(np.int64)


def residuals(R, t, K, D, obj, bR, bt, uv, mask, X, pt_uv, pt_mask):
    """The board part as sba_boards_ref.residuals, then the seen (point, camera) pairs in (point,
    camera, row) order; flat."""
    rb = bref.residuals(R, t, K, D, obj, bR, bt, uv, mask)
    pi, ci = point_obs(pt_mask)
    if len(pi) == 0:
        return rb
    rp = oext.residuals(np.asarray(X).reshape(-1, 3), R, t, K, D, np.asarray(pt_uv)[pi, ci], pi, ci)
    return np.concatenate([rb, rp.ravel()])


def cost(R, t, K, D, obj, bR, bt, uv, mask, X, pt_uv, pt_mask, f):
    Fb = bref.cost(R, t, K, D, obj, bR, bt, uv, mask, f)
    pi, ci = point_obs(pt_mask)
    if len(pi) == 0:
        return Fb
    return Fb + oext.cost(X, R, t, K, D, pt_uv[pi, ci], pi, ci, f)


def linearize(R, t, K, D, obj, bR, bt, uv, mask, X, pt_uv, pt_mask, f_scale):
    """F, U (C,6,6), g_c (C,6) over both sides; W (B,C,6,6), V (B,6,6), g_b (B,6) of the boards;
    V_p (n,3,3), g_p (n,3) and the per-observation W_p (m,6,3) of the points."""
    F, U, gc, W, V, gb = bref.linearize(R, t, K, D, obj, bR, bt, uv, mask, f_scale)
    n = len(X)
    pi, ci = point_obs(pt_mask)
    Vp, gp, Wm = np.zeros((n, 3, 3)), np.zeros((n, 3)), np.zeros((0, 6, 3))
    if len(pi):
        Fp, Up, gcp, Vp, gp, Wm = oext.linearize(X, R, t, K, D, pt_uv[pi, ci], pi, ci, f_scale)[:6]
        F, U, gc = F + Fp, U + Up, gc + gcp
    return F, U, gc, W, V, gb, Vp, gp, Wm


def point_minv(Vp, lam):
    """M_p (n,3,3): the damped block's inverse, zero where its determinant is not > 1e-280."""
    M = np.zeros_like(Vp)
    for p in range(len(Vp)):
        Vd = Vp[p].copy()
        Vd[range(3), range(3)] = Vd[range(3), range(3)] * (1.0 + lam) + 1e-300
        with np.errstate(under='ignore'):
            det = np.linalg.det(Vd)
        if det > 1e-280:
            M[p] = np.linalg.inv(Vd)
    return M


def step(U, gc, W, V, gb, Vp, gp, Wm, mask, pt_mask, lam):
    """The LM step (dc (C,6), db (B,6), dX (n,3)) of the system at damping lam."""
    B, C = mask.shape
    pi, ci = point_obs(pt_mask)
    M, ok = bref.board_minv(V, lam, mask.sum(1))
    Mp = point_minv(Vp, lam)
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
    Zp = np.einsum('mij,mjk->mik', Wm, Mp[pi]) if len(pi) else Wm
    for o1 in range(len(pi)):
        c1 = ci[o1]
        rhs[6 * c1:6 * c1 + 6] += Zp[o1] @ gp[pi[o1]]
        for o2 in np.nonzero(pi == pi[o1])[0]:
            c2 = ci[o2]
            S[6 * c1:6 * c1 + 6, 6 * c2:6 * c2 + 6] -= Zp[o1] @ Wm[o2].T
    dc = np.linalg.solve(S, rhs).reshape(C, 6)
    acc = gb + np.einsum('bcij,ci->bj', W * mask[:, :, None, None], dc)
    db = -np.einsum('bij,bj->bi', M, acc)
    db[~ok] = 0.0
    accp = gp.copy()
    if len(pi):
        np.add.at(accp, pi, np.einsum('mij,mi->mj', Wm, dc[ci]))
    dX = -np.einsum('nij,nj->ni', Mp, accp)
    return dc, db, dX


def sba_boards_points(R0, t0, K, D, obj, bR0, bt0, uv, mask, X0, pt_uv, pt_mask, f_scale=1.0, max_iters=500,
                      ftol=1e-12, xtol=1e-12, gtol=1e-8, lam0=1e-3, trace=None):
    """The LM of the kernels, iterate for iterate. Returns (R, t, bR, bt, X, info). trace: a list; every
    iteration appends the dict oracle.sba_ext.sba_extrinsics writes (F, F_new, dn, xn, gmax, lam,
    accepted)."""
    R = np.array(R0, np.float64).reshape(-1, 3, 3)
    t = np.array(t0, np.float64).reshape(-1, 3)
    bR = np.array(bR0, np.float64).reshape(-1, 3, 3)
    bt = np.array(bt0, np.float64).reshape(-1, 3)
    X = np.array(X0, np.float64).reshape(-1, 3)
    K = np.asarray(K, np.float64)
    D = np.asarray(D, np.float64).reshape(-1, 4)
    obj = np.asarray(obj, np.float64).reshape(-1, 3)
    mask = np.asarray(mask) != 0
    pt_mask = np.asarray(pt_mask).reshape(len(X), len(R)) != 0
    pt_uv = np.asarray(pt_uv, np.float64).reshape(len(X), len(R), 2)
    args = (K, D, obj)
    data = (uv, mask)

    def lin(R, t, bR, bt, X):
        return linearize(R, t, *args, bR, bt, *data, X, pt_uv, pt_mask, f_scale)

    F, U, gc, W, V, gb, Vp, gp, Wm = lin(R, t, bR, bt, X)
    F0, lam, status, iters, nacc = F, lam0, 'maxiter', 0, 0
    while iters < max_iters:
        gmax = max(np.abs(gc).max(), np.abs(gb).max(), np.abs(gp).max() if len(X) else 0.0)
        if gmax <= gtol:
            status = 'gtol'
            break
        dc, db, dX = step(U, gc, W, V, gb, Vp, gp, Wm, mask, pt_mask, lam)
        Rn, tn = bref.apply(R, t, dc)
        bRn, btn = bref.apply(bR, bt, db)
        Xn = X + dX
        Fn = cost(Rn, tn, *args, bRn, btn, *data, Xn, pt_uv, pt_mask, f_scale)
        iters += 1
        dn = np.sqrt((dc ** 2).sum() + (db ** 2).sum() + (dX ** 2).sum())
        xn = np.sqrt((t ** 2).sum() + (bt ** 2).sum() + (X ** 2).sum())
        if trace is not None:
            trace.append(dict(F=F, F_new=Fn, dn=dn, xn=xn, gmax=gmax, lam=lam, accepted=bool(Fn < F)))
        if Fn < F:
            nacc += 1
            fconv = (F - Fn) <= ftol * abs(F)
            R, t, bR, bt, X = Rn, tn, bRn, btn, Xn
            lam = max(lam * 0.1, LAM_MIN)
            F, U, gc, W, V, gb, Vp, gp, Wm = lin(R, t, bR, bt, X)
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
    return R, t, bR, bt, X, dict(status=status, iters=iters, n_accepted=nacc, cost_before=F0, cost_after=F,
                                 lam=lam)


def make_rig(C, B, shape=(4, 3), n_pts=0, seed=0, views=None, mask=None, pt_vis=None, noise=0.0, radius=4.0):
    """sba_boards_ref.make_rig's ring of C cameras and B boards, with n_pts free points near the boards.
    mask: an explicit (B, C) board visibility (else `views` as sba_boards_ref.make_rig reads it).
    pt_vis: an explicit (n_pts, C) point visibility, (lo, hi) for a random number of cameras per
    point, or None for every camera. noise: px, on every observation. Returns sba_boards_ref's dict
    with X (n, 3) (the truth), pt_uv (n, C, 2) (zero where unseen) and pt_mask (n, C) uint8 added."""
    rig = bref.make_rig(C, B, shape=shape, seed=seed, views=views, noise=0.0, radius=radius)
    rng = np.random.default_rng(seed + 50000)
    K, D, R, t, obj = (rig[k] for k in ('K', 'D', 'R', 't', 'obj'))
    if mask is not None:
        mask = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8).reshape(B, C)
        uv = np.zeros((B, C, len(obj), 2))
        vb, vc = np.nonzero(mask)
        uv[vb, vc] = bref._project_views(R, t, K, D, obj, rig['bR'], rig['bt'], vb, vc)[2].reshape(len(vb), -1, 2)
        rig.update(uv=uv, mask=mask)
    if noise:
        rig['uv'] = (rig['uv'] + rng.normal(0, noise, rig['uv'].shape)) * rig['mask'][:, :, None, None]
    X = rng.uniform(-0.8, 0.8, (n_pts, 3)) * [1, 1, 0.4] + [1.9, 6.4, 0.6]
    if pt_vis is None:
        pm = np.ones((n_pts, C), np.uint8)
    elif isinstance(pt_vis, tuple):
        pm = np.zeros((n_pts, C), np.uint8)
        for p, k in enumerate(rng.integers(pt_vis[0], pt_vis[1] + 1, n_pts)):
            pm[p, rng.permutation(C)[:k]] = 1
    else:
        pm = np.ascontiguousarray(np.asarray(pt_vis) != 0, np.uint8).reshape(n_pts, C)
    pt_uv = np.zeros((n_pts, C, 2))
    pi, ci = point_obs(pm)
    if len(pi):
        p = oext.residuals(X, R, t, K, D, np.zeros((len(pi), 2)), pi, ci)  # the projection itself
        pt_uv[pi, ci] = p + rng.normal(0, noise, p.shape) if noise else p
    rig.update(X=X, pt_uv=pt_uv, pt_mask=pm)
    return rig


def perturb(rig, seed, rot=2e-3, trans=5e-3):
    """sba_boards_ref.perturb's start, and every point moved by `trans`."""
    R0, t0, bR0, bt0 = bref.perturb(rig, seed, rot, trans)
    X0 = rig['X'] + np.random.default_rng(seed + 70000).normal(0, trans, rig['X'].shape)
    return R0, t0, bR0, bt0, X0


def move_cameras(R, t, which, rotvec, shift):
    """The cameras `which` moved together, as one rigid body: rotated by rotvec about the mean of their
    centres and shifted. Returns new (R, t)."""
    R, t = np.array(R, np.float64).reshape(-1, 3, 3), np.array(t, np.float64).reshape(-1, 3)
    c = -np.einsum('cji,cj->ci', R, t)
    m = c[which].mean(0)
    Rg = rodrigues(np.asarray(rotvec, np.float64))
    for k in which:
        ck = Rg @ (c[k] - m) + m + shift
        R[k] = R[k] @ Rg.T
        t[k] = -R[k] @ ck
    return R, t


def dense_jacobian(R, t, K, D, obj, bR, bt, mask, X, pt_mask):
    """d residuals / d (camera, board and point perturbations), (2 m, 6 C + 6 B + 3 n): cameras, boards,
    points; rows in residuals()'s order."""
    B, C = np.asarray(mask).shape
    n = len(X)
    Jb = bref.dense_jacobian(R, t, K, D, obj, bR, bt, mask)
    pi, ci = point_obs(pt_mask)
    J = np.zeros((Jb.shape[0] + 2 * len(pi), 6 * C + 6 * B + 3 * n))
    J[:Jb.shape[0], :6 * C + 6 * B] = Jb
    if len(pi):
        Jc, Jp = oext.linearize(X, R, t, K, D, np.zeros((len(pi), 2)), pi, ci, 1.0)[6:8]
        for k in range(len(pi)):
            r0 = Jb.shape[0] + 2 * k
            J[r0:r0 + 2, 6 * ci[k]:6 * ci[k] + 6] = Jc[k]
            J[r0:r0 + 2, 6 * C + 6 * B + 3 * pi[k]:6 * C + 6 * B + 3 * pi[k] + 3] = Jp[k]
    return J


# ---- the problems of the GPU parity tests -------------------------------------------------------
# name -> (C, B, board shape, views per board, n points, cameras per point, seed). 0.5 px noise, the
# start of perturb(rig, seed + 100). The seed is the first from 0 at which every accept / reject
# decision of the compared iterations is at least sba_ext_shapes.TIE (1e-9) from a tie in this helper's
# trace (test_sba_boards_points_cpu.py holds the rule to them).
FIXED_ITERS = 8
PROBLEMS = {
    'c2_b2_nc4_n1': (2, 2, (2, 2), None, 1, None, 0),               # G = 2
    'c3_b5_nc12_n7': (3, 5, (4, 3), None, 7, (2, 3), 0),            # G = 4
    'c5_b4_nc12_n9': (5, 4, (4, 3), None, 9, None, 0),              # K = 5 in G = 8
    'c16_b40_nc54_n42': (16, 40, (9, 6), (2, 16), 42, (2, 16), 0),  # G = 16; point chunks of 41 and 1
    'c3_b65_nc4_n65': (3, 65, (2, 2), None, 65, (2, 3), 0),         # two board and two point chunks
    'c16_b20_nc4_n42': (16, 20, (2, 2), (2, 16), 42, (2, 16), 0),   # the same at C = 16 (chunks 19, 41)
}
_BUILT = {}


def problem(name):
    """(rig, start) of PROBLEMS[name], built once and never changed."""
    if name not in _BUILT:
        C, B, shape, views, n, pt_vis, seed = PROBLEMS[name]
        rig = make_rig(C, B, shape=shape, n_pts=n, seed=seed, views=views, pt_vis=pt_vis, noise=0.5)
        _BUILT[name] = (rig, perturb(rig, seed + 100))
    return _BUILT[name]


def solve(rig, start, trace=None, **kw):
    """sba_boards_points on a rig of make_rig and a start of perturb."""
    R0, t0, bR0, bt0, X0 = start
    return sba_boards_points(R0, t0, rig['K'], rig['D'], rig['obj'], bR0, bt0, rig['uv'], rig['mask'], X0,
                             rig['pt_uv'], rig['pt_mask'], trace=trace, **kw)


def split_rig(noise=0.5, seed=0):
    """The case the feature exists for: 4 ring cameras, boards 0-2 seen only by cameras {0, 1}, boards
    3-5 only by {2, 3}, (4, 3) corners, 6 non-coplanar points seen by all four cameras."""
    mask = np.zeros((6, 4), np.uint8)
    mask[:3, :2] = 1
    mask[3:, 2:] = 1
    return make_rig(4, 6, shape=(4, 3), n_pts=6, seed=seed, mask=mask, noise=noise)


def split_start(rig, seed=100, shift=0.02, angle=5e-3):
    """perturb's start, and cameras {2, 3} moved together by `shift` m and `angle` rad."""
    R0, t0, bR0, bt0, X0 = perturb(rig, seed)
    rng = np.random.default_rng(seed + 1)
    a, s = rng.normal(size=3), rng.normal(size=3)
    R0, t0 = move_cameras(R0, t0, [2, 3], angle * a / np.linalg.norm(a), shift * s / np.linalg.norm(s))
    return R0, t0, bR0, bt0, X0


def cross_distances(R, t):
    """The four centre distances between cameras {0, 1} and cameras {2, 3}."""
    c = -np.einsum('cji,cj->ci', np.asarray(R).reshape(-1, 3, 3), np.asarray(t).reshape(-1, 3))
    return np.array([np.linalg.norm(c[i] - c[j]) for i in (0, 1) for j in (2, 3)])


# The run to convergence of the GPU test (the C = 3 rig): the stop tolerance is
# sba_ext_shapes.choose_stop's on the trace of FREE_ITERS iterations without tolerances
# (test_sba_boards_points_cpu.py recomputes it).
FREE_ITERS = 48
from sba_ext_shapes import Stop  # noqa: E402

CONVERGED = Stop('ftol', 1.2258e-9, 6.50e-8, 2.31e-11, 29)  # (tolerance, the value above, below, iterations)
