"""CPU: the FTE covariance interface is declared and bound, and the block recursion that
acs_fte_covariance implements (selected inversion on the cyclic-reduction tree)
agrees with the dense inverse, in numpy, independently of the kernels.

Measure: for a block S against the reference R, max |S - R| / sqrt(diag R x diag R); bound
10 cond(H) 2.2e-16 (float64 inversion of a matrix of that condition number)."""
import os
import re

import numpy as np

from conftest import REPO

EPS = 2.2e-16


def test_header_and_binding_declare_fte_covariance():
    from acinoset_amd import _native
    src = open(os.path.join(REPO, 'include', 'acinoset_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    assert re.search(r'\bint\s+acs_fte_covariance\s*\(', code)
    assert 'acs_fte_cov_report' in code
    assert re.search(r'#define\s+ACS_ABI_VERSION\s+5\b', code)
    assert 'acs_fte_covariance' in _native.SYMBOLS
    lib = _native.load_library()
    fn = lib.acs_fte_covariance
    assert fn.argtypes is not None and len(fn.argtypes) == 22
    assert hasattr(_native.Context, 'fte_covariance')


def scaled_err(S, R):
    d = np.sqrt(np.abs(np.diag(R)))
    return float(np.max(np.abs(S - R) / np.outer(d, d)))


def block_selected_inverse(H, M, P, n_border):
    """Diagonal blocks of H^-1 for H = [[A, G], [G^T, T]], A block tridiagonal in super-blocks of
    3 frames (3P rows; the last block padded with the identity), by the recursion of
    acs_fte_covariance. Returns (list of S_ii, S_gg)."""
    B, nx = 3 * P, M * P
    n = (M + 2) // 3
    A = np.eye(n * B)
    A[:nx, :nx] = H[:nx, :nx]
    Gf = np.zeros((n * B, n_border))
    Gf[:nx] = H[:nx, nx:]
    T = H[nx:, nx:].copy()
    blk = lambda i: slice(i * B, (i + 1) * B)  # noqa: E731
    D = [A[blk(i), blk(i)].copy() for i in range(n)]
    E = {i: A[blk(i), blk(i - 1)].copy() for i in range(1, n)}   # H(i, previous active block)
    G = [Gf[blk(i)].copy() for i in range(n)]
    # everything outside the block tridiagonal + border pattern must be zero
    chk = A.copy()
    for i in range(n):
        for j in (i - 1, i, i + 1):
            if 0 <= j < n:
                chk[blk(i), blk(j)] = 0
    assert not chk.any()
    Dinv, Wl, Wr, Wg, levels = {}, {}, {}, {}, []
    s = 1
    while s < n:
        Enext = {}
        elim = list(range(s, n, 2 * s))
        for i in elim:
            l, r = i - s, i + s
            Dinv[i] = np.linalg.inv(D[i])
            Wl[i] = Dinv[i] @ E[i]
            Wg[i] = Dinv[i] @ G[i]
            D[l] -= E[i].T @ Wl[i]
            G[l] -= E[i].T @ Wg[i]
            T -= G[i].T @ Wg[i]
            if r < n:
                Wr[i] = Dinv[i] @ E[r].T
                D[r] -= E[r] @ Wr[i]
                G[r] -= E[r] @ Wg[i]
                Enext[r] = -E[r] @ Wl[i]
        E = Enext
        levels.append((s, elim))
        s *= 2
    top = np.block([[D[0], G[0]], [G[0].T, T]])
    ti = np.linalg.inv(top)
    Sii, Sg, Snx = {0: ti[:B, :B]}, {0: ti[:B, B:]}, {}
    Sgg = ti[B:, B:]
    for s, elim in reversed(levels):
        for i in elim:
            l, r = i - s, i + s
            hr = r < n
            Slr = Snx.get(l)
            Sil = -(Wl[i] @ Sii[l] + Wg[i] @ Sg[l].T)
            Sig = -(Wl[i] @ Sg[l] + Wg[i] @ Sgg)
            if hr:
                Sil -= Wr[i] @ Slr.T
                Sir = -(Wl[i] @ Slr + Wr[i] @ Sii[r] + Wg[i] @ Sg[r].T)
                Sig -= Wr[i] @ Sg[r]
            S = Dinv[i] - Sil @ Wl[i].T - Sig @ Wg[i].T
            if hr:
                S -= Sir @ Wr[i].T
                Snx[i] = Sir
            Snx[l] = Sil.T
            Sii[i], Sg[i] = S, Sig
    return [Sii[i] for i in range(n)], Sgg


def _oracle_problem(N, mode, sd, inter):
    from oracle import fte as ofte
    from acinoset_amd import synth
    scene = synth.load_scene_file()
    seq = synth.make_sequence(N, scene, mode=mode, seed=2, tau_max=0.004 if sd else 0.0)
    w = np.where(seq.likelihood > 0.5, 1.0 / 3.0, 0.0)
    prob = ofte.Problem(mode, seq.uv, w, scene.K, scene.D, scene.R, scene.t, seq.Ts, sd=sd, intermode=inter)
    X = np.concatenate([seq.x[:1], seq.x[:1], seq.x], 0) + np.random.default_rng(4).normal(0, 0.002,
                                                                                          (prob.M, prob.P))
    tau = np.zeros(prob.C)
    if sd:
        tau[1:] = np.random.default_rng(5).uniform(-0.003, 0.003, prob.C - 1)
    return prob, X, tau


def test_block_recursion_matches_dense_inverse():
    for N, mode, sd, inter in [(8, 'default_nolure', True, 'vel'), (11, 'head', False, 'pos')]:
        prob, X, tau = _oracle_problem(N, mode, sd, inter)
        _, H, _ = prob.linearize(X, tau)
        H = H.toarray()
        keep = np.setdiff1d(np.arange(prob.nv), prob.pinned())
        Hk = H[np.ix_(keep, keep)]
        ev = np.linalg.eigvalsh(Hk)
        assert ev.min() > 0, ev.min()
        bound = 10 * (ev.max() / ev.min()) * EPS
        R = np.linalg.inv(Hk)
        M, P = prob.M, prob.P
        Sii, Sgg = block_selected_inverse(Hk, M, P, len(keep) - M * P)
        worst = 0.0
        for f in range(M):
            a = (f % 3) * P
            S = Sii[f // 3][a:a + P, a:a + P]
            worst = max(worst, scaled_err(S, R[f * P:(f + 1) * P, f * P:(f + 1) * P]))
        if sd:
            worst = max(worst, scaled_err(Sgg, R[M * P:, M * P:]))
        print(f'N={N} {mode}: cond {ev.max() / ev.min():.2e}, recursion vs inv {worst:.2e}, bound {bound:.2e}')
        assert worst < bound, (N, mode, worst, bound)
