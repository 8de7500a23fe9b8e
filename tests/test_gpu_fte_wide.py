"""GPU: the FTE solve's size-selected paths, at every super-block shape.

Most of csrc/fte.hip is chosen by problem size: k_cr_level's one-wave-per-column-block path
(`w`: upper tiles, symmask, own_all, the perm tables, the GB2 idle-wave loads) runs only while
a level's grid is past the chip, the 512-thread compact-row k_cr_assemble_build only past two
rounds of the CUs, k_fte_linearize<5> past 1,024 frames. The sizes here are the smallest at
which those paths exist, found through acs_fte_debug_plan (the dispatch's own functions), and
every test first asserts through it that its case runs the path it is named for:

  N_W    smallest N at which, for every mode and border width, levels 0 and 1 are `w` and
         level 0 runs the narrowest split of its shape (770 on 256 CUs: nsplit 1 w, 2 w; GB2 and
         NB = 6 shapes 2 w, 2 w)
  N_3W   smallest N at which 'default' (NB = 6) has a `w` level with nsplit = 3 (386)
  N_ASM  smallest N that takes the 512-thread assembly (6 n_cu - 1 = 1,535); also
         k_fte_linearize<5> and three `w` levels (1 w, 1 w, 2 w / 2 w, 2 w, 2 w)

The 6-camera scene file gives one border column-block (GR = 16), synth.ring_scene(16) two
(GR = 32, the GB2 instances); variable delays build through k_cr_build and take the non-DUP
instances; no delay gives Cg = 0.

The issue's cases start from tau = 0 (the solve's default). There every term a frame adds to the
rows of its two neighbours (the `prev` / `prev2` terms: the second-round entries of
assemble_row, whose thread range is at its limit at Cg = 16) is exactly zero, so the `-tau`
cases of (a) and (b) start from delays of +-0.3 Ts. A library whose compact rows skipped the
last of those entries passed every tau = 0 single-step and block case and fails the `-tau` steps
(and the three-step case); one whose survivors ignored `symmask` fails all of (a) and (c).
(Cases below: size-mode-cameras[-delay-intermode][-tau] x iterations.)

(a) One LM step (and three, at N_ASM) against the oracle's sparse solve: the oracle's own
    functions (linearize, the damping and pins of oracle.fte._solve, _solve_step, cost), one
    iteration at a time so the step and its floor come from one factorisation. The loop equals
    oracle.fte.solve bit for bit (checked on the CPU at head/6/770 and default_nolure/6/1535x3).
    Tolerance: the project's (1e-9 on X, 1e-12 on tau, 1e-11 with variable delays: the N <= 64
    tests), unless the reference itself cannot hold it: the floor of a case is |d - d'| with d'
    one refinement step further (residual A d + g accumulated in long double over the COO
    entries), and where 10 x floor exceeds the project's value the case takes 10 x floor. The
    floor is computed from the reference alone, in the test; the GPU's error never sets it.
    Measured on the MI355X box (this reference, one BLAS thread; X / tau). Every floor is below a
    tenth of the project's value except tau with variable delays (the oracle's sparse LU), so
    those two cases take 10 x floor and the rest run at 1e-9 / 1e-12:
      N_W-head-6 x1 floor 4.9e-15 / 0.0 tol 1.0e-9 / 1.0e-12 GPU 7.0e-15 / 0.0
      N_W-head-16 x1 floor 3.8e-15 / 0.0 tol 1.0e-9 / 1.0e-12 GPU 6.2e-15 / 0.0
      N_W-upper_body-6 x1 floor 1.4e-14 / 5.7e-16 tol 1.0e-9 / 1.0e-12 GPU 2.4e-14 / 4.6e-15
      N_W-upper_body-16 x1 floor 1.5e-14 / 0.0 tol 1.0e-9 / 1.0e-12 GPU 1.8e-14 / 0.0
      N_W-default_nolure-16 x1 floor 4.6e-14 / 0.0 tol 1.0e-9 / 1.0e-12 GPU 7.9e-14 / 0.0
      N_W-default-6 x1 floor 4.4e-14 / 0.0 tol 1.0e-9 / 1.0e-12 GPU 1.0e-13 / 0.0
      N_W-default-16 x1 floor 4.5e-14 / 0.0 tol 1.0e-9 / 1.0e-12 GPU 9.5e-14 / 0.0
      N_W-head-6-variable-vel x1 floor 7.1e-14 / 1.0e-11 tol 1.0e-9 / 1.0e-10 GPU 7.0e-14 / 1.0e-11
      N_W-default_nolure-6-variable-vel x1 floor 1.6e-11 / 3.1e-12 tol 1.0e-9 / 3.1e-11 GPU 1.6e-11 / 3.1e-12
      N_W-default_nolure-6-nodelay-pos x1 floor 3.9e-14 / 0.0 tol 1.0e-9 / 1.0e-12 GPU 9.1e-14 / 0.0
      N_W-upper_body-6-const-acc x1 floor 1.4e-14 / 5.7e-16 tol 1.0e-9 / 1.0e-12 GPU 2.4e-14 / 4.6e-15
      N_3W-default-6 x1 floor 4.8e-14 / 1.7e-17 tol 1.0e-9 / 1.0e-12 GPU 1.1e-13 / 3.8e-17
      N_3W-default-16 x1 floor 3.9e-14 / 0.0 tol 1.0e-9 / 1.0e-12 GPU 9.3e-14 / 0.0
      N_ASM-head-6 x1 floor 5.3e-15 / 0.0 tol 1.0e-9 / 1.0e-12 GPU 7.1e-15 / 0.0
      N_ASM-head-16 x1 floor 5.7e-15 / 0.0 tol 1.0e-9 / 1.0e-12 GPU 7.8e-15 / 0.0
      N_ASM-upper_body-16 x1 floor 1.4e-14 / 2.3e-16 tol 1.0e-9 / 1.0e-12 GPU 1.8e-14 / 6.2e-16
      N_ASM-default_nolure-6-nodelay-pos x1 floor 7.5e-14 / 0.0 tol 1.0e-9 / 1.0e-12 GPU 8.9e-14 / 0.0
      N_ASM-default-6 x1 floor 5.7e-14 / 7.8e-17 tol 1.0e-9 / 1.0e-12 GPU 8.8e-14 / 2.5e-15
      N_ASM-head-16-tau x1 floor 6.4e-15 / 0.0 tol 1.0e-9 / 1.0e-12 GPU 9.9e-15 / 0.0
      N_ASM-default-6-tau x1 floor 4.5e-14 / 1.5e-16 tol 1.0e-9 / 1.0e-12 GPU 8.3e-14 / 7.5e-16
      N40-default-16-tau x1 floor 2.9e-14 / 1.1e-16 tol 1.0e-9 / 1.0e-12 GPU 6.4e-14 / 2.7e-16
      N_ASM-default_nolure-6 x3 floor 4.3e-13 / 6.7e-16 tol 1.0e-9 / 1.0e-12 GPU 1.4e-11 / 4.7e-15
      N_ASM-head-16 x3 floor 2.7e-13 / 0.0 tol 1.0e-9 / 1.0e-12 GPU 6.8e-13 / 0.0
(b) The assembled, damped (lam = 1e-3) blocks against the oracle's sparse normal matrix plus
    lam max(H_ii, 1e-12), cut into 3-frame blocks: bitwise symmetry, identity padding, and every
    block within 1e-8 after scaling rows and columns by 1/sqrt(diag) of the reference (an angle
    entry cannot hide under a 1e8 position entry). 1e-8 is the project's figure for the normal
    matrix (test_fte_eval_matches_oracle).
(c) The blocks after 1, 2, 3 reduction levels against the float64 Schur complement of the same
    oracle blocks onto each survivor 2^L m, formed twice: eliminating the two runs of 2^L - 1
    neighbours as one dense solve each, and level by level. The GPU (Newton-refined tile
    inverses, another summation order) may differ from the first form by 1,000 x the two forms'
    disagreement on the scaled blocks; a failure names the level and the block.
    Measured maximum of (b), scaled error:
      N_ASM-head-6 4.4e-16
      N_ASM-head-16 4.4e-16
      N_ASM-upper_body-6 4.4e-16
      N_ASM-upper_body-16 4.4e-16
      N_ASM-default_nolure-6 1.1e-14
      N_ASM-default_nolure-16 2.4e-15
      N_ASM-default-6 2.8e-14
      N_ASM-default-16 2.7e-15
      N_ASM-default_nolure-6-nodelay-pos 1.1e-14
      N40-default-16 1.4e-15
      N_ASM-head-16-tau 4.4e-16
      N_ASM-default-6-tau 1.3e-14
      N40-default-16-tau 2.6e-15
    Measured in (c), two-form disagreement / GPU error at L = 1, 2, 3:
      N_W-head-6 7.6e-15 / 9.3e-15 5.4e-14 / 7.2e-14 4.3e-14 / 7.2e-14
      N_W-head-16 8.1e-15 / 9.3e-15 5.2e-14 / 7.2e-14 5.2e-14 / 6.8e-14
      N_W-upper_body-6 8.0e-15 / 1.1e-14 6.9e-14 / 7.7e-14 6.3e-14 / 6.6e-14
      N_W-upper_body-16 1.0e-14 / 1.2e-14 8.2e-14 / 8.2e-14 5.0e-14 / 6.1e-14
      N_W-default_nolure-6 1.1e-14 / 1.5e-14 2.0e-13 / 2.0e-13 2.3e-13 / 2.3e-13
      N_W-default_nolure-16 1.3e-14 / 1.4e-14 7.5e-14 / 7.9e-14 8.8e-14 / 8.8e-14
      N_W-default-6 1.2e-14 / 1.6e-14 1.6e-13 / 1.6e-13 1.8e-13 / 1.8e-13
      N_W-default-16 1.2e-14 / 1.5e-14 9.6e-14 / 9.6e-14 8.9e-14 / 8.9e-14
      N_3W-default-6 1.2e-14 / 1.4e-14 2.5e-13 / 2.5e-13 1.4e-13 / 1.4e-13
      N_3W-default-16 9.9e-15 / 1.3e-14 9.7e-14 / 9.7e-14 9.7e-14 / 9.7e-14

'default' with the 6-camera scene: initial_state leaves the lure at the world origin, which is
camera 0 of the scene file, where the projection is singular (NaN in the oracle); those cases
start the lure at its mean true position.
"""
import collections

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import fte as ofte, kinematics as okin
from acinoset_amd import _native, kinematics as pkin
from test_gpu_fte import _problem

pytestmark = pytest.mark.gpu

MODES = ('head', 'upper_body', 'default_nolure', 'default')
LAM = 1e-3
Case = collections.namedtuple('Case', 'size mode n_cams sd inter sd_mode seed tau')


def _case(size, mode, n_cams=6, sd=True, inter=None, sd_mode='const', seed=2, tau=False):
    return Case(size, mode, n_cams, sd, inter or ('vel' if sd else 'pos'), sd_mode, seed, tau)


def _id(c):
    if not isinstance(c, Case):
        return str(c)
    delay = 'nodelay' if not c.sd else c.sd_mode
    return f'{c.size}-{c.mode}-{c.n_cams}cam-{delay}-{c.inter}' + ('-tau' if c.tau else '')


def _P(mode):
    return pkin.build_table(mode).P


def _plan(ctx, c, N):
    return _native.fte_debug_plan(N, _P(c.mode), c.n_cams, shutter_delay=c.sd, sd_mode=c.sd_mode, ctx=ctx)


def find_sizes(plan):
    """(N_W, N_3W, N_ASM) of the module docstring; plan(N, mode, n_cams) -> fte_debug_plan dict."""
    def narrow(p):  # cr_nsplit's `need`: the narrowest split of the shape
        NB = p['BP'] // 16
        NBB = 2 * NB + p['GR'] // 16
        n = -(-NBB // (16 - NB))
        while p['GR'] > 16 and 1 < n < NBB and 16 - NB - -(-NBB // n) < 2:
            n += 1
        return n

    def is_w(N):
        for m in MODES:
            for c in (6, 16):
                p = plan(N, m, c)
                lv = p['levels']
                if len(lv) < 2 or lv[0][3] or lv[1][3] or lv[0][2] != narrow(p):
                    return False
        return True

    def is_3w(N):
        return all(any(ne > 0 and n == 3 and not deep for ne, _, n, deep in plan(N, 'default', c)['levels'])
                   for c in (6, 16))

    first = lambda ok: next(N for N in range(8, 20000) if ok(N))  # noqa: E731
    return first(is_w), first(is_3w), first(lambda N: plan(N, 'head', 6)['asm'] == 512)


@pytest.fixture(scope='module')
def sizes(ctx):
    nw, n3w, nasm = find_sizes(lambda N, m, c: _native.fte_debug_plan(N, _P(m), c, ctx=ctx))
    return {'N_W': nw, 'N_3W': n3w, 'N_ASM': nasm, 'N40': 40}


class Ref:
    """One problem and the oracle products the tests share (built once, never modified)."""

    def __init__(self, c, N):
        self.case, self.N = c, N
        self.seq, self.prob, self.cams = _problem(N, mode=c.mode, sd=c.sd, inter=c.inter, seed=c.seed,
                                                  sd_mode=c.sd_mode, n_cams=None if c.n_cams == 6 else c.n_cams)
        assert self.prob.C == c.n_cams
        self.table = pkin.build_table(c.mode)
        self.X0 = ofte.initial_state(self.prob, np.arange(N), self.seq.pos3d[:, 0, 0])
        if c.mode == 'default' and c.n_cams == 6:
            # initial_state leaves the lure at the world origin, which is camera 0 of the scene
            # file: the projection is singular there (NaN in the oracle too). Start the lure at
            # its mean true position instead.
            li = list(self.table.markers).index('lure')
            pi = okin.POSE[c.mode].index('x_l')
            self.X0[:, pi:pi + 3] = self.seq.pos3d[:, 0, li].mean(0)
            assert np.array_equal(okin.marker_positions(c.mode, self.X0[:1])[0, li], self.X0[0, pi:pi + 3])
        self.X0.setflags(write=False)
        # the start of the delays: 0 as the solve's default, or (tau cases) +-0.3 Ts alternating over
        # the cameras (camera 0 is pinned at 0). At tau = 0 every term a frame adds to the rows of its
        # two neighbours is exactly zero, so only these cases see the assembly's second-round entries
        # and the couplings between the X rows and the delays of the previous frames.
        self.tau0 = np.zeros(self.prob.tau_shape)
        if c.tau:
            assert c.sd and c.sd_mode == 'const'
            self.tau0 = 0.3 * self.prob.Ts * np.where(np.arange(c.n_cams) % 2, 1.0, -1.0)
            self.tau0[0] = 0.0
        self.tau0.setflags(write=False)
        self._lin = self._blocks = None
        self._lm = {}
        self._red = {}

    def lin(self):
        if self._lin is None:
            self._lin = self.prob.linearize(self.X0, self.tau0)
        return self._lin

    def lm(self, iters):
        if iters not in self._lm:
            self._lm[iters] = oracle_lm(self.prob, self.X0, self.tau0, iters, self.lin())
        return self._lm[iters]

    def blocks(self):
        """(D, E) of the oracle's damped X-X normal matrix: D[i] = block (i, i), E[i] = block
        (i, i - 1), 3-frame blocks padded to BP with the identity / zeros; and the half-width of
        the band, checked to be block tridiagonal."""
        if self._blocks is None:
            prob = self.prob
            P, M = prob.P, prob.M
            n = M * P
            H = self.lin()[1][:n, :n]
            dg = H.diagonal()
            A = (H + sp.diags(LAM * np.maximum(dg, 1e-12))).tocoo()
            nblk, BP = (M + 2) // 3, (3 * P + 15) // 16 * 16
            bi, bj = A.row // (3 * P), A.col // (3 * P)
            assert np.abs(bi - bj).max() <= 1, 'the oracle matrix is not block tridiagonal in 3-frame blocks'
            D = np.zeros((nblk, BP, BP))
            E = np.zeros((nblk, BP, BP))
            pad, last = np.arange(3 * P, BP), np.arange(n - 3 * P * (nblk - 1), BP)
            D[:, pad, pad] = 1.0               # rows past the block's frames: identity
            D[nblk - 1, last, last] = 1.0
            r, cc = A.row - bi * 3 * P, A.col - bj * 3 * P
            m = bi == bj
            np.add.at(D, (bi[m], r[m], cc[m]), A.data[m])
            m = bi == bj + 1
            np.add.at(E, (bi[m], r[m], cc[m]), A.data[m])
            D.setflags(write=False)
            E.setflags(write=False)
            self._blocks = (D, E)
        return self._blocks

    def reduced(self, L):
        if L not in self._red:
            D, E = self.blocks()
            self._red[L] = (schur_runs(D, E, L), schur_levels(D, E, L))
        return self._red[L]


def oracle_lm(prob, X0, tau0, iters, lin0=None):
    """`iters` iterations of oracle.fte._solve from (X0, tau0) at its default options, from the
    oracle's own functions. Returns X, tau, n_accepted, and the reference's floor: max |X - X'|,
    |tau - tau'| where X' takes every step one refinement further (long-double residual)."""
    from threadpoolctl import threadpool_limits
    out = []
    with threadpool_limits(1, user_api='blas'):
        for refine in (False, True):
            X = np.array(X0, np.float64)
            tau = np.array(tau0, np.float64)
            F, H, g = lin0 if lin0 is not None else prob.linearize(X, tau)
            lam, n_acc = 1e-3, 0
            pin0 = prob.pinned() if prob.sd else None
            for it in range(iters):
                gp, pin = g, pin0
                if pin0 is not None:
                    pin = np.concatenate([pin0, ofte.active_bounds(prob, tau, g)])
                    gp = g.copy()
                    gp[pin] = 0.0
                assert float(np.abs(gp).max()) > 1e-8, 'the oracle stops here (gtol) or is not finite'
                A = (H + sp.diags(lam * np.maximum(H.diagonal(), 1e-12))).tocsc()
                if pin is not None:
                    keep = np.ones(prob.nv)
                    keep[pin] = 0.0
                    A = (sp.diags(keep) @ A @ sp.diags(keep) + sp.diags(1.0 - keep)).tocsc()
                d = ofte._solve_step(prob, A, -gp)
                if refine:
                    co = A.tocoo()
                    r = gp.astype(np.longdouble)
                    np.add.at(r, co.row, co.data.astype(np.longdouble) * d.astype(np.longdouble)[co.col])
                    d = d - ofte._solve_step(prob, A, np.asarray(r, np.float64))
                dX, dtau = prob.unpack(d)
                Xn = X + dX
                taun = np.clip(tau + dtau, -prob.Ts, prob.Ts) if prob.sd else tau
                if prob.sd:
                    taun[..., 0] = 0.0
                Fn = prob.cost(Xn, taun)[0]
                if Fn < F:
                    n_acc += 1
                    X, tau = Xn, taun
                    lam = max(lam * 0.1, 1e-15)
                    if it + 1 < iters:
                        F, H, g = prob.linearize(X, tau)
                else:
                    lam *= 10.0
            out.append((X, tau, n_acc))
    (X, tau, n_acc), (Xr, taur, n_accr) = out
    assert n_acc == n_accr
    return X, tau, n_acc, float(np.abs(X - Xr).max()), float(np.abs(tau - taur).max())


def schur_runs(D, E, L):
    """Schur complement onto each block j = 2^L m of the block-tridiagonal (D, E): the runs of
    2^L - 1 blocks on either side of j, each eliminated as one dense solve. {j: block}."""
    nblk, BP = D.shape[:2]
    s = 1 << L

    def run(a, b):  # dense matrix of blocks a .. b
        k = b - a + 1
        R = np.zeros((k * BP, k * BP))
        for q in range(k):
            R[q * BP:(q + 1) * BP, q * BP:(q + 1) * BP] = D[a + q]
            if q:
                R[q * BP:(q + 1) * BP, (q - 1) * BP:q * BP] = E[a + q]
                R[(q - 1) * BP:q * BP, q * BP:(q + 1) * BP] = E[a + q].T
        return R

    out = {}
    for j in range(0, nblk, s):
        S = D[j].copy()
        if j > 0:  # left run j - s + 1 .. j - 1 couples through E_j = A[j, j - 1]
            k = s - 1
            C = np.zeros((k * BP, BP))
            C[(k - 1) * BP:] = E[j].T
            S -= C.T @ np.linalg.solve(run(j - s + 1, j - 1), C)
        b = min(j + s - 1, nblk - 1)
        if b > j:  # right run j + 1 .. b couples through E_{j+1} = A[j + 1, j]
            C = np.zeros(((b - j) * BP, BP))
            C[:BP] = E[j + 1]
            S -= C.T @ np.linalg.solve(run(j + 1, b), C)
        out[j] = S
    return out


def schur_levels(D, E, L):
    """The same by cyclic reduction, one level at a time, the eliminated blocks factored by
    Cholesky (schur_runs: LU), so that the two forms differ in arithmetic from level 1 on.
    {j: block}."""
    from scipy.linalg import cho_factor, cho_solve
    nblk = D.shape[0]
    D = {i: D[i].copy() for i in range(nblk)}
    E = {i: E[i].copy() for i in range(1, nblk)}  # E[i]: coupling of block i to the kept block below it
    s = 1
    for _ in range(L):
        for i in range(s, nblk, 2 * s):
            lo, hi = i - s, i + s
            cf = cho_factor(D[i])
            Wl = cho_solve(cf, E[i])  # D_i^-1 A[i, lo]
            D[lo] -= E[i].T @ Wl
            if hi < nblk:
                D[hi] -= E[hi] @ cho_solve(cf, E[hi].T)
                E[hi] = -E[hi] @ Wl
        s *= 2
    return {j: D[j] for j in range(0, nblk, s)}


def _scaled(B, ref):
    d = 1.0 / np.sqrt(np.diagonal(ref, axis1=-2, axis2=-1))
    return B * d[..., :, None] * d[..., None, :]


_REFS = {}


@pytest.fixture(scope='module')
def ref(sizes):
    def get(c):
        key = (c, sizes[c.size])
        if key not in _REFS:
            _REFS[key] = Ref(c, sizes[c.size])
        return _REFS[key]
    yield get
    _REFS.clear()


def _solve_gpu(ctx, R, iters):
    p, c = R.prob, R.case
    return ctx.fte_solve(R.table, R.cams, p.meas, p.w, p.Ts, p.qinv, R.X0, tau0=R.tau0, shutter_delay=c.sd,
                         intermode=p.im, sd_mode=c.sd_mode, opts=ctx.fte_default_opts(max_iters=iters))


def _assert_path(ctx, c, N):
    """The case runs the path its size is named for (fails if the dispatch moves)."""
    p = _plan(ctx, c, N)
    lv = p['levels']
    assert p['GR'] == (32 if c.sd and c.sd_mode == 'const' and c.n_cams > 15 else 16), p
    assert p['BP'] == {'head': 32, 'upper_body': 48, 'default_nolure': 80, 'default': 96}[c.mode], p
    assert p['Cg'] == (c.n_cams if c.sd and c.sd_mode == 'const' else 0), p
    if c.sd_mode == 'variable':
        assert p['asm'] == 0 and not p['d_upper'], p          # k_cr_build, the non-DUP instances
    else:
        assert p['d_upper'] == (p['GR'] == 16), p
    if c.size == 'N_W':
        assert not lv[0][3] and not lv[1][3] and lv[2][3] and p['asm'] in (0, 1024) and p['lin'] == 4, p
        assert lv[0][2] == (2 if p['BP'] == 96 or (p['GR'] == 32 and p['BP'] == 80) else 1) and lv[1][2] == 2, p
    elif c.size == 'N_3W':
        assert lv[0][2] == 3 and not lv[0][3] and lv[1][3] and p['asm'] == 1024, p
    elif c.size == 'N_ASM':
        assert p['asm'] == (0 if c.sd_mode == 'variable' else 512) and p['lin'] == 5, p
        assert not lv[0][3] and not lv[1][3] and not lv[2][3] and lv[3][3], p
    else:
        assert p['asm'] == 1024 and all(deep for _, _, _, deep in lv), p
    return p


STEP_CASES = [
    _case('N_W', 'head'), _case('N_W', 'head', 16), _case('N_W', 'upper_body'), _case('N_W', 'upper_body', 16),
    _case('N_W', 'default_nolure', 16), _case('N_W', 'default'), _case('N_W', 'default', 16),
    _case('N_W', 'head', sd_mode='variable'), _case('N_W', 'default_nolure', sd_mode='variable'),
    _case('N_W', 'default_nolure', sd=False), _case('N_W', 'upper_body', inter='acc'),
    _case('N_3W', 'default'), _case('N_3W', 'default', 16),
    _case('N_ASM', 'head'), _case('N_ASM', 'head', 16), _case('N_ASM', 'upper_body', 16),
    _case('N_ASM', 'default_nolure', sd=False), _case('N_ASM', 'default'),
    # from nonzero delays (Ref.tau0)
    _case('N_ASM', 'head', 16, tau=True), _case('N_ASM', 'default', tau=True), _case('N40', 'default', 16, tau=True),
]
STEP3_CASES = [_case('N_ASM', 'default_nolure'), _case('N_ASM', 'head', 16)]


def _check_steps(ctx, sizes, ref, c, iters):
    _assert_path(ctx, c, sizes[c.size])
    R = ref(c)
    Xo, to, n_acc, fx, ft = R.lm(iters)
    # a rejected step leaves X = X0 and checks nothing
    assert n_acc == iters, f'the oracle rejected a step of {_id(c)}: pick another seed'
    X, tau, rep = _solve_gpu(ctx, R, iters)
    tol_x = max(1e-9, 10.0 * fx)
    tol_t = max(1e-11 if c.sd_mode == 'variable' else 1e-12, 10.0 * ft)
    ex = float(np.abs((X - R.X0) - (Xo - R.X0)).max())
    et = float(np.abs(tau - to).max())
    print(f'FTE-WIDE step {_id(c)} x{iters} N={R.N}: floor X {fx:.1e} tau {ft:.1e}  tol X {tol_x:.1e} tau '
          f'{tol_t:.1e}  GPU err X {ex:.2e} tau {et:.2e}  max|dX| {np.abs(Xo - R.X0).max():.2e}')
    assert rep['n_bad_pivots'] == 0 and rep['iters'] == iters, rep
    assert rep['n_accepted'] == n_acc, rep
    assert tau.shape == to.shape
    np.testing.assert_allclose(X - R.X0, Xo - R.X0, rtol=0, atol=tol_x)
    np.testing.assert_allclose(tau, to, rtol=0, atol=tol_t)


@pytest.mark.parametrize('c', STEP_CASES, ids=_id)
def test_fte_wide_single_lm_step_matches_oracle(ctx, sizes, ref, c):
    _check_steps(ctx, sizes, ref, c, 1)


@pytest.mark.parametrize('c', STEP3_CASES, ids=_id)
def test_fte_wide_three_lm_steps_match_oracle(ctx, sizes, ref, c):
    """k_fte_linearize<5> at the trial state, the buffer flip, and re-assembly through the compact
    rows: three accepted iterations on both sides."""
    _check_steps(ctx, sizes, ref, c, 3)


ASM_CASES = [_case('N_ASM', m, n) for m in MODES for n in (6, 16)] + [_case('N_ASM', 'default_nolure', sd=False),
                                                                      _case('N40', 'default', 16)]
ASM_CASES += [_case('N_ASM', 'head', 16, tau=True), _case('N_ASM', 'default', tau=True),
              _case('N40', 'default', 16, tau=True)]


def _gpu_blocks(ctx, R, levels):
    p, c = R.prob, R.case
    return ctx.fte_debug_blocks(R.table, R.cams, p.meas, p.w, p.Ts, p.qinv, R.X0, R.tau0, lam=LAM,
                                levels=levels, shutter_delay=c.sd, intermode=p.im)


@pytest.mark.parametrize('c', ASM_CASES, ids=_id)
def test_fte_wide_assembled_damped_blocks_match_oracle(ctx, sizes, ref, c):
    _assert_path(ctx, c, sizes[c.size])
    R = ref(c)
    Dr, _ = R.blocks()
    D, L = _gpu_blocks(ctx, R, 0)
    assert L == 0 and D.shape == Dr.shape and np.isfinite(D).all()
    bad = np.nonzero((D != np.swapaxes(D, 1, 2)).any((1, 2)))[0]
    assert len(bad) == 0, f'{len(bad)} of {len(D)} assembled blocks not bitwise symmetric, first {bad[:5]}'
    # outside the frames' entries (where the reference holds the identity): exactly the identity
    valid = np.zeros(D.shape, bool)
    n3 = 3 * R.prob.P
    valid[:, :n3, :n3] = True
    last = R.prob.M * R.prob.P - n3 * (len(D) - 1)
    valid[-1] = False
    valid[-1, :last, :last] = True
    ib = np.nonzero(((D != Dr) & ~valid).any((1, 2)))[0]
    assert len(ib) == 0, f'padding of blocks {ib[:5]} is not the identity'
    err = np.abs(_scaled(D, Dr) - _scaled(Dr, Dr)).max((1, 2))
    print(f'FTE-WIDE asm {_id(c)} N={R.N}: max scaled err {err.max():.2e} (block {int(err.argmax())})')
    assert err.max() <= 1e-8, f'block {int(err.argmax())}: scaled error {err.max():.3e}'


RED_CASES = [_case('N_W', m, n) for m in MODES for n in (6, 16)] + [_case('N_3W', 'default'),
                                                                    _case('N_3W', 'default', 16)]


@pytest.mark.parametrize('L', [1, 2, 3])
@pytest.mark.parametrize('c', RED_CASES, ids=_id)
def test_fte_wide_reduced_blocks_match_schur_complement(ctx, sizes, ref, c, L):
    p = _assert_path(ctx, c, sizes[c.size])
    R = ref(c)
    Sa, Sb = R.reduced(L)
    D, Lrun = _gpu_blocks(ctx, R, L)
    assert Lrun == L
    js = sorted(Sa)
    assert js == list(range(0, p['nblk'], 1 << L))
    A = np.stack([Sa[j] for j in js])
    B = np.stack([Sb[j] for j in js])
    G = D[js]
    two = float(np.abs(_scaled(A, A) - _scaled(B, A)).max())
    err = np.abs(_scaled(G, A) - _scaled(A, A)).max((1, 2))
    k = int(err.argmax())
    print(f'FTE-WIDE red {_id(c)} L={L} N={R.N}: two-form {two:.2e}  GPU err {err.max():.2e} (block {js[k]})  '
          f'ratio {err.max() / two:.1f}')
    assert np.isfinite(G).all()
    assert err.max() <= 1000.0 * two, (f'level {L}, block {js[k]}: scaled error {err.max():.3e} against '
                                       f'{two:.3e} between the two reference forms')
