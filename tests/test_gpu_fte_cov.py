"""GPU: acs_fte_covariance (the per-frame pose, shutter-delay and marker covariances of the FTE
estimate) against the dense inverse of the GPU's own acs_fte_eval normal matrix.

Reference: np.linalg.inv of the kept rows and columns of H (held delays removed).
Measure: for a block S against the reference block R, max |S - R| / sqrt(diag R x diag R).
Bound: 10 cond(H_kept) 2.2e-16, cond from eigvalsh: the error of a float64 inverse of a matrix
of that condition number (two dense float64 inverses of these problems differ by ~4e-9 at
cond ~5e7). Every case first asserts that H_kept is positive definite.
Inputs as tests/test_gpu_fte.py::_problem: seed 2, X = truth with two leading copies of frame 0
+ default_rng(4).normal(0, 0.002), tau = [0, U(-0.003, 0.003) ...]."""
import functools
import importlib

import numpy as np
import pytest

from oracle import fte as ofte
from acinoset_amd import _native, kinematics as pkin
from test_gpu_fte import _problem

pytestmark = pytest.mark.gpu
cfte = importlib.import_module('acinoset_amd.core.fte')   # `core.fte` the attribute is the driver function

EPS = 2.2e-16

CASES = [
    # N, mode, shutter delay, intermode, cameras
    (3, 'default_nolure', True, 'vel', 6),     # 2 blocks, eliminated block without right neighbour
    (5, 'default_nolure', False, 'pos', 6),    # 3 blocks, no border
    (8, 'default_nolure', True, 'acc', 6),     # 4 blocks, last block one real frame
    (11, 'default', True, 'vel', 6),           # BP = 96, 5 blocks
    (14, 'upper_body', True, 'vel', 6),        # BP = 48
    (10, 'head', True, 'acc', 6),              # BP = 32
    (25, 'default_nolure', True, 'acc', 6),    # 9 = 2^3 + 1 blocks
    (49, 'default_nolure', True, 'vel', 6),    # 17 blocks
    (8, 'default_nolure', True, 'vel', 16),    # full border
    (8, 'default_nolure', True, 'vel', 2),     # cond ~ 2e9
]


@functools.lru_cache(maxsize=None)
def _inputs(N, mode, sd, inter, n_cams, tau_set=(), zero_frames=(), tau_max=0.004):
    seq, prob, cams = _problem(N, mode=mode, sd=sd, inter=inter, n_cams=None if n_cams == 6 else n_cams,
                               tau_max=tau_max)
    rng = np.random.default_rng(4)
    X = np.concatenate([seq.x[:1], seq.x[:1], seq.x], 0) + rng.normal(0, 0.002, (prob.M, prob.P))
    tau = np.zeros(prob.C)
    if sd:
        tau[1:] = rng.uniform(-0.003, 0.003, prob.C - 1)
    for c, sign in (() if tau_set == 'clip' else tau_set):
        tau[c] = sign * prob.Ts
    if tau_set == 'clip':   # the true delays, those beyond a bound put on it
        tau = np.clip(seq.tau, -prob.Ts, prob.Ts)
    w = prob.w.copy()
    for f in zero_frames:
        w[f] = 0.0
    for a in (X, tau, w):
        a.setflags(write=False)
    return seq, prob, cams, pkin.build_table(mode), X, tau, w


def _held(prob, tau, g):
    """tau_held of the LM step: camera 0, or a delay on a bound whose descent direction points out."""
    gt = g[prob.M * prob.P:]
    return np.array([c == 0 or (tau[c] >= prob.Ts and gt[c] < 0) or (tau[c] <= -prob.Ts and gt[c] > 0)
                     for c in range(prob.C)])


@functools.lru_cache(maxsize=None)
def _case(ctx, key):
    """GPU covariance and the dense reference of one case (computed once, shared, read-only)."""
    seq, prob, cams, table, X, tau, w = _inputs(*key)
    sd = prob.sd
    _, g, H = ctx.fte_eval(table, cams, prob.meas, w, prob.Ts, prob.qinv, X, tau, shutter_delay=sd,
                           intermode=prob.im)
    nx = prob.M * prob.P
    held = _held(prob, tau, g) if sd else np.ones(prob.C, bool)
    free = np.flatnonzero(~held)
    keep = np.concatenate([np.arange(nx), nx + free]) if sd else np.arange(nx)
    Hk = H[np.ix_(keep, keep)]
    ev = np.linalg.eigvalsh(Hk)
    ref = np.linalg.inv(Hk) if ev.min() > 0 else None
    cov = ctx.fte_covariance(table, cams, prob.meas, w, prob.Ts, prob.qinv, X, tau, shutter_delay=sd,
                             intermode=prob.im, markers=True)
    return dict(prob=prob, table=table, X=X, tau=tau, cov=cov, ev=ev, ref=ref, held=held, free=free,
                cond=ev.max() / ev.min(), bound=10 * (ev.max() / ev.min()) * EPS)


def _scaled_err(S, R):
    d = np.sqrt(np.diag(R))
    return float(np.max(np.abs(S - R) / np.outer(d, d)))


def _check_against_dense(c, label):
    prob, cov, R = c['prob'], c['cov'], c['ref']
    assert c['ev'].min() > 0, (label, c['ev'].min())
    M, P, nx = prob.M, prob.P, prob.M * prob.P
    xc, tc = cov['x_cov'], cov['tau_cov']
    assert xc.shape == (M, P, P) and np.isfinite(xc).all() and int(np.isfinite(xc).sum()) == M * P * P
    assert tc.shape == (prob.C, prob.C) and np.isfinite(tc).all()
    assert cov['n_bad_pivots'] == 0
    err_x = max(_scaled_err(xc[f], R[f * P:(f + 1) * P, f * P:(f + 1) * P]) for f in range(M))
    free, held = c['free'], c['held']
    err_t = 0.0
    if prob.sd and len(free):
        err_t = _scaled_err(tc[np.ix_(free, free)], R[nx:, nx:])
    print(f'{label}: cond {c["cond"]:.2e} bound {c["bound"]:.2e} err cov_x {err_x:.2e} cov_tau {err_t:.2e}')
    assert err_x < c['bound'], (label, err_x, c['bound'])
    assert err_t < c['bound'], (label, err_t, c['bound'])
    # held rows and columns are zero; every block symmetric; variances positive
    assert not tc[held].any() and not tc[:, held].any()
    assert cov['n_tau_free'] == (len(free) if prob.sd else 0)
    for f in range(M):
        assert np.abs(xc[f] - xc[f].T).max() <= 1e-13 * np.abs(xc[f]).max()
        assert (np.diag(xc[f]) > 0).all()
    assert np.abs(tc - tc.T).max() <= 1e-13 * max(np.abs(tc).max(), 1e-300)
    assert (np.diag(tc)[free] > 0).all() if prob.sd else True
    d = np.concatenate([np.diag(xc[f]) for f in range(2, M)])
    assert cov['var_min'] == d.min() and cov['var_max'] == d.max()


@pytest.mark.parametrize('N,mode,sd,inter,n_cams', CASES)
def test_cov_matches_dense_inverse(ctx, N, mode, sd, inter, n_cams):
    c = _case(ctx, (N, mode, sd, inter, n_cams))
    _check_against_dense(c, f'N={N} {mode} sd={sd} {inter} C={n_cams}')
    mc = c['cov']['marker_cov']
    assert mc.shape == (N, c['table'].L, 3, 3) and np.isfinite(mc).all()
    assert np.abs(mc - mc.transpose(0, 1, 3, 2)).max() <= 1e-13 * np.abs(mc).max()
    assert (np.diagonal(mc, axis1=2, axis2=3) > 0).all()


def test_held_delays_are_constants(ctx):
    """Delays on a bound with the descent direction pointing out are held: zero rows and columns in
    cov_tau, the rest is the inverse without them."""
    c = _case(ctx, (8, 'default_nolure', True, 'vel', 6, ((2, 1.0), (3, -1.0))))
    assert c['held'][0]
    _check_against_dense(c, 'held delays')
    assert c['cov']['n_tau_free'] == len(c['free'])


def test_delays_beyond_the_bound_are_held(ctx):
    """True delays up to 0.03 s with the bound Ts = 0.011 s: the delays whose truth lies beyond a
    bound sit on it with the descent direction pointing out (cameras 3 and 5 at this seed, by the
    oracle's gradient), so this case has held delays besides camera 0."""
    c = _case(ctx, (8, 'default_nolure', True, 'vel', 6, 'clip', (), 0.03))
    assert c['held'].sum() >= 2 and not c['held'].all(), c['held']
    _check_against_dense(c, 'delays on the bound')
    assert c['cov']['n_tau_free'] == len(c['free']) == int((~c['held']).sum())


def test_unobserved_frames_widen_the_estimate(ctx):
    key = (11, 'default_nolure', True, 'vel', 6)
    full = _case(ctx, key)
    gap = _case(ctx, key + ((), (4, 5)))
    _check_against_dense(gap, 'frames 4, 5 unobserved')
    d0 = np.stack([np.diag(b) for b in full['cov']['x_cov']])
    d1 = np.stack([np.diag(b) for b in gap['cov']['x_cov']])
    bound = max(full['bound'], gap['bound'])
    assert (d1 >= d0 - bound * np.maximum(d0, d1)).all()


def test_marker_cov_is_J_S_Jt(ctx):
    c = _case(ctx, (11, 'default', True, 'vel', 6))
    _, J = ctx.fk(c['table'], c['X'][2:], jac=True)
    ref = np.einsum('nlap,npq,nlbq->nlab', J, c['cov']['x_cov'][2:], J)
    mc = c['cov']['marker_cov']
    assert np.abs(mc - ref).max() <= 1e-12 * np.abs(ref).max()


def test_cov_deterministic_and_allocation_free(ctx):
    seq, prob, cams, table, X, tau, w = _inputs(25, 'default_nolure', True, 'acc', 6)
    args = (table, cams, prob.meas, w, prob.Ts, prob.qinv, X, tau)
    kw = dict(shutter_delay=True, intermode=prob.im, markers=True)
    a = ctx.fte_covariance(*args, **kw)
    ev = _native.alloc_events()
    b = ctx.fte_covariance(*args, **kw)
    assert _native.alloc_events() == ev
    for k in ('x_cov', 'tau_cov', 'marker_cov'):
        assert np.array_equal(a[k], b[k]), k
    assert all(a[k] == b[k] for k in ('n_bad_pivots', 'n_tau_free', 'var_min', 'var_max'))


def test_cov_through_the_solve(ctx):
    N, mode = 30, 'default_nolure'
    seq, prob, cams = _problem(N)
    from acinoset_amd import synth
    scene = synth.load_scene_file()
    X0 = ofte.initial_state(prob, np.arange(N), seq.pos3d[:, 0, 0])
    cp = (scene.K, scene.D, scene.R, scene.t)
    fps = 1.0 / seq.Ts
    X, tau, rep = cfte.solve(prob.meas, prob.w, cp, mode, fps, X0, ctx=ctx, covariance=True)
    X2, tau2, rep2 = cfte.solve(prob.meas, prob.w, cp, mode, fps, X0, ctx=ctx)
    assert np.array_equal(X, X2) and np.array_equal(tau, tau2)
    assert not any(k in rep2 for k in ('x_cov', 'tau_cov', 'marker_cov', 'cov_bad_pivots'))
    assert {k: v for k, v in rep.items() if k in rep2} == rep2
    cov = ctx.fte_covariance(pkin.build_table(mode), cams, prob.meas, prob.w, 1.0 / float(fps),
                             cfte.model_weights(mode), X, tau, shutter_delay=True, intermode=1, markers=True)
    assert np.array_equal(rep['x_cov'], cov['x_cov'])
    assert np.array_equal(rep['tau_cov'], cov['tau_cov'])
    assert np.array_equal(rep['marker_cov'], cov['marker_cov'])
    assert rep['cov_bad_pivots'] == 0 and rep['x_cov'].shape == (N + 2, prob.P, prob.P)


def test_cov_rejects_variable_delays(ctx):
    seq, prob, cams, table, X, tau, w = _inputs(8, 'default_nolure', True, 'vel', 6)
    with pytest.raises(RuntimeError, match='variable'):
        ctx.fte_covariance(table, cams, prob.meas, w, prob.Ts, prob.qinv, X, shutter_delay=True, intermode=1,
                           sd_mode='variable')


def test_core_fte_writes_the_covariances(ctx, tmp_path):
    """core.fte(covariance=True): fte.pickle gains x_cov (N, P, P), shutter_delay_cov (C, C) and
    positions_cov (N, L, 3, 3), consistent with each other; the default pickle has none of them and
    the same solution."""
    import json
    import pickle
    from acinoset_amd import core, synth
    scene = synth.load_scene_file()
    N, mode = 12, 'head'
    seq = synth.make_sequence(N, scene, mode=mode, seed=13, tau_max=0.003)
    cp = scene.camera_params()
    st = {}
    for name, kw in (('plain', {}), ('cov', dict(covariance=True))):
        out = core.fte(str(tmp_path / name), seq.to_df(), mode, cp, 0, N - 1, 0.5, 'scene.json',
                       params={'vid_fps': 90.0}, shutter_delay=True, interpolation_mode='vel', video=False, **kw)
        with open(out, 'rb') as f:
            st[name] = pickle.load(f)
    new = {'x_cov', 'shutter_delay_cov', 'positions_cov'}
    assert not new & set(st['plain']) and set(st['cov']) == set(st['plain']) | new
    assert st['cov']['x'] == st['plain']['x'] and st['cov']['shutter_delay'] == st['plain']['shutter_delay']
    table = pkin.build_table(mode)
    xc, tc, pc = (st['cov'][k] for k in ('x_cov', 'shutter_delay_cov', 'positions_cov'))
    assert xc.shape == (N, table.P, table.P) and tc.shape == (6, 6) and pc.shape == (N, table.L, 3, 3)
    assert (np.diagonal(xc, axis1=1, axis2=2) > 0).all() and not tc[0].any() and (np.diag(tc)[1:] > 0).all()
    _, J = ctx.fk(table, np.asarray(st['cov']['x']), jac=True)
    ref = np.einsum('nlap,npq,nlbq->nlab', J, xc, J)
    assert np.abs(pc - ref).max() <= 1e-12 * np.abs(ref).max()
    with open(tmp_path / 'cov' / 'solver_report.json') as f:
        assert json.load(f)['cov_bad_pivots'] == 0
    with pytest.raises(ValueError, match='variable'):
        core.fte(str(tmp_path / 'var'), seq.to_df(), mode, cp, 0, N - 1, 0.5, 'scene.json',
                 params={'vid_fps': 90.0}, shutter_delay=True, shutter_delay_mode='variable',
                 interpolation_mode='vel', video=False, covariance=True)
