"""The problems of the extrinsics-SBA shape tests (test_sba_ext_shapes_cpu.py, test_gpu_sba_ext_shapes.py)
and the rules they are chosen by. numpy, synth.ring_scene and the oracle only: no GPU, no library.

acs_sba_extrinsics selects its code by K, the largest number of observations of one point: the
lane group G = K rounded up to 2, 4, ..., 64 (k_ext_linearize<G>, k_ext_cost<G>), and the points per
Schur block chunk = max(1, min(64, 96 KiB / (148 K + 24))) (plan() is the Python form of ext_dims).

problem(): the generator of tools/sba_ext_bitcheck.py (ext_problem): a ring of C cameras, point 0 with
K observations, point n - 2 with one, point n - 1 with none, the others 2..K; a point with more than C
observations repeats cameras (ext_schur_entry then sums several slots of one camera); shuffled
observation order, 0.5 px noise, translations of cameras 1.. and the points perturbed by 5 mm. The
seed is 100 + K, but for the one-camera problem (test_sba_ext_shapes_cpu.py says why).

SHAPES: (C, K, n) -> G, chunk, number of chunks, size of the last chunk. Every lane group but 8 and 16
(the golden problem and the rings of test_gpu_sba_ext.py have those), K at a power of two (2, 4, 64) and
just above one (3, 17, 33), K above C (4 > 3, 17..64 > 16), K = EXT_MAXK, one camera, one chunk and
several with a ragged last one.

Which runs may be compared with the GPU at rounding-level tolerances is decided on the oracle alone
(test_sba_ext_shapes_cpu.py): a fixed-iteration run needs every accept / reject decision far from a
tie; a run to convergence needs, besides, a stop that does not sit on its threshold. choose_stop()
picks the tolerance of such a run from the trace of a run without tolerances: the geometric mean of
two consecutive values of the deciding quantity that are at least 10x apart, so the stop is more than
3x off its threshold on both sides. STOPS records what it chose (the CPU test recomputes it).
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import sba_ext as oext

EXT_MAXK = 64
FIXED_ITERS = 8

Shape = namedtuple('Shape', 'C K n G chunk nchunk last seed')
SHAPES = [
    Shape(1, 1, 30, 2, 64, 1, 30, 106),  # not seed 101, n = 20: see test_sba_ext_shapes_cpu.py on the costs
    Shape(2, 2, 70, 2, 64, 2, 6, 102),
    Shape(3, 3, 70, 4, 64, 2, 6, 103),
    Shape(3, 4, 70, 4, 64, 2, 6, 104),
    Shape(16, 17, 70, 32, 38, 2, 32, 117),
    Shape(16, 20, 70, 32, 32, 3, 6, 120),
    Shape(16, 33, 40, 64, 20, 2, 20, 133),
    Shape(16, 40, 70, 64, 16, 5, 6, 140),
    Shape(16, 64, 24, 64, 10, 3, 4, 164),
]
SMALL, LARGE = SHAPES[1], SHAPES[8]  # the smallest and the largest lane group (stops, convergence)
DIST_SHAPES = [SHAPES[1], SHAPES[7]]


def shape_id(s):
    return f'C{s.C}-K{s.K}-n{s.n}'


def seed_of(s):
    return s.seed  # 100 + K but for the one-camera problem


def plan(n, K):
    """ext_dims / ext_nchunk (csrc/sba_ext.hpp) in Python: G, chunk, number of chunks."""
    G = 2
    while G < K:
        G *= 2
    chunk = max(1, min(64, (96 * 1024) // (148 * K + 24)))
    return dict(G=G, chunk=chunk, nchunk=(n + chunk - 1) // chunk)


Problem = namedtuple('Problem', 'K D R0 t0 uv pi ci X0')


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def make_problem(C, K, n, seed):
    from acinoset_amd import synth
    rng = np.random.default_rng(seed)
    sc = synth.ring_scene(C)
    X = rng.uniform(-2, 2, (n, 3)) * [1, 1, 0.3] + [1.9, 6.4, 0.5]
    sizes = rng.integers(min(2, K), K + 1, n)  # K = 1: every point but the last has one observation
    sizes[0], sizes[n - 2], sizes[n - 1] = K, 1, 0
    pi = np.repeat(np.arange(n), sizes).astype(np.int32)
    ci = np.concatenate([np.concatenate([rng.permutation(C)[:min(s, C)], rng.integers(0, C, max(s - C, 0))])
                         for s in sizes]).astype(np.int32)
    order = rng.permutation(len(pi))
    pi, ci = pi[order], ci[order]
    Kc, D, R = np.array(sc.K, np.float64), np.array(sc.D, np.float64).reshape(-1, 4), np.array(sc.R, np.float64)
    t = np.array(sc.t, np.float64).reshape(-1, 3)
    uv = oext.residuals(X, R, t, Kc, D, np.zeros((len(pi), 2)), pi, ci)  # the projection itself
    uv = uv + rng.normal(0, 0.5, uv.shape)
    t0 = t + rng.normal(0, 5e-3, (C, 3)) * (np.arange(C) > 0)[:, None]
    X0 = X + rng.normal(0, 5e-3, X.shape)
    return Problem(*_frozen(Kc, D, R, t0, uv, pi, ci, X0))


@functools.lru_cache(maxsize=None)
def problem(s):
    return make_problem(s.C, s.K, s.n, seed_of(s))


@functools.lru_cache(maxsize=None)
def probe_problem(s):
    """The ulp probe: every pixel coordinate moved to a neighbouring double, up or down at random."""
    p = problem(s)
    up = np.random.default_rng(7000 + seed_of(s)).random(p.uv.shape) < 0.5
    uv = np.where(up, np.nextafter(p.uv, np.inf), np.nextafter(p.uv, -np.inf))
    return p._replace(uv=_frozen(uv)[0])


Run = namedtuple('Run', 'X R t info trace')


def oracle(p, **kw):
    trace = []
    X, R, t, info = oext.sba_extrinsics(p.uv, p.X0, p.pi.astype(np.int64), p.ci.astype(np.int64), p.K, p.D, p.R0,
                                        p.t0, trace=trace, **kw)
    return Run(*_frozen(X, R, t), info, trace)


@functools.lru_cache(maxsize=None)
def _run(s, probe, opts):
    return oracle(probe_problem(s) if probe else problem(s), **dict(opts))


def run(s, probe=False, **opts):
    """The oracle's solve of shape s (of its ulp probe), computed once per set of options."""
    return _run(s, probe, tuple(sorted(opts.items())))


def residuals(p, r):
    return oext.residuals(r.X, r.R, r.t, p.K, p.D, p.uv, p.pi, p.ci).ravel()


# ---- the trace ---------------------------------------------------------------------------
def margin(e):
    """How far a decision is from a tie: |F - F_new| / F."""
    return abs(e['F'] - e['F_new']) / e['F']


def decrease(e):
    return (e['F'] - e['F_new']) / abs(e['F'])


def xratio(e, xtol):
    """The xtol test reads dn <= xtol (xtol + xn): dn / (xtol + xn) against xtol."""
    return e['dn'] / (xtol + e['xn'])


# ---- the stop tolerance of a run to convergence ------------------------------------------
Stop = namedtuple('Stop', 'kind tol above below iters')  # above > tol > below bracket it; iters: where it stops
FREE = dict(ftol=0.0, xtol=0.0, gtol=0.0)  # no stop but max_iters and lam > 1e16
TIE = 1e-9       # every decision before the stop is at least this far from a tie
MIN_DECREASE = 1e-11  # ... and the accepted step that stops an ftol / xtol run this far


def choose_stop(trace, kind):
    """The stop tolerance `kind` ('ftol', 'xtol', 'gtol') from the trace of a run with the options FREE:
    the geometric mean of two consecutive values of the deciding quantity, the later one at least
    10x smaller, such that no earlier value is within 3x of the tolerance, every decision before the
    stop is TIE from a tie, and an ftol / xtol stop is an accepted step with a relative decrease of
    MIN_DECREASE or more. ftol, xtol: the quantity is the relative decrease, the step norm over the
    state norm, of the accepted steps; gtol: gmax of every iteration (it is tested before the step).
    The last admissible pair of the trace; None when there is none (change the seed or n)."""
    if kind == 'gtol':
        idx = list(range(len(trace)))
        q = [e['gmax'] for e in trace]
    else:
        idx = [i for i, e in enumerate(trace) if e['accepted']]
        q = [decrease(trace[i]) if kind == 'ftol' else trace[i]['dn'] / trace[i]['xn'] for i in idx]
    for k in range(len(q) - 2, -1, -1):
        above, below = q[k], q[k + 1]
        if not (below > 0 and above >= 10 * below):
            continue
        tol = float(np.sqrt(above * below))
        stop_at = idx[k + 1]  # ftol / xtol: the iteration whose step stops; gtol: the one that is not run
        n_dec = stop_at if kind == 'gtol' else stop_at + 1
        if any(v < 3 * tol for v in q[:k + 1]):
            continue
        if any(margin(e) < TIE for e in trace[:stop_at]):
            continue
        if kind != 'gtol' and decrease(trace[stop_at]) < MIN_DECREASE:
            continue
        return Stop(kind, tol, above, below, n_dec)
    return None


def stop_opts(stop, max_iters=200):
    return dict(FREE, max_iters=max_iters, **{stop.kind: stop.tol})


# What choose_stop gave for the runs to convergence of the GPU test (test_sba_ext_shapes_cpu.py holds
# the rule to them): (shape, kind) -> (tolerance, the value above, the value below, iterations).
STOPS = {
    (SMALL, 'ftol'): Stop('ftol', 1.11e-9, 3.68e-9, 3.37e-10, 38),
    (SMALL, 'xtol'): Stop('xtol', 1.77e-6, 6.26e-6, 5.03e-7, 35),
    (SMALL, 'gtol'): Stop('gtol', 14.2, 48.5, 4.16, 33),
    (LARGE, 'ftol'): Stop('ftol', 3.43e-10, 5.12e-9, 2.30e-11, 46),
    (LARGE, 'xtol'): Stop('xtol', 3.35e-8, 1.67e-7, 6.69e-9, 46),
    (LARGE, 'gtol'): Stop('gtol', 0.388, 1.33, 0.113, 45),
}
FREE_ITERS = 48  # iterations of the run without tolerances that choose_stop reads: past every stop above
