"""Time of one extrinsics-SBA covariance call (acs_sba_extrinsics_covariance) beside one LM
iteration of the solve (acs_sba_extrinsics) of the same shape in the same session, device-resident:
the sba_extrinsics golden shape (6 cameras, 80 points), C = 16 / n = 400 and a board-sized shape of
6 cameras x 20,000 points.

Both calls take device pointers and wait for the stream themselves, so each is timed on its own
with a pair of device events on the one stream that carries the context's kernels, after one
untimed call that sizes the workspace. One run each (recorded, not a target). The yardstick is the
solve's time divided by the iterations its report gives. No oracle, no reference reads: it only
times. The table goes to --out as JSON (one record per shape) and to stdout.

    python tools/time_sba_ext_cov.py [--cov-calls 30] [--out profiles/r15/sba_ext_cov_time.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from acinoset_amd import _native, synth  # noqa: E402
from oracle import sba_ext as oext  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden', 'sba_extrinsics.npz')


def ring_problem(n_pts, n_cams, seed=7, noise=0.5):
    """A ring of cameras, points in a slab each seen by 2..C cameras, noisy observations and a
    perturbed start (the generator of the extrinsics SBA's tests)."""
    rng = np.random.default_rng(seed)
    sc = synth.ring_scene(n_cams)
    X = rng.uniform(-2, 2, (n_pts, 3)) * [1, 1, 0.3] + [1.9, 6.4, 0.5]
    sizes = rng.integers(2, n_cams + 1, n_pts)
    pi = np.repeat(np.arange(n_pts), sizes).astype(np.int32)
    ci = np.concatenate([rng.choice(n_cams, size=s, replace=False) for s in sizes]).astype(np.int32)
    t = sc.t.reshape(-1, 3)
    uv = oext.residuals(X, sc.R, t, sc.K, sc.D.reshape(-1, 4), np.zeros((len(pi), 2)), pi, ci)
    uv = uv + rng.normal(0, noise, uv.shape)
    R0, t0 = sc.R.copy(), t.copy()
    for c in range(1, n_cams):
        R0[c] = oext.rodrigues(rng.normal(0, 2e-3, 3)) @ R0[c]
        t0[c] += rng.normal(0, 5e-3, 3)
    return _native.pack_cameras(sc.K, sc.D, R0, t0), uv, pi, ci, X + rng.normal(0, 5e-3, X.shape)


def _timed(dev, fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize(dev)
    return s.elapsed_time(e), out


def time_case(ctx, dev, name, cams, uv, pi, ci, X0, max_iters, cov_calls=1):
    T = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)  # noqa: E731
    n, nc, m = len(X0), len(cams), len(pi)
    d_uv, d_pi, d_ci = T(uv, np.float64), T(pi, np.int32), T(ci, np.int32)
    d_cams0, d_pts0 = T(cams, np.float64), T(X0, np.float64)
    d_cc = torch.empty((6 * nc, 6 * nc), dtype=torch.float64, device=dev)
    d_cp = torch.empty((n, 3, 3), dtype=torch.float64, device=dev)
    d_st = torch.empty(n, dtype=torch.int32, device=dev)
    v = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    flags = _native.ACS_DEVICE_PTRS
    sopts = ctx.sba_ext_opts(max_iters=max_iters)
    srep = _native.SbaExtReport()
    copts = _native.SbaExtCovOpts(_native.GAUGES['anchor'], 0, nc // 2, 0, 1.0, 1.0)
    crep = _native.SbaExtCovReport()

    def solve():
        d_cams, d_pts = d_cams0.clone(), d_pts0.clone()
        torch.cuda.synchronize(dev)

        def call():
            ctx.check(ctx.lib.acs_sba_extrinsics(ctx.h, v(d_cams), nc, v(d_uv), v(d_pi), v(d_ci), m, v(d_pts), n,
                                                 C.byref(sopts), None, None, C.byref(srep), flags), 'acs_sba_extrinsics')
        ms, _ = _timed(dev, call)
        return ms, d_cams, d_pts

    def cov(d_cams, d_pts):
        def call():
            ctx.check(ctx.lib.acs_sba_extrinsics_covariance(ctx.h, v(d_cams), nc, v(d_uv), v(d_pi), v(d_ci), m,
                                                            v(d_pts), n, C.byref(copts), v(d_cc), v(d_cp), v(d_st),
                                                            C.byref(crep), flags), 'acs_sba_extrinsics_covariance')
        return _timed(dev, call)[0]

    _, d_cams, d_pts = solve()       # sizes the workspace
    cov(d_cams, d_pts)
    before = _native.alloc_events()
    solve_ms, d_cams, d_pts = solve()
    cov_ms = cov(d_cams, d_pts)
    iters = max(int(srep.iters), 1)
    rec = dict(shape=name, n_cams=nc, n_pts=n, n_obs=m, solve_ms=round(solve_ms, 4), solve_iters=int(srep.iters),
               solve_status=srep.as_dict()['status_name'], lm_iteration_ms=round(solve_ms / iters, 5),
               cov_ms=round(cov_ms, 4), cov_over_lm_iteration=round(cov_ms / (solve_ms / iters), 3),
               alloc_events_in_timed_calls=_native.alloc_events() - before, cov_report=crep.as_dict())
    if cov_calls > 1:  # one call is at the mercy of a single stall: the spread of repeats in one process
        ts = sorted(cov(d_cams, d_pts) for _ in range(cov_calls))
        rec['cov_ms_repeats'] = dict(calls=cov_calls, median=round(ts[len(ts) // 2], 4), min=round(ts[0], 4),
                                     max=round(ts[-1], 4))
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'r15', 'sba_ext_cov_time.json'))
    ap.add_argument('--max-iters', type=int, default=40)
    ap.add_argument('--cov-calls', type=int, default=1, help='further timed covariance calls (median, min, max)')
    a = ap.parse_args()
    device = int(os.environ.get('ACINOSET_DEVICE', 0))
    ctx = _native.Context(device)
    dev = torch.device('cuda', device)
    # one explicit stream carries the copies, the kernels and the timing events
    stream = torch.cuda.Stream(device=device)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    g = np.load(GOLDEN, allow_pickle=False)
    shapes = [('golden: 6 cameras x 80 points', _native.pack_cameras(g['K'], g['D'], g['R0'], g['t0']), g['points_2d'],
               g['point_indices'], g['camera_indices'], g['points_3d']),
              ('16 cameras x 400 points',) + ring_problem(400, 16),
              ('board-sized: 6 cameras x 20,000 points',) + ring_problem(20000, 6)]
    out = [time_case(ctx, dev, *s, a.max_iters, a.cov_calls) for s in shapes]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
