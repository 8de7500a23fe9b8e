"""Time acs_fte_covariance beside one LM iteration of acs_fte_solve, on one MI355X.

Sizes: the configs[2] (1,000 frames) and configs[3] (10,000 frames) FTE workloads of bench.py
(acinoset_amd.workloads). Every array is resident in HBM (device pointers). The state is the
one five LM iterations from the reference initialisation leave (not converged, so the next
iteration does a full step). Both calls are timed with device events on the context's stream,
warm, in one process: the covariance without cov_marker (asynchronous enqueue), and
acs_fte_solve limited to one iteration from that state (its own host polling included).
Writes profiles/<round>/fte_cov_time.json:  python tools/time_fte_cov.py [round] [reps]."""
import json
import os
import sys

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402


def _median_ms(torch, stream, fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts = np.array(ts)
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def measure(ctx, torch, stream, n_frames, reps):
    from acinoset_amd import _native, workloads
    wl = workloads.fte_workload(ctx, n_frames)
    table, N, C = wl.table, wl.meas.shape[0], len(wl.cams)
    dv = torch.device('cuda', torch.cuda.current_device())
    T = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dv, dt)  # noqa: E731
    d = dict(ints=T(table.ints, torch.int32), reals=T(table.reals), cams=T(wl.cams), meas=T(wl.meas), w=T(wl.w),
             qinv=T(wl.qinv))
    head = (d['ints'].data_ptr(), len(table.ints), d['reals'].data_ptr(), len(table.reals), d['cams'].data_ptr(), C,
            d['meas'].data_ptr(), d['w'].data_ptr(), N, True, wl.Ts, d['qinv'].data_ptr(), 1)
    # the common state: five LM iterations from the initialisation
    X5, tau5 = T(wl.X0), torch.zeros(C, dtype=torch.float64, device=dv)
    rep5 = ctx.fte_solve_dev(*head, X5.data_ptr(), tau5.data_ptr(), ctx.fte_default_opts(max_iters=5))
    d_X, d_tau = X5.clone(), tau5.clone()
    P = table.P
    x_cov = torch.empty((N + 2, P, P), dtype=torch.float64, device=dv)
    tau_cov = torch.empty((C, C), dtype=torch.float64, device=dv)
    one = ctx.fte_default_opts(max_iters=1)
    last = {}

    def cov():
        ctx.fte_covariance_dev(*head, X5.data_ptr(), tau5.data_ptr(), x_cov.data_ptr(),
                               tau_cov.data_ptr())

    def lm1():
        d_X.copy_(X5)
        d_tau.copy_(tau5)
        last['rep'] = ctx.fte_solve_dev(*head, d_X.data_ptr(), d_tau.data_ptr(), one)

    def copies():
        d_X.copy_(X5)
        d_tau.copy_(tau5)

    cov()
    torch.cuda.synchronize()
    a0 = _native.alloc_events()
    t_cov = _median_ms(torch, stream, cov, reps)
    allocs = _native.alloc_events() - a0
    t_lm = _median_ms(torch, stream, lm1, reps)
    t_cp = _median_ms(torch, stream, copies, reps)
    rep = ctx.fte_covariance_dev(*head, X5.data_ptr(), tau5.data_ptr(), x_cov.data_ptr(),
                                 tau_cov.data_ptr(), report=True)
    nblk, BP, GR = (N + 4) // 3, (3 * P + 15) // 16 * 16, (C + 1 + 15) // 16 * 16
    store = 8 * nblk * (4 * BP * BP + 2 * BP * GR)
    sd = np.sqrt(np.diagonal(x_cov.cpu().numpy(), axis1=1, axis2=2))
    return {
        'frames': N, 'cameras': C, 'P': P, 'n_blk': nblk, 'BP': BP, 'GR': GR, 'reps': reps,
        'state': f'after {rep5["iters"]} LM iterations from the reference initialisation',
        'covariance_ms': {'median': t_cov[0], 'min': t_cov[1], 'max': t_cov[2]},
        'one_lm_iteration_ms': {'median': t_lm[0] - t_cp[0], 'min': t_lm[1] - t_cp[0], 'max': t_lm[2] - t_cp[0],
                                'state_reset_copies_ms_subtracted': t_cp[0], 'iters': last['rep']['iters']},
        'ratio_cov_over_lm_iteration': t_cov[0] / (t_lm[0] - t_cp[0]),
        'alloc_events_in_timed_covariance_calls': allocs,
        'covariance_store_bytes': store,
        'report': rep,
        'root_position_sd_m': {'first_virtual_frame': float(sd[0, :3].max()), 'mid_clip': float(sd[N // 2, :3].max())},
        'how': 'device events on the context stream around each call, warm (3 calls first), median of reps; '
               'covariance: device pointers, no cov_marker, no report (asynchronous enqueue); LM iteration: '
               'acs_fte_solve max_iters = 1 from the same state, minus the two state-reset copies',
    }


def main():
    rnd = sys.argv[1] if len(sys.argv) > 1 else 'r09'
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    import torch
    from acinoset_amd import _native
    ctx = _native.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    out = {'device': torch.cuda.get_device_name(0), 'sizes': [measure(ctx, torch, stream, n, reps)
                                                              for n in (1000, 10000)]}
    path = os.path.join(REPO, 'profiles', rnd)
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, 'fte_cov_time.json'), 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
