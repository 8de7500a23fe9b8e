"""Time of acs_sba_boards_covariance, beside one LM iteration of acs_sba_boards on the same data in
the same process.

    python tools/time_sba_boards_cov.py [OUT.json]

Device pointers, a pair of device events around each call. Per shape: the solver runs twice (the first
run sizes the workspace, the second is timed; its time over the iterations of its report is the
yardstick), then the covariance is evaluated at that solution: two untimed calls, then REPEATS timed
windows of CALLS calls each (median and spread over the windows), with acs_alloc_events read before
and after the timed windows (the calls allocate nothing). The call includes its own wait for the stream and
the copy of the report to the host. Shapes: 6 cameras x 40 boards x 54 corners and 16 cameras x 200
boards x 54 corners, 2..C views per board, 0.5 px noise, a perturbed start, 40 iterations at most. Prints
one JSON line per shape and writes them to OUT.json. No time or ratio is asserted.
"""
import json
import os
import sys

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
import numpy as np  # noqa: E402

SHAPES = [(6, 40, (9, 6)), (16, 200, (9, 6))]
MAX_ITERS = 40
REPEATS, CALLS = 7, 20


def _window(torch, call, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        rep = call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n, rep


def main(out):
    import torch
    import sba_boards_ref as ref
    from acinoset_amd import _native
    ctx = _native.Context(int(os.environ.get('ACINOSET_DEVICE', 0)))
    dev = torch.device('cuda', int(os.environ.get('ACINOSET_DEVICE', 0)))
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    rows = []
    for C, B, shape in SHAPES:
        rig = ref.make_rig(C, B, shape=shape, seed=1, views=(2, C), noise=0.5)
        R0, t0, bR0, bt0 = ref.perturb(rig, 2)
        nc = len(rig['obj'])
        cams = _native.pack_cameras(rig['K'], rig['D'], R0, t0)
        poses = np.concatenate([bR0.reshape(-1, 9), bt0], 1)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        d = dict(obj=up(rig['obj']), uv=up(rig['uv']), mask=up(rig['mask']))
        opts = ctx.sba_ext_opts(max_iters=MAX_ITERS)
        state = {}

        def solve():
            state['c'], state['p'] = up(cams), up(poses)
            return ctx.sba_boards_dev(state['c'].data_ptr(), C, d['obj'].data_ptr(), nc, d['uv'].data_ptr(),
                                      d['mask'].data_ptr(), B, state['p'].data_ptr(), opts)

        solve()
        ctx.sync()
        ts, rs = _window(torch, solve, 1)
        cc = torch.empty((6 * C, 6 * C), dtype=torch.float64, device=dev)
        cb = torch.empty((B, 6, 6), dtype=torch.float64, device=dev)
        st = torch.empty((B,), dtype=torch.int32, device=dev)

        def cov():
            return ctx.sba_boards_covariance_dev(state['c'].data_ptr(), C, d['obj'].data_ptr(), nc, d['uv'].data_ptr(),
                                                 d['mask'].data_ptr(), B, state['p'].data_ptr(), cc.data_ptr(),
                                                 cb.data_ptr(), st.data_ptr())

        cov()
        cov()
        before = _native.alloc_events()
        wins = [_window(torch, cov, CALLS) for _ in range(REPEATS)]
        allocs = _native.alloc_events() - before
        us = sorted(w[0] for w in wins)
        rc = wins[-1][1]
        per_iter = ts / max(rs['iters'], 1)
        row = dict(n_cams=C, n_boards=B, n_corners=nc, n_views=int(rig['mask'].sum()),
                   solve=dict(solve_us=ts, iters=rs['iters'], us_per_iter=per_iter, status=rs['status_name']),
                   covariance=dict(us_median=us[len(us) // 2], us_min=us[0], us_max=us[-1], windows=REPEATS,
                                   calls_per_window=CALLS, alloc_events_in_timed_calls=allocs, status=rc['status_name'],
                                   n_ok=rc['n_ok'], min_pivot=rc['min_pivot'], sigma_hat_px=rc['sigma_hat_px'],
                                   rot_sd_max=rc['rot_sd_max'], trans_sd_max=rc['trans_sd_max']),
                   covariance_in_lm_iterations=us[len(us) // 2] / per_iter)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if out:
        with open(out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else None)
