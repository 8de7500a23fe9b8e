"""Time per LM iteration of acs_sba_boards_points (rigid boards with free points in one solve), beside
acs_sba_boards on the same boards in the same session and build.

    python tools/time_sba_boards_points.py [OUT.json] [--shape I]

Device pointers, a pair of device events around each call, one timed run per shape (after one untimed
run that sizes the workspace; the state is uploaded before the first event); the solve time is divided by
the iterations of the report. Shapes: 6 cameras x 40 boards x 54 corners with 20 points and 16 cameras x
200 boards x 54 corners with 50 points; 2..C views per board and per point, 0.5 px noise, a perturbed
start, 40 iterations at most. Prints one JSON line per shape and writes them to OUT.json. --shape I runs
shape I alone (for a kernel trace of its own).
"""
import json
import os
import sys

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
import numpy as np  # noqa: E402

SHAPES = [(6, 40, (9, 6), 20), (16, 200, (9, 6), 50)]
MAX_ITERS = 40


def _timed(torch, ctx, prepare, call):
    call(*prepare())
    ctx.sync()
    state = prepare()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    rep = call(*state)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3, rep


def main(out, only=None):
    import torch
    import sba_boards_points_ref as ref
    from acinoset_amd import _native
    ctx = _native.Context(int(os.environ.get('ACINOSET_DEVICE', 0)))
    dev = torch.device('cuda', int(os.environ.get('ACINOSET_DEVICE', 0)))
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    rows = []
    for i, (C, B, shape, n) in enumerate(SHAPES):
        if only is not None and i != only:
            continue
        rig = ref.make_rig(C, B, shape=shape, n_pts=n, seed=1, views=(2, C), pt_vis=(2, C), noise=0.5)
        R0, t0, bR0, bt0, X0 = ref.perturb(rig, 2)
        nc = len(rig['obj'])
        cams = _native.pack_cameras(rig['K'], rig['D'], R0, t0)
        poses = np.concatenate([bR0.reshape(-1, 9), bt0], 1)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        d = dict(obj=up(rig['obj']), uv=up(rig['uv']), mask=up(rig['mask']), puv=up(rig['pt_uv']),
                 pm=up(rig['pt_mask']))
        opts = ctx.sba_ext_opts(max_iters=MAX_ITERS)

        def prepare():
            return up(cams), up(poses), up(X0)

        def boards(c, p, x):
            return ctx.sba_boards_dev(c.data_ptr(), C, d['obj'].data_ptr(), nc, d['uv'].data_ptr(), d['mask'].data_ptr(),
                                      B, p.data_ptr(), opts)

        def mixed(c, p, x):
            return ctx.sba_boards_points_dev(c.data_ptr(), C, d['obj'].data_ptr(), nc, d['uv'].data_ptr(),
                                             d['mask'].data_ptr(), B, p.data_ptr(), d['puv'].data_ptr(),
                                             d['pm'].data_ptr(), n, x.data_ptr(), opts)

        tb, rb = _timed(torch, ctx, prepare, boards)
        tm, rm = _timed(torch, ctx, prepare, mixed)
        row = dict(n_cams=C, n_boards=B, n_corners=nc, n_views=int(rig['mask'].sum()), n_points=n,
                   n_point_obs=int(rig['pt_mask'].sum()),
                   boards=dict(solve_us=tb, iters=rb['iters'], us_per_iter=tb / max(rb['iters'], 1),
                               status=rb['status_name'], cost_after=rb['cost_after']),
                   boards_points=dict(solve_us=tm, iters=rm['iters'], us_per_iter=tm / max(rm['iters'], 1),
                                      status=rm['status_name'], cost_after=rm['cost_after']))
        row['added_us_per_iter'] = row['boards_points']['us_per_iter'] - row['boards']['us_per_iter']
        rows.append(row)
        print(json.dumps(row), flush=True)
    if out:
        with open(out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    args = sys.argv[1:]
    only = None
    if '--shape' in args:
        k = args.index('--shape')
        only = int(args[k + 1])
        del args[k:k + 2]
    main(args[0] if args else None, only)
