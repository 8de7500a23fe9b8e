"""Time per LM iteration of acs_sba_boards, beside acs_sba_extrinsics on the same data posed as free
corners.

    python tools/time_sba_boards.py [OUT.json]

Device pointers, a pair of device events around each call, one timed run per shape (after one untimed
run that sizes the workspace); the solve time is divided by the iterations of the report. Shapes:
6 cameras x 40 boards x 54 corners and 16 cameras x 200 boards x 54 corners, 2..C views per board, 0.5 px
noise, a perturbed start, 40 iterations at most. Prints one JSON line per shape and writes them to OUT.json.
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


def _timed(torch, ctx, call):
    call()
    ctx.sync()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    rep = call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3, rep


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
        p2, X, pi, ci = ref.free_corners(rig, bR0, bt0)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        d = dict(obj=up(rig['obj']), uv=up(rig['uv']), mask=up(rig['mask']), p2=up(p2), pi=up(pi.astype(np.int32)),
                 ci=up(ci.astype(np.int32)))
        opts = ctx.sba_ext_opts(max_iters=MAX_ITERS)

        def boards():
            c, p = up(cams), up(poses)
            return ctx.sba_boards_dev(c.data_ptr(), C, d['obj'].data_ptr(), nc, d['uv'].data_ptr(), d['mask'].data_ptr(),
                                      B, p.data_ptr(), opts)

        def free():
            import ctypes
            c, x = up(cams), up(X)
            rep = _native.SbaExtReport()
            v = ctypes.c_void_p
            ctx.check(ctx.lib.acs_sba_extrinsics(ctx.h, v(c.data_ptr()), C, v(d['p2'].data_ptr()), v(d['pi'].data_ptr()),
                                                 v(d['ci'].data_ptr()), len(p2), v(x.data_ptr()), len(X),
                                                 ctypes.byref(opts), None, None, ctypes.byref(rep),
                                                 _native.ACS_DEVICE_PTRS), 'acs_sba_extrinsics')
            return rep.as_dict()

        tb, rb = _timed(torch, ctx, boards)
        tf, rf = _timed(torch, ctx, free)
        row = dict(n_cams=C, n_boards=B, n_corners=nc, n_views=int(rig['mask'].sum()),
                   boards=dict(solve_us=tb, iters=rb['iters'], us_per_iter=tb / max(rb['iters'], 1),
                               status=rb['status_name'], cost_after=rb['cost_after']),
                   free_corners=dict(solve_us=tf, iters=rf['iters'], us_per_iter=tf / max(rf['iters'], 1),
                                     status=rf['status_name'], cost_after=rf['cost_after'], n_points=len(X)))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if out:
        with open(out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else None)
