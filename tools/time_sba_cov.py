"""Time of one SBA covariance call (acs_sba_points_dense_covariance) beside one solve
(acs_sba_points_dense_io) of the same shape in the same session, device-resident, at the
configs[1] shape (the reference's ~2,000 points x 6 cameras) and the configs[4] shape (400,000
points x 12 cameras), fisheye and standard model.

The covariance is evaluated at the solve's solution. Every call is timed on its own with a pair
of device events on the one stream that carries the context's kernels, after a warm-up; the
figure is the median of 20. The standard problem is tools/time_sba_models.py's. No oracle, no
reference reads: it only times. The table goes to --out as JSON (one record per shape and model)
and to stdout.

    python tools/time_sba_cov.py [--calls 20] [--frames 20000] [--out profiles/r13/sba_cov_time.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from acinoset_amd import _native, synth, workloads  # noqa: E402
from time_sba_models import standard_problem  # noqa: E402


def _median_ms(dev, fn, calls, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(calls):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize(dev)
        ms.append(s.elapsed_time(e))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def time_case(ctx, dev, name, model, cams, uv, mask, pts0, calls):
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_cams, d_uv, d_mask, d_pts0 = T(cams), T(uv), T(mask), T(pts0)
    n, C = mask.shape
    d_pts = d_pts0.clone()
    d_cov = torch.empty((n, 3, 3), dtype=torch.float64, device=dev)
    d_st = torch.empty(n, dtype=torch.int32, device=dev)
    sargs = (d_cams.data_ptr(), C, d_uv.data_ptr(), d_mask.data_ptr(), n, d_pts.data_ptr())
    skw = dict(pts_in_p=d_pts0.data_ptr(), camera_model=model)
    cargs = sargs + (d_cov.data_ptr(),)
    srep = ctx.sba_points_dense_dev(*sargs, report=True, **skw)
    crep = ctx.sba_points_dense_covariance_dev(*cargs, status_p=d_st.data_ptr(), report=True, camera_model=model)
    before = _native.alloc_events()
    solve = _median_ms(dev, lambda: ctx.sba_points_dense_dev(*sargs, **skw), calls)
    cov = _median_ms(dev, lambda: ctx.sba_points_dense_covariance_dev(*cargs, status_p=d_st.data_ptr(),
                                                                     camera_model=model), calls)
    nobs = int(mask.sum())
    # bytes the covariance kernel moves per point: observation slots (16 + 1 B each), the point, cov, status
    bytes_pt = 17.0 * C + 24 + 72 + 4
    rec = dict(shape=name, model=model, n_pts=int(n), n_cams=int(C), n_obs=nobs, calls=calls,
               cov_ms_median=round(cov[0], 5), cov_ms_min=round(cov[1], 5), cov_ms_max=round(cov[2], 5),
               solve_ms_median=round(solve[0], 5), solve_ms_min=round(solve[1], 5), solve_ms_max=round(solve[2], 5),
               cov_over_solve=round(cov[0] / solve[0], 4), bytes_per_point=bytes_pt,
               cov_gb_per_s=round(bytes_pt * n / (cov[0] * 1e-3) / 1e9, 2),
               alloc_events_in_timed_calls=_native.alloc_events() - before,
               solve_iters_max=srep['iters_max'], solve_iters_sum=srep['iters_sum'], cov_report=crep)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--frames', type=int, default=20000, help='frames of the 12-camera sequence (20 points each)')
    ap.add_argument('--out', default=os.path.join('profiles', 'r13', 'sba_cov_time.json'))
    a = ap.parse_args()
    device = int(os.environ.get('ACINOSET_DEVICE', 0))
    ctx = _native.Context(device)
    dev = torch.device('cuda', device)
    # one explicit stream carries the copies, the kernels and the timing events
    stream = torch.cuda.Stream(device=device)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    wl = workloads.sba_reference_workload()
    shapes = [('configs[1]', wl.K, wl.R, wl.t, wl.cams, wl.uv, wl.mask, wl.pts0, wl.truth)]
    scene = synth.ring_scene(12)
    seq = synth.make_sequence(a.frames, scene, mode='default_nolure', seed=4242)
    uv, mask, pts0, truth, _ = synth.dense_sba_problem(seq)
    shapes.append(('configs[4]', scene.K, scene.R, scene.t, _native.pack_cameras(scene.K, scene.D, scene.R, scene.t), uv,
                   mask, pts0, truth))
    out = []
    for name, K, R, t, cams, uv, mask, pts0, truth in shapes:
        scams, suv = standard_problem(ctx, K, R, t, truth, mask, seed=12)
        for model, c, o in (('fisheye', cams, uv), ('standard', scams, suv)):
            out.append(time_case(ctx, dev, name, model, c, o, mask, pts0, a.calls))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
