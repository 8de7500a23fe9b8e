"""Per-solve time of the points-only SBA for both camera models, device-resident, at the
configs[1] shape (the reference's ~2,000 points x 6 cameras) and the configs[4] shape (400,000
points x 12 cameras):

    fisheye, layout auto       what the headline runs (ROW / HOIST instances at the small shape)
    fisheye, layout butterfly  the LDS-staged instance family, forced where the row one is legal
    standard                   LDS-staged butterfly instances only (there are no others)

The standard problem has the fisheye problem's geometry, masks and start; its observations are
the truth projected through standard records (the scene's K, R, t with the coefficients below)
on the GPU, plus 1 px noise. No oracle, no reference reads: it only times. One JSON line per
case: ms per solve of every repeat (device events on the one stream that carries the context's
kernels, and a host clock around the same solves ending in a synchronise), and the solve's report.

    python tools/time_sba_models.py [--repeats 3] [--small-solves 20000] [--large-solves 1000] [--frames 20000]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from acinoset_amd import _native, synth, workloads  # noqa: E402

COEFFS = (-0.12, 0.03, 8e-4, -5e-4, -0.004, 0.05, -0.01, 0.002)   # k1 k2 p1 p2 k3 k4 k5 k6


def standard_problem(ctx, K, R, t, truth, mask, seed):
    """Standard records and (n, C, 2) observations of `truth` through them, 1 px noise."""
    C = len(K)
    rng = np.random.default_rng(seed)
    D = np.asarray(COEFFS) * (1.0 + rng.normal(0.0, 0.05, (C, 8)))
    cams = _native.pack_cameras_standard(K, D, R, t)
    n = len(truth)
    uv = np.empty((n, C, 2))
    for c in range(C):
        uv[:, c] = ctx.project(cams, truth, c)
    uv += rng.normal(0.0, 1.0, uv.shape)
    return cams, np.where(mask[..., None] > 0, uv, 0.0)


def time_case(ctx, dev, name, model, layout, cams, uv, mask, pts0, solves, repeats):
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_cams, d_uv, d_mask, d_pts0 = T(cams), T(uv), T(mask), T(pts0)
    d_pts = d_pts0.clone()
    n, C = mask.shape
    ctx.sba_set_lm_layout(layout)
    try:
        args = (d_cams.data_ptr(), C, d_uv.data_ptr(), d_mask.data_ptr(), n, d_pts.data_ptr())
        kw = dict(pts_in_p=d_pts0.data_ptr(), camera_model=model)
        rep = ctx.sba_points_dense_dev(*args, report=True, **kw)
        picked = ctx.sba_lm_layout(C, n, camera_model=model)[0]
        torch.cuda.synchronize(dev)
        for _ in range(max(solves // 10, 2)):      # warm-up of this instance and of the clocks
            ctx.sba_points_dense_dev(*args, **kw)
        torch.cuda.synchronize(dev)
        ms, host_ms = [], []
        for _ in range(repeats):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            s.record()
            for _ in range(solves):
                ctx.sba_points_dense_dev(*args, **kw)
            e.record()
            torch.cuda.synchronize(dev)
            host_ms.append(1e3 * (time.perf_counter() - t0) / solves)
            ms.append(s.elapsed_time(e) / solves)
    finally:
        ctx.sba_set_lm_layout('auto')
    print(json.dumps(dict(shape=name, n_pts=int(n), n_cams=int(C), model=model, layout=layout, instance=picked,
                          ms_per_solve=[round(v, 5) for v in ms], host_ms_per_solve=[round(v, 5) for v in host_ms],
                          iters_max=rep['iters_max'],
                          iters_sum=rep['iters_sum'], status=rep['status_counts'])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--small-solves', type=int, default=20000)
    ap.add_argument('--large-solves', type=int, default=1000)
    ap.add_argument('--frames', type=int, default=20000, help='frames of the 12-camera sequence (20 points each)')
    a = ap.parse_args()
    device = int(os.environ.get('ACINOSET_DEVICE', 0))
    ctx = _native.Context(device)
    dev = torch.device('cuda', device)
    # one explicit stream carries the copies, the kernels and the timing events
    stream = torch.cuda.Stream(device=device)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    wl = workloads.sba_reference_workload()
    shapes = [('configs[1]', wl.K, wl.R, wl.t, wl.cams, wl.uv, wl.mask, wl.pts0, wl.truth, a.small_solves)]
    scene = synth.ring_scene(12)
    seq = synth.make_sequence(a.frames, scene, mode='default_nolure', seed=4242)
    uv, mask, pts0, truth, _ = synth.dense_sba_problem(seq)
    shapes.append(('configs[4]', scene.K, scene.R, scene.t, _native.pack_cameras(scene.K, scene.D, scene.R, scene.t), uv,
                   mask, pts0, truth, a.large_solves))
    for name, K, R, t, cams, uv, mask, pts0, truth, solves in shapes:
        scams, suv = standard_problem(ctx, K, R, t, truth, mask, seed=12)
        for model, layout, c, o in (('fisheye', 'auto', cams, uv), ('fisheye', 'butterfly', cams, uv),
                                    ('standard', 'auto', scams, suv)):
            time_case(ctx, dev, name, model, layout, c, o, mask, pts0, solves, a.repeats)


if __name__ == '__main__':
    main()
