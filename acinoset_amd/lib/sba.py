"""Mirror of src/lib/sba.py (points-only SBA and its data glue) on the GPU.

* `bundle_adjust_points_only` (:181-195) -> acs_sba_points: the same robust objective
  (Cauchy, f_scale, residual = reprojection - observation) minimised per point by the
  fused LM kernel; returns (obj_pts, {'before', 'after'}) exactly like the reference.
* `cost_func_points_only` (:149-153) -> acs_sba_residuals.
* `_sba_points` (:285-313) keeps the reference's point selection (adjacent-pair
  triangulation + inner merge on (frame, marker)) and index semantics.
* `bundle_adjust_points_and_extrinsics` (:158-178) -> acs_sba_extrinsics (Schur LM).
* Calibration-board front end (:37-137, :196-282): `prepare_calib_board_data_for_bundle_
  adjustment`, `prepare_manual_points_for_bundle_adjustment`, `bundle_adjust_board_points_only`
  and `_sba_board_points`, with every image's first-two-camera triangulation batched into one
  GPU call (acs_triangulate_pairs) and the joint points + extrinsics solve on the GPU.
"""
import json
import os
from time import time

import numpy as np

from .. import _native
from . import calib
from .utils import get_pairwise_3d_points_from_df, load_manual_points, load_points, load_scene, save_scene


def create_bundle_adjustment_jacobian_sparsity_matrix(n_cams, n_params_per_camera, camera_indices, n_points,
                                                      point_indices):
    """The Jacobian sparsity pattern of `src/lib/sba.py:11-22` as metadata (the GPU solver
    works on the per-point blocks directly and never builds it): residual rows 2i, 2i+1 of
    observation i touch its camera's parameter columns and its point's 3 columns, laid
    out [cameras | points]. Built in one COO pass and returned as a lil matrix of ints."""
    from scipy.sparse import coo_matrix
    cam = np.asarray(camera_indices, np.int64)
    pt = np.asarray(point_indices, np.int64)
    n_obs = cam.size
    cols_per_obs = np.concatenate([cam[:, None] * n_params_per_camera + np.arange(n_params_per_camera),
                                   n_cams * n_params_per_camera + pt[:, None] * 3 + np.arange(3)], 1)
    k = cols_per_obs.shape[1]
    rows = (2 * np.arange(n_obs)[:, None, None] + np.arange(2)[None, :, None]).repeat(k, 2)
    cols = np.broadcast_to(cols_per_obs[:, None, :], rows.shape)
    shape = (2 * n_obs, n_cams * n_params_per_camera + 3 * n_points)
    A = coo_matrix((np.ones(rows.size, int), (rows.ravel(), cols.ravel())), shape=shape).tolil()
    return A


def is_standard_model(func):
    """Whether a `project_func` / `triangulate_func` argument selects the standard (pinhole)
    model: only `calib.project_points` and `calib.triangulate_points` themselves do. None and
    the fisheye functions select the fisheye model, and so does any other callable (it is not
    called: the model is built into the kernels)."""
    return func is calib.project_points or func is calib.triangulate_points


def _cams(k_arr, d_arr, r_arr, t_arr, standard=False):
    n = len(k_arr)
    if standard:
        return _native.pack_cameras_standard(k_arr, d_arr, r_arr, np.asarray(t_arr).reshape(n, 3))
    return _native.pack_cameras(k_arr, np.asarray(d_arr).reshape(n, 4), r_arr, np.asarray(t_arr).reshape(n, 3))


def cost_func_points_only(params, n_points, point_3d_indices, camera_indices, k_arr, d_arr, r_arr, t_arr, points_2d,
                          project_func=None):
    """`src/lib/sba.py:149-153`. `project_func is calib.project_points` selects the standard
    model; None, the fisheye function and any other callable the fisheye model."""
    obj = np.asarray(params, np.float64).reshape(n_points, 3)
    cams = _cams(k_arr, d_arr, r_arr, t_arr, is_standard_model(project_func))
    return _native.default_context().sba_residuals(cams, points_2d, point_3d_indices, camera_indices, obj)


def bundle_adjust_points_only(points_2d, points_3d, point_3d_indices, camera_indices, k_arr, d_arr, r_arr, t_arr,
                              project_func=None, f_scale=50, covariance=False, sigma_px=1.0, **opts):
    """Points-only robust BA. Both camera models are built into the kernel and `project_func`
    selects between them: `calib.project_points` (src/lib/app.py:129-132) runs the standard
    model; None and `calib.project_points_fisheye` (src/lib/app.py:135-138) the fisheye model,
    and so does any other callable, which is never called.
    `covariance=True` adds to the returned dict `cov` (n, 3, 3) in m^2, `cov_status` (n,) and
    `cov_report` (acs_sba_points_covariance at the solved points, same f_scale, pixel noise
    `sigma_px`); the points and residuals are those of the plain call."""
    ctx = _native.default_context()
    o = ctx.sba_opts(f_scale=float(f_scale), **opts)
    t0 = time()
    cams = _cams(k_arr, d_arr, r_arr, t_arr, is_standard_model(project_func))
    pts, rb, ra, rep = ctx.sba_points(cams, np.asarray(points_2d, np.float64),
                                      np.asarray(point_3d_indices), np.asarray(camera_indices),
                                      np.asarray(points_3d, np.float64), o)
    t1 = time()
    print(f'GPU SBA: {rep["n_problems"]} points, iters max {rep["iters_max"]}, cost {rep["cost_before"]:.4e} -> '
          f'{rep["cost_after"]:.4e}, status {rep["status_counts"]}')
    print(f'\nOptimization took {t1 - t0:.2f} seconds')
    res = dict(before=rb, after=ra)
    if covariance:
        cov, cst, crep = ctx.sba_points_covariance(cams, np.asarray(points_2d, np.float64),
                                                   np.asarray(point_3d_indices), np.asarray(camera_indices), pts,
                                                   f_scale=float(f_scale), sigma_px=float(sigma_px))
        print(f'GPU SBA covariance: {crep["n_ok"]} ok, {crep["n_degenerate"]} degenerate, {crep["n_noobs"]} without '
              f'observations; sigma_hat {crep["sigma_hat_px"]:.4f} px (sigma_px {float(sigma_px):g})')
        res.update(cov=cov, cov_status=cst, cov_report=crep)
    return pts, res


def _sba_points(scene_fpath, points_2d_df, triangulate_func=None, project_func=None, covariance=False, sigma_px=1.0):
    """`src/lib/sba.py:285-313`. `calib.triangulate_points` / `calib.project_points` select the
    standard model for the initialisation / the solve (see bundle_adjust_points_only).
    With `covariance`, res['cov'] / res['cov_status'] rows follow the returned DataFrame's rows."""
    k_arr, d_arr, r_arr, t_arr, cam_res = load_scene(scene_fpath)
    d_tri = d_arr if is_standard_model(triangulate_func) else d_arr.reshape((-1, 4))
    points_3d_df = get_pairwise_3d_points_from_df(points_2d_df, k_arr, d_tri, r_arr, t_arr, triangulate_func)
    points_3d_df['point_index'] = points_3d_df.index
    points_3d = np.array(points_3d_df[['x', 'y', 'z']], dtype=np.float64)
    points_df = points_2d_df.merge(points_3d_df, how='inner', on=['frame', 'marker'], suffixes=('_cam', ''))
    points_2d = np.array(points_df[['x_cam', 'y_cam']], dtype=np.float64)
    point_indices = np.array(points_df['point_index'])
    camera_indices = np.array(points_df['camera'])
    print('bundle_adjust_points_only')
    pts_3d, res = bundle_adjust_points_only(points_2d, points_3d, point_indices, camera_indices, k_arr, d_arr, r_arr,
                                            t_arr, project_func, f_scale=50, covariance=covariance,
                                            sigma_px=sigma_px)
    print(f"\nBefore: mean: {np.mean(res['before'])}, std: {np.std(res['before'])}")
    print(f"After: mean: {np.mean(res['after'])}, std: {np.std(res['after'])}\n")
    new_points_3d_df = points_3d_df.copy()
    new_points_3d_df[['x', 'y', 'z']] = pts_3d
    return new_points_3d_df, res


def rodrigues_to_matrix(rvecs):
    """Rotation vectors (n,3) -> matrices (n,3,3) (cv::Rodrigues, vector -> matrix)."""
    rv = np.asarray(rvecs, np.float64).reshape(-1, 3)
    out = np.empty((len(rv), 3, 3))
    for i, r in enumerate(rv):
        th = np.linalg.norm(r)
        if th < np.finfo(np.float64).eps:
            out[i] = np.eye(3)
            continue
        k = r / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        out[i] = np.cos(th) * np.eye(3) + (1 - np.cos(th)) * np.outer(k, k) + np.sin(th) * Kx
    return out


def matrix_to_rodrigues(R_arr):
    """Rotation matrices (n,3,3) -> rotation vectors (n,3) (cv::Rodrigues, matrix -> vector)."""
    out = []
    for R in np.asarray(R_arr, np.float64).reshape(-1, 3, 3):
        U, _, Vt = np.linalg.svd(R)
        R = U @ Vt
        c = np.clip((np.trace(R) - 1) * 0.5, -1.0, 1.0)
        th = np.arccos(c)
        v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
        s = np.linalg.norm(v) * 0.5
        if s < 1e-5:
            if c > 0:
                out.append(np.zeros(3))
                continue
            w, V = np.linalg.eigh((R + np.eye(3)) * 0.5)
            ax = V[:, np.argmax(w)]
            out.append(ax * th)
            continue
        out.append(v * (th / (2 * s)))
    return np.array(out)


def params_to_points_extrinsics(params, n_cams, n_points):
    """`src/lib/sba.py:25-32`."""
    r_end = n_cams * 3
    t_end = r_end + n_cams * 3
    r_arr = rodrigues_to_matrix(params[:r_end].reshape(n_cams, 3))
    t_arr = params[r_end:t_end].reshape((n_cams, 3, 1))
    obj_pts = params[t_end:].reshape((n_points, 3))
    return obj_pts, r_arr, t_arr


def cost_func_points_extrinsics(params, n_cams, n_points, point_3d_indices, camera_indices, k_arr, d_arr, points_2d,
                                project_func=None):
    """`src/lib/sba.py:142-146`."""
    obj, r_arr, t_arr = params_to_points_extrinsics(np.asarray(params, np.float64), n_cams, n_points)
    return cost_func_points_only(obj.ravel(), n_points, point_3d_indices, camera_indices, k_arr, d_arr, r_arr, t_arr,
                                 points_2d, project_func)


def camera_centres(r_arr, t_arr):
    """World-frame camera centres c = -R^T t, (C, 3)."""
    R = np.asarray(r_arr, np.float64).reshape(-1, 3, 3)
    t = np.asarray(t_arr, np.float64).reshape(-1, 3)
    return -np.einsum('cji,cj->ci', R, t)


def default_anchor(r_arr, t_arr):
    """The default anchor pair of the pose covariance: camera 0 and the camera whose centre is
    farthest from it (the lowest index on ties)."""
    c = camera_centres(r_arr, t_arr)
    return 0, int(np.argmax(np.linalg.norm(c - c[0], axis=1)))


def camera_centre_covariance(cov_block, r, t):
    """Covariance (3, 3, m^2) of a camera's centre c = -R^T t in world coordinates from its pose
    block (6, 6) over (dw, dt) with R <- exp([dw]x) R, t <- t + dt: J cov J^T with
    J = dc/d(dw, dt) = [-R^T [t]x | -R^T]."""
    R = np.asarray(r, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64).reshape(3)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    J = np.concatenate([-R.T @ tx, -R.T], 1)
    return J @ np.asarray(cov_block, np.float64).reshape(6, 6) @ J.T


def bundle_adjust_points_and_extrinsics(points_2d, points_3d, point_3d_indices, camera_indices, k_arr, d_arr, r_arr,
                                        t_arr, project_func=None, f_scale=1.0, covariance=False, sigma_px=1.0,
                                        gauge='anchor', anchor=None, **opts):
    """`src/lib/sba.py:158-178` -> acs_sba_extrinsics: points and every camera's rotation and
    translation refined together (intrinsics fixed) on the same Cauchy objective (scipy's
    default f_scale = 1). Returns (obj_pts (n,3), r_arr (C,3,3), t_arr (C,3,1),
    {'before', 'after'}) like the reference; rotations stay orthonormal matrices (updated
    on SO(3), which is what the reference's Rodrigues round trip represents).
    Fisheye model only: `project_func=calib.project_points` raises NotImplementedError.
    `covariance=True` adds to the returned dict, evaluated at the returned solution with the same
    f_scale and the pixel noise `sigma_px` (acs_sba_extrinsics_covariance): `cov_cams` (6C, 6C),
    camera c's (dw, dt) at rows 6c..6c+5 with R <- exp([dw]x) R (rad) and t <- t + dt (m);
    `cov_cam_blocks` (C, 6, 6), its diagonal blocks; `cov_points` (n, 3, 3), the joint point
    covariances; `cov_status` (n,) and `cov_report` (with 'gauge' and 'anchor'). gauge 'anchor'
    holds camera anchor[0]'s pose and the distance between the centres of anchor[0] and anchor[1]
    (default: default_anchor of the solution); 'free' is the inner-constraint gauge. The points,
    cameras and residuals are those of the plain call."""
    if is_standard_model(project_func):
        raise NotImplementedError('bundle_adjust_points_and_extrinsics: the standard camera model is built for the '
                                  'points-only SBA only (the joint solve would silently use the fisheye model)')
    ctx = _native.default_context()
    n = len(k_arr)
    o = ctx.sba_ext_opts(f_scale=float(f_scale), **opts)
    t0 = time()
    cams, pts, rb, ra, rep = ctx.sba_extrinsics(_cams(k_arr, d_arr, r_arr, t_arr), np.asarray(points_2d, np.float64),
                                                np.asarray(point_3d_indices), np.asarray(camera_indices),
                                                np.asarray(points_3d, np.float64), o)
    t1 = time()
    print(f'GPU SBA (points + extrinsics): {len(pts)} points, {n} cameras, {rep["iters"]} iterations, cost '
          f'{rep["cost_before"]:.6e} -> {rep["cost_after"]:.6e} ({rep["status_name"]})')
    print(f'\nOptimization took {t1 - t0:.2f} seconds')
    r_out = cams[:, 8:17].reshape(n, 3, 3).copy()
    t_out = cams[:, 17:20].reshape(n, 3, 1).copy()
    res = dict(before=rb, after=ra)
    if covariance:
        pair = default_anchor(r_out, t_out) if anchor is None else (int(anchor[0]), int(anchor[1]))
        cc, cp, cst, crep = ctx.sba_extrinsics_covariance(cams, np.asarray(points_2d, np.float64),
                                                          np.asarray(point_3d_indices), np.asarray(camera_indices),
                                                          pts, f_scale=float(f_scale), sigma_px=float(sigma_px),
                                                          gauge=gauge, anchor=pair)
        crep.update(gauge=gauge, anchor=pair if gauge == 'anchor' else None)
        print(f'GPU SBA pose covariance ({gauge}): {crep["status_name"]}, rotation sd <= {crep["rot_sd_max"]:.3e} rad, '
              f'translation sd <= {crep["trans_sd_max"]:.3e} m; sigma_hat {crep["sigma_hat_px"]:.4f} px (sigma_px '
              f'{float(sigma_px):g})')
        blocks = np.stack([cc[6 * c:6 * c + 6, 6 * c:6 * c + 6] for c in range(n)])
        res.update(cov_cams=cc, cov_cam_blocks=blocks, cov_points=cp, cov_status=cst, cov_report=crep)
    return pts, r_out, t_out, res


# ---- calibration-board front end (src/lib/sba.py:37-137, :196-282) -----------------------

def _triangulate_batch(jobs, k_arr, d_arr, r_arr, t_arr, triangulate_func):
    """jobs: [(uv_a (n,2), uv_b (n,2), cam_a, cam_b)] -> list of (n, 3). The fisheye model
    (triangulate_func None or calib.triangulate_points_fisheye) and the standard model
    (calib.triangulate_points) run as ONE GPU batch; any other triangulate_func is called per
    job, as the reference does."""
    from .calib import triangulate_points_fisheye
    if not jobs:
        return []
    standard = is_standard_model(triangulate_func)
    if triangulate_func is not None and triangulate_func is not triangulate_points_fisheye and not standard:
        return [np.asarray(triangulate_func(a, b, k_arr[ca], d_arr[ca], r_arr[ca], t_arr[ca],
                                            k_arr[cb], d_arr[cb], r_arr[cb], t_arr[cb])).reshape(-1, 3)
                for a, b, ca, cb in jobs]
    cams = _cams(k_arr, d_arr, r_arr, t_arr, standard)
    uva = np.concatenate([np.asarray(a, np.float64).reshape(-1, 2) for a, _, _, _ in jobs])
    uvb = np.concatenate([np.asarray(b, np.float64).reshape(-1, 2) for _, b, _, _ in jobs])
    cia = np.concatenate([np.full(len(np.asarray(a).reshape(-1, 2)), ca, np.int32) for a, _, ca, _ in jobs])
    cib = np.concatenate([np.full(len(np.asarray(a).reshape(-1, 2)), cb, np.int32) for a, _, _, cb in jobs])
    xyz = _native.default_context().triangulate_pairs(cams, uva, uvb, cia, cib)
    out, o = [], 0
    for a, _, _, _ in jobs:
        n = len(np.asarray(a).reshape(-1, 2))
        out.append(xyz[o:o + n])
        o += n
    return out


def prepare_calib_board_data_for_bundle_adjustment(img_pts_arr, fnames_arr, board_shape, k_arr, d_arr, r_arr,
                                                   t_arr, triangulate_func=None):
    """`src/lib/sba.py:37-92`: every image name seen by at least two cameras contributes its
    board corners once per camera that saw it (u,v), one 3-D point per corner, initialised
    by triangulating the first two of those cameras. Returns (points_2d (n_obs,2) float32,
    points_3d (n_pts,3) float32, point_3d_indices, camera_indices).

    The reference walks the image names in the iteration order of a Python `set` of
    strings, which depends on PYTHONHASHSEED; here the order is sorted, so it is
    reproducible. Any order gives the same problem up to a permutation of the points."""
    n_cam = len(img_pts_arr)
    lists = [list(f) for f in fnames_arr]
    seen = {}
    for fnames in lists:
        for fn in set(fnames):
            seen[fn] = seen.get(fn, 0) + 1
    ppi = board_shape[0] * board_shape[1]
    points_2d, point_3d_indices, camera_indices, jobs = [], [], [], []
    counter = 0
    for fn in sorted(k for k, v in seen.items() if v >= 2):
        tri = []
        for cam in range(n_cam):
            if fn in lists[cam]:
                f_idx = lists[cam].index(fn)
                tri.append((cam, f_idx))
                points_2d.append(np.asarray(img_pts_arr[cam][f_idx]).reshape(ppi, 2))
                point_3d_indices.append(np.arange(counter, counter + ppi))
                camera_indices.append(np.full(ppi, cam))
        (a, a_pt), (b, b_pt) = tri[0], tri[1]
        jobs.append((img_pts_arr[a][a_pt], img_pts_arr[b][b_pt], a, b))
        counter += ppi
    points_3d = _triangulate_batch(jobs, k_arr, d_arr, r_arr, t_arr, triangulate_func)
    if not jobs:
        return (np.zeros((0, 2), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.int64),
                np.zeros(0, np.int64))
    return (np.concatenate(points_2d).astype(np.float32), np.concatenate(points_3d).astype(np.float32),
            np.concatenate(point_3d_indices).astype(np.int64), np.concatenate(camera_indices).astype(np.int64))


def prepare_manual_points_for_bundle_adjustment(img_pts_arr, k_arr, d_arr, r_arr, t_arr, triangulate_func=None):
    """`src/lib/sba.py:95-137`: img_pts_arr (n_points, n_cams, 2) with NaN where a camera did
    not label the point; a point seen by >= 2 cameras becomes one 3-D point initialised
    from its first two cameras. Returns the four arrays of the board variant."""
    pts = np.asarray(img_pts_arr).swapaxes(0, 1)  # (n_cams, n_points, 2)
    n_cam, n_pts = pts.shape[0], pts.shape[1]
    points_2d, point_3d_indices, camera_indices, jobs = [], [], [], []
    idx = 0
    for i in range(n_pts):
        cams = [c for c in range(n_cam) if not np.isnan(pts[c, i]).any()]
        if len(cams) > 1:
            points_2d.extend(pts[c, i] for c in cams)
            camera_indices.extend(cams)
            point_3d_indices.extend([idx] * len(cams))
            jobs.append((pts[cams[0], i], pts[cams[1], i], cams[0], cams[1]))
            idx += 1
    points_3d = _triangulate_batch(jobs, k_arr, d_arr, r_arr, t_arr, triangulate_func)
    return (np.array(points_2d, np.float32).reshape(-1, 2),
            (np.concatenate(points_3d) if points_3d else np.zeros((0, 3))).astype(np.float32),
            np.array(point_3d_indices, np.int64), np.array(camera_indices, np.int64))


def bundle_adjust_board_points_only(img_pts_arr, fnames_arr, board_shape, k_arr, d_arr, r_arr, t_arr,
                                    triangulate_func=None, project_func=None):
    """`src/lib/sba.py:196-204`."""
    p2, p3, pi, ci = prepare_calib_board_data_for_bundle_adjustment(img_pts_arr, fnames_arr, board_shape, k_arr,
                                                                    d_arr, r_arr, t_arr, triangulate_func)
    return bundle_adjust_points_only(p2, p3, pi, ci, k_arr, d_arr, r_arr, t_arr, project_func)


def _sba_board_points(scene_fpath, points_fpaths, manual_points_fpath, out_fpath, triangulate_func=None,
                      project_func=None, camera_indices=None, manual_points_only=False, covariance=False,
                      sigma_px=1.0):
    """`src/lib/sba.py:209-282`: board corners (+ optional hand-labelled points) -> joint
    points + extrinsics SBA -> refined scene JSON at out_fpath. Returns the residuals.
    `covariance=True` also writes `<out_fpath stem>_cov.json` beside it: the gauge and anchor
    pair, the per-camera 6 x 6 pose blocks over (dw, dt), the rotation (rad) and translation (m)
    sds, the covariance of every camera centre in world coordinates, sigma_hat_px and the
    status; the scene JSON is byte-equal to the plain call's.

    Kept as the reference has it: manual point indices are offset by the LAST board point
    index (`manual + board.max()`, :249), so the first manual point shares its index with
    the last board corner and the final initial 3-D point is unused."""
    img_pts_arr, fnames_arr, board_shape = [], [], None
    if camera_indices is None:
        camera_indices = range(len(points_fpaths))
    for i in camera_indices:
        points, fnames, board_shape, *_ = load_points(points_fpaths[i])
        img_pts_arr.append(points)
        fnames_arr.append(fnames)
    k_arr, d_arr, r_arr, t_arr, cam_res = load_scene(scene_fpath)
    assert len(k_arr) == len(img_pts_arr)
    if manual_points_fpath is not None:
        manual_points, _, *_ = load_manual_points(manual_points_fpath)
        m2, m3, mi, mc = prepare_manual_points_for_bundle_adjustment(manual_points, k_arr, d_arr, r_arr, t_arr,
                                                                     triangulate_func)
        if manual_points_only:
            print('bundle_adjust_board_points_and_extrinsics (with manual points only)')
            p2, p3, pi, ci = m2, m3, mi, mc
        else:
            print('bundle_adjust_board_points_and_extrinsics (with manual points)')
            p2, p3, pi, ci = prepare_calib_board_data_for_bundle_adjustment(img_pts_arr, fnames_arr, board_shape,
                                                                            k_arr, d_arr, r_arr, t_arr,
                                                                            triangulate_func)
            p2 = np.append(p2, m2, axis=0)
            p3 = np.append(p3, m3, axis=0)
            pi = np.append(pi, mi + pi.max(), axis=0)
            ci = np.append(ci, mc, axis=0)
    else:
        print('bundle_adjust_board_points_and_extrinsics')
        p2, p3, pi, ci = prepare_calib_board_data_for_bundle_adjustment(img_pts_arr, fnames_arr, board_shape, k_arr,
                                                                        d_arr, r_arr, t_arr, triangulate_func)
    obj_pts, r_arr, t_arr, res = bundle_adjust_points_and_extrinsics(p2, p3, pi, ci, k_arr, d_arr, r_arr, t_arr,
                                                                     project_func, covariance=covariance,
                                                                     sigma_px=sigma_px)
    print(f"\nBefore: mean: {np.mean(res['before'])}, std: {np.std(res['before'])}")
    print(f"After: mean: {np.mean(res['after'])}, std: {np.std(res['after'])}\n")
    save_scene(out_fpath, k_arr, d_arr, r_arr, t_arr, cam_res)
    if covariance:
        save_pose_covariance(os.path.splitext(out_fpath)[0] + '_cov.json', res, r_arr, t_arr, sigma_px)
    return res


def save_pose_covariance(fpath, res, r_arr, t_arr, sigma_px):
    """The `_cov.json` sibling of a refined scene file, from the residual dict of
    bundle_adjust_points_and_extrinsics(covariance=True)."""
    rep = res['cov_report']
    blocks = np.asarray(res['cov_cam_blocks'])
    sd = np.sqrt(np.diagonal(blocks, axis1=1, axis2=2))

    def lst(a):  # NaN (a degenerate problem) is not JSON: null
        return [lst(x) for x in a] if np.ndim(a) else (None if np.isnan(a) else float(a))

    data = dict(status=rep['status_name'], gauge=rep['gauge'], anchor=rep['anchor'], sigma_px=float(sigma_px),
                sigma_hat_px=lst(rep['sigma_hat_px']), dof=int(rep['dof']), min_pivot=lst(rep['min_pivot']),
                parameters='per camera (dw, dt): R <- exp([dw]x) R (rad), t <- t + dt (m)',
                cameras=[dict(cov=lst(blocks[c]), rotation_sd=lst(sd[c, :3]), translation_sd=lst(sd[c, 3:]),
                              centre=lst(camera_centres(r_arr, t_arr)[c]),
                              centre_cov=lst(camera_centre_covariance(blocks[c], r_arr[c], t_arr[c])))
                         for c in range(len(blocks))])
    with open(fpath, 'w') as f:
        json.dump(data, f, indent=2)


# ---- rigid-board bundle adjustment: one pose per board image (acs_sba_boards) -------------

def board_poses_from_points(obj_pts, pts_3d):
    """Rigid fit (Kabsch, det > 0) of the board model to triangulated corners: obj_pts (nc, 3) board
    coordinates, pts_3d (B, nc, 3) or (nc, 3) world points. Returns (board_r (B, 3, 3), board_t (B, 3))
    with X = R p + t in the least-squares sense. Host numpy: a one-off initialisation."""
    p = np.asarray(obj_pts, np.float64).reshape(-1, 3)
    X = np.asarray(pts_3d, np.float64).reshape(-1, len(p), 3)
    pm = p.mean(0)
    r_out, t_out = np.empty((len(X), 3, 3)), np.empty((len(X), 3))
    for b, Xb in enumerate(X):
        xm = Xb.mean(0)
        U, _, Vt = np.linalg.svd((Xb - xm).T @ (p - pm))
        R = U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt)) or 1.0]) @ Vt
        r_out[b] = R
        t_out[b] = xm - R @ pm
    return r_out, t_out


def prepare_calib_boards_for_bundle_adjustment(img_pts_arr, fnames_arr, board_shape, square_len, k_arr, d_arr, r_arr,
                                               t_arr):
    """The rigid-board form of prepare_calib_board_data_for_bundle_adjustment, with its image-name
    rule (sorted names, seen by at least two cameras): one board per such image. Returns
    (uv (B, C, nc, 2) float64, zero where unseen; mask (B, C) uint8; obj_pts (nc, 3); board_r (B, 3, 3);
    board_t (B, 3); names), the initial poses fitted (board_poses_from_points) to the corners
    triangulated from each board's first two cameras, all boards in one GPU batch."""
    from .utils import create_board_object_pts
    n_cam = len(img_pts_arr)
    lists = [list(f) for f in fnames_arr]
    seen = {}
    for fnames in lists:
        for fn in set(fnames):
            seen[fn] = seen.get(fn, 0) + 1
    names = sorted(k for k, v in seen.items() if v >= 2)
    nc = board_shape[0] * board_shape[1]
    obj = np.asarray(create_board_object_pts(board_shape, square_len), np.float64)
    uv = np.zeros((len(names), n_cam, nc, 2))
    mask = np.zeros((len(names), n_cam), np.uint8)
    jobs = []
    for b, fn in enumerate(names):
        cams = [c for c in range(n_cam) if fn in lists[c]]
        for c in cams:
            uv[b, c] = np.asarray(img_pts_arr[c][lists[c].index(fn)], np.float64).reshape(nc, 2)
            mask[b, c] = 1
        jobs.append((uv[b, cams[0]], uv[b, cams[1]], cams[0], cams[1]))
    pts = _triangulate_batch(jobs, k_arr, d_arr, r_arr, t_arr, None)
    if not jobs:
        return uv, mask, obj, np.zeros((0, 3, 3)), np.zeros((0, 3)), names
    board_r, board_t = board_poses_from_points(obj, np.stack(pts))
    return uv, mask, obj, board_r, board_t, names


def prepare_manual_points_dense(manual_points, k_arr, d_arr, r_arr, t_arr):
    """The dense form of prepare_manual_points_for_bundle_adjustment for the rigid-board SBA with free
    points, with its rule: manual_points (n_points, n_cams, 2) with NaN where a camera did not label
    the point; a point seen by >= 2 cameras is kept and initialised from its first two cameras, all of
    them in one GPU triangulation batch. Returns (pt_uv (n, C, 2) float64, zero where unseen; pt_mask
    (n, C) uint8; points_3d (n, 3) float64; kept, the indices of the kept points in the file). The
    points are a separate input of the solve, so the reference's index offset (`manual +
    board.max()`) has no counterpart here."""
    pts = np.asarray(manual_points, np.float64)
    if pts.ndim != 3 or pts.shape[2] != 2:
        raise ValueError(f'manual points must be (n_points, n_cams, 2), got {pts.shape}')
    if pts.shape[1] != len(k_arr):
        raise ValueError(f'manual points are labelled in {pts.shape[1]} cameras, the scene has {len(k_arr)}')
    seen = ~np.isnan(pts).any(axis=2)
    kept = np.nonzero(seen.sum(1) >= 2)[0]
    pt_mask = np.ascontiguousarray(seen[kept], np.uint8)
    pt_uv = np.where(pt_mask[:, :, None] != 0, pts[kept], 0.0)
    jobs = []
    for i in range(len(kept)):
        a, b = np.nonzero(pt_mask[i])[0][:2]
        jobs.append((pt_uv[i, a], pt_uv[i, b], int(a), int(b)))
    tri = _triangulate_batch(jobs, k_arr, d_arr, r_arr, t_arr, None)
    points_3d = np.concatenate(tri).astype(np.float64) if tri else np.zeros((0, 3))
    return pt_uv, pt_mask, points_3d, kept


def bundle_adjust_boards_and_extrinsics(uv, mask, obj_pts, board_r, board_t, k_arr, d_arr, r_arr, t_arr, f_scale=1.0,
                                        covariance=False, sigma_px=1.0, gauge='anchor', anchor=None, points_uv=None,
                                        points_mask=None, points_3d=None, **opts):
    """acs_sba_boards: every camera's rotation and translation (intrinsics fixed, fisheye model) and one
    rigid pose per board image refined together on the Cauchy objective of
    bundle_adjust_points_and_extrinsics. The known board geometry fixes the metric scale. uv
    (B, C, nc, 2), mask (B, C), obj_pts (nc, 3), board poses X = board_r p + board_t. Returns (board_r
    (B, 3, 3), board_t (B, 3), r_arr (C, 3, 3), t_arr (C, 3, 1), {'before', 'after', 'report'}); the
    residuals hold the seen views in (board, camera, corner, row) order. opts: max_iters, ftol, xtol,
    gtol, lambda0.
    `covariance=True` adds to the returned dict, evaluated at the returned solution with the same
    f_scale and the pixel noise `sigma_px` (acs_sba_boards_covariance): `cov_cams` (6C, 6C), camera
    c's (dw, dt) at rows 6c..6c+5 with R <- exp([dw]x) R (rad) and t <- t + dt (m); `cov_cam_blocks`
    (C, 6, 6), its diagonal blocks; `cov_boards` (B, 6, 6), every board pose's (dw_b, dt_b) (NaN for
    a board that is not OK); `cov_status` (B,) and `cov_report` (with 'gauge' and 'anchor'). gauge
    'anchor' holds the pose of camera `anchor` (default 0) and nothing else: the board fixes the
    scale; 'free' is the inner-constraint gauge. The poses and residuals are those of the plain
    call.
    With free points (points_uv (n, C, 2), points_mask (n, C), points_3d (n, 3): the arrays of
    prepare_manual_points_dense) they are solved in the same LM (acs_sba_boards_points). The 5-tuple
    keeps its shape; the dict gains `points_3d` (n, 3), the refined points, and `n_board_residuals`:
    `before` / `after` hold the board residuals up to it, then the seen (point, camera) pairs in
    (point, camera, row) order. Together with `covariance` this raises ValueError before any solve:
    acs_sba_boards_covariance describes the boards-only problem, and its answer would be silently too
    wide."""
    with_points = points_uv is not None or points_mask is not None or points_3d is not None
    if with_points and (points_uv is None or points_mask is None or points_3d is None):
        raise ValueError('points_uv, points_mask and points_3d go together')
    if with_points and covariance:
        raise ValueError('covariance=True describes the boards-only problem (acs_sba_boards_covariance): '
                         'not available together with free points')
    ctx = _native.default_context()
    n = len(k_arr)
    o = ctx.sba_ext_opts(f_scale=float(f_scale), **opts)
    t0 = time()
    if with_points:
        if np.shape(points_mask) != (len(np.asarray(points_3d).reshape(-1, 3)), n):
            raise ValueError(f'points_mask {np.shape(points_mask)} does not match {n} cameras and the points')
        cams, br, bt, px, rb, ra, rep = ctx.sba_boards_points(_cams(k_arr, d_arr, r_arr, t_arr), obj_pts, uv, mask,
                                                              board_r, board_t, points_uv, points_mask, points_3d, o)
    else:
        cams, br, bt, rb, ra, rep = ctx.sba_boards(_cams(k_arr, d_arr, r_arr, t_arr), obj_pts, uv, mask, board_r,
                                                   board_t, o)
    t1 = time()
    extra = f', {len(px)} free points with {int(np.count_nonzero(points_mask))} observations' if with_points else ''
    print(f'GPU SBA (boards + extrinsics): {len(br)} boards of {len(np.asarray(obj_pts).reshape(-1, 3))} corners, '
          f'{int(np.count_nonzero(mask))} views{extra}, {n} cameras, {rep["iters"]} iterations, cost '
          f'{rep["cost_before"]:.6e} -> {rep["cost_after"]:.6e} ({rep["status_name"]})')
    print(f'\nOptimization took {t1 - t0:.2f} seconds')
    r_out = cams[:, 8:17].reshape(n, 3, 3).copy()
    t_out = cams[:, 17:20].reshape(n, 3, 1).copy()
    res = dict(before=rb, after=ra, report=rep)
    if with_points:
        res.update(points_3d=px, n_board_residuals=2 * len(np.asarray(obj_pts).reshape(-1, 3))
                   * int(np.count_nonzero(mask)))
    if covariance:
        a = 0 if anchor is None else int(anchor)
        cc, cb, cst, crep = ctx.sba_boards_covariance(cams, obj_pts, uv, mask, br, bt, f_scale=float(f_scale),
                                                      sigma_px=float(sigma_px), gauge=gauge, anchor=a)
        crep.update(gauge=gauge, anchor=a if gauge == 'anchor' else None)
        print(f'GPU SBA board-rig covariance ({gauge}): {crep["status_name"]}, rotation sd <= '
              f'{crep["rot_sd_max"]:.3e} rad, translation sd <= {crep["trans_sd_max"]:.3e} m; sigma_hat '
              f'{crep["sigma_hat_px"]:.4f} px (sigma_px {float(sigma_px):g})')
        blocks = np.stack([cc[6 * c:6 * c + 6, 6 * c:6 * c + 6] for c in range(n)])
        res.update(cov_cams=cc, cov_cam_blocks=blocks, cov_boards=cb, cov_status=cst, cov_report=crep)
    return br, bt, r_out, t_out, res


def _sba_board_poses(scene_fpath, points_fpaths, out_fpath, camera_indices=None, covariance=False, sigma_px=1.0,
                     manual_points_fpath=None):
    """Board corners -> rigid-board SBA (bundle_adjust_boards_and_extrinsics) -> refined scene JSON at
    out_fpath and `<out_fpath stem>_boards.json` beside it: per board image its name, pose (r, t) and
    view count, and the report. The square length is the points files'. Returns the residual dict.
    `covariance=True` also writes `<out_fpath stem>_cov.json` (save_pose_covariance: camera 0 held,
    nothing else; camera blocks, sds, centres and centre covariances) and gives each board entry of
    `_boards.json` its `cov` (6 x 6, (dw_b, dt_b)), `rotation_sd`, `translation_sd` and `status`
    (NaN written as null). The scene file is the same either way.
    `manual_points_fpath`: the hand-labelled points of that file (prepare_manual_points_dense) are free
    points of the same solve; `_boards.json` gains `manual_points`: per kept point its index in the
    file, refined `xyz` and `n_views`, and `report` covers the mixed solve. ValueError, before anything
    is solved or written, together with `covariance` or when the file's camera count is not the
    scene's. Without a file every output file is byte-equal to the call without the argument."""
    if manual_points_fpath is not None and covariance:
        raise ValueError('covariance=True describes the boards-only problem: not available together with '
                         'manual_points_fpath')
    img_pts_arr, fnames_arr, board_shape, square_len = [], [], None, None
    if camera_indices is None:
        camera_indices = range(len(points_fpaths))
    for i in camera_indices:
        points, fnames, board_shape, square_len, *_ = load_points(points_fpaths[i])
        img_pts_arr.append(points)
        fnames_arr.append(fnames)
    k_arr, d_arr, r_arr, t_arr, cam_res = load_scene(scene_fpath)
    assert len(k_arr) == len(img_pts_arr)
    print('bundle_adjust_boards_and_extrinsics')
    uv, mask, obj, br, bt, names = prepare_calib_boards_for_bundle_adjustment(img_pts_arr, fnames_arr, board_shape,
                                                                              square_len, k_arr, d_arr, r_arr, t_arr)
    kw = dict(covariance=True, sigma_px=sigma_px) if covariance else {}
    kept = None
    if manual_points_fpath is not None:
        manual_points, _, *_ = load_manual_points(manual_points_fpath)
        pt_uv, pt_mask, pts_3d, kept = prepare_manual_points_dense(manual_points, k_arr, d_arr, r_arr, t_arr)
        kw.update(points_uv=pt_uv, points_mask=pt_mask, points_3d=pts_3d)
    br, bt, r_arr, t_arr, res = bundle_adjust_boards_and_extrinsics(uv, mask, obj, br, bt, k_arr, d_arr, r_arr, t_arr,
                                                                    **kw)
    print(f"\nBefore: mean: {np.mean(res['before'])}, std: {np.std(res['before'])}")
    print(f"After: mean: {np.mean(res['after'])}, std: {np.std(res['after'])}\n")
    save_scene(out_fpath, k_arr, d_arr, r_arr, t_arr, cam_res)
    rep = {k: v for k, v in res['report'].items() if isinstance(v, (int, float, str))}
    data = dict(board_shape=list(board_shape), board_square_len=float(square_len),
                parameters='per board X = r p + t: board coordinates to world coordinates (m)',
                boards=[dict(name=fn, r=br[b].tolist(), t=bt[b].tolist(), n_views=int(mask[b].sum()))
                        for b, fn in enumerate(names)], report=rep)
    if kept is not None:
        data['manual_points'] = [dict(index=int(i), xyz=res['points_3d'][k].tolist(), n_views=int(pt_mask[k].sum()))
                                 for k, i in enumerate(kept)]
        res.update(points_uv=pt_uv, points_mask=pt_mask, points_kept=kept)
    if covariance:
        save_pose_covariance(os.path.splitext(out_fpath)[0] + '_cov.json', res, r_arr, t_arr, sigma_px)
        names_st = ('ok', 'noobs', 'degenerate')

        def lst(a):  # NaN (a board that is not OK, a degenerate problem) is not JSON: null
            return [lst(x) for x in a] if np.ndim(a) else (None if np.isnan(a) else float(a))
        for b, entry in enumerate(data['boards']):
            blk = res['cov_boards'][b]
            sd = np.sqrt(blk.diagonal())
            entry.update(cov=lst(blk), rotation_sd=lst(sd[:3]), translation_sd=lst(sd[3:]),
                         status=names_st[int(res['cov_status'][b])])
    with open(os.path.splitext(out_fpath)[0] + '_boards.json', 'w') as f:
        json.dump(data, f, indent=2)
    res.update(board_r=br, board_t=bt, names=names, mask=mask, uv=uv, obj_pts=obj)
    return res
