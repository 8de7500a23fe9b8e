"""`core.sba` (src/core/sba.py:27-70): filter by likelihood and frame window, GPU SBA,
reprojection metric, sba.pickle. `camera_model='standard'` runs the solve, the metric and the
2-D export through the standard (pinhole) model (`lib.app.sba_points_standard`).
`covariance=True` adds the per-point position covariance (acs_sba_points_covariance at the solved
points, pixel noise `sigma_px`) to sba.pickle / .mat: `positions_cov` (N, L, 3, 3) in m^2 and
`positions_cov_status` (N, L) int8 in the order of `misc.get_markers()` (no direction markers;
NaN / -1 where there is no point, NaN where the status is not 0), `sigma_px` and `sigma_hat_px`."""
import json
import os
from typing import Dict

import numpy as np

from ..lib import app, calib, metric, misc


def sba(DATA_DIR, points_2d_df, start_frame, end_frame, dlc_thresh, camera_params, scene_fpath, params: Dict = {},
        plot: bool = False, camera_model: str = 'fisheye', covariance: bool = False, sigma_px: float = 1.0) -> str:
    if camera_model not in ('fisheye', 'standard'):
        raise ValueError(f"camera_model must be 'fisheye' or 'standard', not {camera_model!r}")
    standard = camera_model == 'standard'
    OUT_DIR = os.path.join(DATA_DIR, 'sba')
    os.makedirs(OUT_DIR, exist_ok=True)
    app.start_logging(os.path.join(OUT_DIR, 'sba.log'))
    markers = misc.get_markers()
    params = dict(params)
    params.update(start_frame=start_frame, end_frame=end_frame, dlc_thresh=dlc_thresh)
    with open(os.path.join(OUT_DIR, 'reconstruction_params.json'), 'w') as f:
        json.dump(params, f)
    points_2d_df = points_2d_df.query(f'likelihood > {dlc_thresh}')
    points_2d_df = points_2d_df[points_2d_df['frame'].between(start_frame, end_frame)]
    try:
        solve = app.sba_points_standard if standard else app.sba_points_fisheye
        points_3d_df, residuals = solve(scene_fpath, points_2d_df, covariance=covariance, sigma_px=sigma_px)
    finally:
        app.stop_logging()
    project_func = calib.project_points if standard else None
    pix_errors = metric.residual_error(points_2d_df, points_3d_df, markers, camera_params, project_func)
    print(f'reprojection RMS: {metric.reprojection_rms(pix_errors):.4f} px')
    positions = np.full((end_frame - start_frame + 1, len(markers), 3), np.nan)
    mi = {m: i for i, m in enumerate(markers)}
    fr = points_3d_df['frame'].to_numpy().astype(int) - start_frame
    mk = np.array([mi[m] for m in points_3d_df['marker']])
    positions[fr, mk] = points_3d_df[['x', 'y', 'z']].to_numpy()
    extra = None
    if covariance:
        positions_cov = np.full(positions.shape[:2] + (3, 3), np.nan)
        positions_cov_status = np.full(positions.shape[:2], -1, np.int8)
        positions_cov[fr, mk] = residuals['cov']
        positions_cov_status[fr, mk] = residuals['cov_status']
        extra = dict(positions_cov=positions_cov, positions_cov_status=positions_cov_status, sigma_px=float(sigma_px),
                     sigma_hat_px=float(residuals['cov_report']['sigma_hat_px']))
    return app.save_sba(positions, OUT_DIR, scene_fpath, markers, start_frame, project_func=project_func, extra=extra)
