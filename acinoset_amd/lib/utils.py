"""Mirror of src/lib/utils.py I/O used on the SBA / FTE path (formats kept: scene JSON,
DLC long DataFrame, pickle + .mat outputs).

`get_pairwise_3d_points_from_df` (:319-349) triangulates on the GPU. DLC `.h5` input
needs PyTables (pandas.read_hdf); where it is absent, `load_dlc_points_as_df` raises a
clear ImportError and `.csv` DLC exports are accepted instead.
"""
import json
import os
import pickle
from datetime import datetime
from errno import ENOENT
from glob import glob

import numpy as np
import pandas as pd

from .. import _native


def load_points(fpath, verbose=False):
    """`src/lib/utils.py:18-28`: checkerboard corners JSON -> (points (n_img, n_corner, 1, 2)
    float32, fnames, board_shape, board_square_len, cam_res)."""
    with open(fpath) as f:
        data = json.load(f)
    fnames = list(data['points'].keys())
    points = np.array(list(data['points'].values()), dtype=np.float32)
    board_shape = tuple(data['board_shape'])
    board_square_len = data['board_square_len']
    cam_res = tuple(data['camera_resolution'])
    if verbose:
        print(f'Loaded checkerboard points from {fpath}\n')
    return points, fnames, board_shape, board_square_len, cam_res


def load_manual_points(fpath, verbose=True):
    """`src/lib/utils.py:31-41`: hand-labelled points JSON -> (points (n_pts, n_cams, 2),
    fnames 'imgNNNNN.jpg', cam_res)."""
    with open(fpath) as f:
        data = json.load(f)
    points = np.array(data['points'])
    fnames = [f'img{str(i).zfill(5)}.jpg' for i in data['frame_idx']]
    cam_res = tuple(data['camera_resolution'])
    if verbose:
        print(f'Loaded manual points from {fpath}\n')
    return points, fnames, cam_res


def load_camera(fpath, verbose=False):
    """`src/lib/utils.py:44-52`: intrinsics JSON -> (k (3,3), d (4,1), cam_res)."""
    with open(fpath) as f:
        data = json.load(f)
    cam_res = tuple(data['camera_resolution'])
    k = np.array(data['k'], dtype=np.float64)
    d = np.array(data['d'], dtype=np.float64)
    if verbose:
        print(f'Loaded intrinsics from {fpath}\n')
    return k, d, cam_res


def save_points(out_fpath, img_points, img_fnames, board_shape, board_square_len, cam_res):
    """`src/lib/utils.py:156-170`."""
    if isinstance(img_points, np.ndarray):
        img_points = img_points.tolist()
    data = {'timestamp': str(datetime.now()), 'board_shape': board_shape, 'board_square_len': board_square_len,
            'camera_resolution': cam_res, 'points': dict(zip(img_fnames, img_points))}
    with open(out_fpath, 'w') as f:
        json.dump(data, f)
    print(f'Saved points to {out_fpath}\n')


def save_camera(out_fpath, cam_res, k, d):
    """`src/lib/utils.py:173-183`."""
    data = {'timestamp': str(datetime.now()), 'camera_resolution': cam_res, 'k': np.asarray(k).tolist(),
            'd': np.asarray(d).tolist()}
    with open(out_fpath, 'w') as f:
        json.dump(data, f)
    print(f'Saved intrinsics to {out_fpath}\n')


def load_scene(fpath, verbose=True):
    """`src/lib/utils.py:55-74` -> (k_arr (C,3,3), d_arr (C,4,1), r_arr, t_arr (C,3,1), cam_res)."""
    with open(fpath) as f:
        data = json.load(f)
    cam_res = tuple(data['camera_resolution'])
    k = np.array([c['k'] for c in data['cameras']], dtype=np.float64)
    d = np.array([c['d'] for c in data['cameras']], dtype=np.float64)
    r = np.array([c['r'] for c in data['cameras']], dtype=np.float64)
    t = np.array([c['t'] for c in data['cameras']], dtype=np.float64)
    if verbose:
        print(f'Loaded extrinsics from {fpath}\n')
    return k, d, r, t, cam_res


def save_scene(out_fpath, k_arr, d_arr, r_arr, t_arr, cam_res):
    """`src/lib/utils.py:186-203`."""
    cams = [{'k': np.asarray(k).tolist(), 'd': np.asarray(d).tolist(), 'r': np.asarray(r).tolist(),
             't': np.asarray(t).tolist()} for k, d, r, t in zip(k_arr, d_arr, r_arr, t_arr)]
    with open(out_fpath, 'w') as f:
        json.dump({'timestamp': str(datetime.now()), 'camera_resolution': cam_res, 'cameras': cams}, f)
    print(f'Saved extrinsics to {out_fpath}\n')


def find_scene_file(dir_path, scene_fname=None, verbose=True):
    """`src/lib/utils.py:290-310`."""
    if scene_fname is None:
        n_cams = len(glob(os.path.join(dir_path, 'cam[1-9].mp4')))
        scene_fname = f'{n_cams}_cam_scene_sba.json' if n_cams else '[1-9]_cam_scene*.json'
    if dir_path and dir_path != os.path.join('..', 'data'):
        scene_fpath = os.path.join(dir_path, 'extrinsic_calib', scene_fname)
        files = sorted([f for f in glob(scene_fpath) if ('before_corrections' not in f) or (f == scene_fpath)])
        if files:
            k, d, r, t, res = load_scene(files[-1], verbose)
            n_cams = int(os.path.basename(files[-1])[0])
            return k, d, r, t, res, n_cams, files[-1]
        return find_scene_file(os.path.dirname(dir_path), scene_fname, verbose)
    raise FileNotFoundError(ENOENT, os.strerror(ENOENT), os.path.join('extrinsic_calib', scene_fname))


def _read_dlc(path):
    if path.endswith('.csv'):
        return pd.read_csv(path, header=[0, 1, 2], index_col=0)
    try:
        return pd.read_hdf(path)
    except ImportError as e:  # PyTables missing
        raise ImportError(f'reading {path} needs PyTables (pandas.read_hdf); export the DLC file as .csv '
                          'or install tables') from e


# the head-detector outputs (`dlc_head` in the first path, src/lib/utils.py:84-103): three
# generic body parts renamed, a fourth ('objectA') dropped, markers kept in this order
DLC_HEAD_PARTS = {'bodypart1': 'r_eye', 'bodypart2': 'l_eye', 'bodypart3': 'nose'}
DLC_HEAD_ORDER = ('nose', 'r_eye', 'l_eye')


def _frame_from_label(label):
    """DLC image-path row label 'labeled-data/.../img0042.png' -> 42 (`int(s[-7:-4])`). An
    integer label (a video-analysis row number) is kept; the reference would fail on it."""
    if isinstance(label, (int, np.integer)):
        return int(label)
    return int(str(label)[-7:-4])


def load_dlc_points_as_df(dlc_df_fpaths, frame_shifts=None, verbose=False):
    """`src/lib/utils.py:77-151`: per-camera DLC tables (scorer/bodyparts/coords columns) ->
    long DataFrame [frame, camera, marker, x, y, likelihood], camera-major, then frame, then
    marker. Pinned to the reference function itself by `tests/golden/dlc.npz`. Three input
    branches, as in the reference:
    * a likelihood column present: rows keep their index as the frame, markers sorted (the
      reference's `.T.unstack().T` orders the bodyparts level, :120);
    * no likelihood column (:104-117): likelihood = 1 where y is present, 0 where it is NaN;
      the frame is parsed from the image-path row label;
    * `dlc_head` in the FIRST path (:84-103, applied to every file): bodypart1/2/3 renamed
      r_eye/l_eye/nose, objectA dropped, likelihood = 1 where x is present, markers in the
      order nose, r_eye, l_eye, frames from the row labels.
    A frame shift moves every marker's (x, y, likelihood) by that many frames; the frames
    shifted in are NaN with likelihood 0 and the frame column is not shifted (:124-137)."""
    assert frame_shifts is None or len(dlc_df_fpaths) == len(frame_shifts), \
        '`frame_shifts` should be the same size with `dlc_df_fpaths`'
    head = len(dlc_df_fpaths) > 0 and 'dlc_head' in dlc_df_fpaths[0]
    out = []
    for i, path in enumerate(dlc_df_fpaths):
        df = _read_dlc(path)
        df = df.droplevel(0, axis=1)                        # scorer
        coords = set(df.columns.get_level_values(1))
        idx = df.index
        if head:
            df = df.rename(columns=DLC_HEAD_PARTS, level=0)
            parts = list(DLC_HEAD_ORDER)
            lik_from = 'x'
            frames = np.array([_frame_from_label(s) for s in idx])
        elif 'likelihood' not in coords:
            parts = sorted(dict.fromkeys(df.columns.get_level_values(0)))
            lik_from = 'y'
            frames = np.array([_frame_from_label(s) for s in idx])
        else:
            parts = sorted(dict.fromkeys(df.columns.get_level_values(0)))
            lik_from = None
            frames = np.asarray(idx)
        shift = 0 if frame_shifts is None else int(frame_shifts[i])
        n, L = len(frames), len(parts)
        vals = np.full((3, n, L), np.nan)
        for j, bp in enumerate(parts):
            vals[0, :, j] = df[(bp, 'x')].to_numpy(np.float64)
            vals[1, :, j] = df[(bp, 'y')].to_numpy(np.float64)
            if lik_from is None:
                vals[2, :, j] = df[(bp, 'likelihood')].to_numpy(np.float64)
            else:
                vals[2, :, j] = np.isfinite(vals[0 if lik_from == 'x' else 1, :, j])
        if shift:
            sh = np.full_like(vals, np.nan)
            if shift > 0:
                sh[:, shift:] = vals[:, :n - shift]
            else:
                sh[:, :n + shift] = vals[:, -shift:]
            vals = sh
        out.append(pd.DataFrame({'frame': np.repeat(frames, L), 'camera': i, 'marker': np.tile(parts, n),
                                 'x': vals[0].ravel(), 'y': vals[1].ravel(),
                                 'likelihood': np.nan_to_num(vals[2].ravel())}))
    dlc = pd.concat(out, ignore_index=True)[['frame', 'camera', 'marker', 'x', 'y', 'likelihood']]
    if verbose:
        print(f'DLC points dataframe:\n{dlc}\n')
    return dlc


def save_optimised_cheetah(positions, out_fpath, extra_data=None, for_matlab=True, save_as_csv=False):
    """`src/lib/utils.py:206-234`: pickle {positions, **extra} (+ .mat)."""
    file_data = dict(positions=positions)
    if extra_data is not None:
        assert type(extra_data) is dict
        file_data.update(extra_data)
    with open(out_fpath, 'wb') as f:
        pickle.dump(file_data, f)
    print('Saved', out_fpath)
    if for_matlab:
        from scipy.io import savemat
        mat = {k: v for k, v in file_data.items() if not isinstance(v, dict)}
        savemat(os.path.splitext(out_fpath)[0] + '.mat', mat)
        print('Saved', os.path.splitext(out_fpath)[0] + '.mat')


def _write_h5(df, fpath, key):
    """`DataFrame.to_hdf(format='table')` where pandas can (PyTables installed); otherwise
    the .csv beside it is the output. Returns whether the .h5 was written."""
    try:
        df.to_hdf(fpath, key=key, format='table', mode='w')
        return True
    except ImportError:
        return False


def save_3d_cheetah_as_2d(position3d_arr, out_dir, scene_fpath, bodyparts, project_func, start_frame,
                          save_as_csv=True, out_fname=None):
    """`src/lib/utils.py:237-286`: reproject 3-D markers into every camera as DLC-format
    tables, `cam{n}_{out_fname}.h5` (+ `.csv`), one per `cam[1-9].mp4` found in `out_dir`
    or its parent. Columns are (bodyparts × [x, y, likelihood]) with likelihood NaN; a
    projection with u or v outside [0, cam_res] is NaN in both. `position3d_arr` is one
    (n_frames, L, 3) array for every camera or a per-camera list (the FTE's shutter-delay
    shifted positions). `project_func` is the GPU projection (`calib.project_points_fisheye`)
    in the drop-in; any callable with the reference's signature works. Without PyTables the
    `.h5` is skipped (said once) and the `.csv` is written whatever `save_as_csv` says.
    Returns the per-camera DataFrames ([] when no video is found)."""
    assert os.path.dirname(os.path.dirname(scene_fpath)) in out_dir, \
        'scene_fpath does not belong to the same parent folder as out_dir'
    video_fpaths = sorted(glob(os.path.join(out_dir, 'cam[1-9].mp4')))
    if not video_fpaths:
        video_fpaths = sorted(glob(os.path.join(os.path.dirname(out_dir), 'cam[1-9].mp4')))
    if not video_fpaths:
        print('Could not save 3D cheetah to 2D - No videos were found in', out_dir, 'or', os.path.dirname(out_dir))
        return []
    k_arr, d_arr, r_arr, t_arr, cam_res = load_scene(scene_fpath, verbose=False)
    assert len(k_arr) == len(video_fpaths)
    if not isinstance(position3d_arr, list):
        position3d_arr = [position3d_arr] * len(video_fpaths)
    pdindex = pd.MultiIndex.from_product([list(bodyparts), ['x', 'y', 'likelihood']], names=['bodyparts', 'coords'])
    out_fname = os.path.basename(out_dir) if out_fname is None else out_fname
    res = np.asarray(cam_res, np.float64)
    result_dfs, h5_ok = [], True
    for i, vid in enumerate(video_fpaths):
        position3d = np.asarray(position3d_arr[i], np.float64)
        n_frames = len(position3d)
        prj = np.array(project_func(position3d, k_arr[i], d_arr[i], r_arr[i], t_arr[i]), np.float64).reshape(-1, 2)
        with np.errstate(invalid='ignore'):
            out = ((prj > res) | (prj < 0.0)).any(axis=1)
        prj[out] = np.nan
        data = np.full(position3d.shape, np.nan)
        data[:, :, 0:2] = prj.reshape((n_frames, -1, 2))
        cam_name = os.path.splitext(os.path.basename(vid))[0]
        fpath = os.path.join(out_dir, f'{cam_name}_{out_fname}.h5')
        df = pd.DataFrame(data.reshape((n_frames, -1)), columns=pdindex, index=range(start_frame, start_frame + n_frames))
        h5_ok = _write_h5(df, fpath, f'{out_fname}_df') and h5_ok
        if save_as_csv or not h5_ok:
            df.to_csv(os.path.splitext(fpath)[0] + '.csv')
        result_dfs.append(df)
    pattern = os.path.join(out_dir, f'cam*_{out_fname}')
    print('Saved', pattern + ('.h5' if h5_ok else '.csv (no PyTables: .h5 skipped)'))
    if save_as_csv and h5_ok:
        print('Saved', pattern + '.csv')
    print()
    return result_dfs


def create_board_object_pts(board_shape, square_edge_length):
    obj = np.zeros((board_shape[0] * board_shape[1], 3), np.float32)
    obj[:, :2] = np.mgrid[0:board_shape[0], 0:board_shape[1]].T.reshape(-1, 2) * square_edge_length
    return obj


def get_pairwise_3d_points_from_df(points_2d_df, k_arr, d_arr, r_arr, t_arr, triangulate_func=None, verbose=True):
    """`src/lib/utils.py:319-349` with the GPU triangulation: for adjacent camera pairs
    (i, i+1 mod C), inner join on (frame, marker), triangulate, then mean per
    (frame, marker) in pair order. Returns [frame, marker, x, y, z] sorted by
    (frame, marker) like the reference's groupby. `triangulate_func is calib.triangulate_points`
    selects the standard model (d_arr then holds 4, 5 or 8 coefficients per camera); None,
    `calib.triangulate_points_fisheye` and any other callable (never called) the fisheye model."""
    from . import calib
    n_cams = len(k_arr)
    if triangulate_func is calib.triangulate_points:
        cams = _native.pack_cameras_standard(k_arr, d_arr, r_arr, t_arr)
    else:
        cams = _native.pack_cameras(k_arr, np.asarray(d_arr).reshape(-1, 4), r_arr, t_arr)
    parts = []
    for ca in range(n_cams):
        cb = (ca + 1) % n_cams
        d0 = points_2d_df[points_2d_df['camera'] == ca]
        d1 = points_2d_df[points_2d_df['camera'] == cb]
        j = d0.merge(d1, how='inner', on=['frame', 'marker'], suffixes=('_a', '_b'))
        if j.shape[0] > 0:
            if verbose:
                print(f'Found {j.shape[0]} pairwise points between camera {ca} and {cb}')
            parts.append((j, ca, cb))
        elif verbose:
            print(f'No pairwise points between camera {ca} and {cb}')
    if verbose:
        print()
    if not parts:
        return pd.DataFrame(columns=['frame', 'marker', 'x', 'y', 'z'])
    uva = np.concatenate([p[0][['x_a', 'y_a']].to_numpy(np.float64) for p in parts])
    uvb = np.concatenate([p[0][['x_b', 'y_b']].to_numpy(np.float64) for p in parts])
    cia = np.concatenate([np.full(len(p[0]), p[1], np.int32) for p in parts])
    cib = np.concatenate([np.full(len(p[0]), p[2], np.int32) for p in parts])
    xyz = _native.default_context().triangulate_pairs(cams, uva, uvb, cia, cib)
    frames = np.concatenate([p[0]['frame'].to_numpy() for p in parts])
    markers = np.concatenate([p[0]['marker'].to_numpy() for p in parts])
    df = pd.DataFrame({'frame': frames, 'marker': markers, 'x': xyz[:, 0], 'y': xyz[:, 1], 'z': xyz[:, 2]})
    return df.groupby(['frame', 'marker']).mean().reset_index()
