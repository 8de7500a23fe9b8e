"""Standard (pinhole) camera model, no GPU: the numpy helper against the reference's golden
vectors (tests/golden/standard.npz, written by make_golden_standard.py), the monkeypatched
oracle LM against the reference's scipy solution, the camera packer and the header.

Tolerances: the helper restates the formulas the fixture was computed with (1e-9 px, 1e-9 m:
rounding only); oracle LM against scipy TRF (stops on xtol 1e-8) within the project's
1e-6 m RMS / 1e-5 m max (test_gpu_core.py).
"""
import os
import re

import numpy as np
import pytest

import standard_model as sm
from conftest import REPO, golden
from acinoset_amd import _native


@pytest.fixture(scope='module')
def g():
    return golden('standard')


def test_helper_projection_matches_fixture(g):
    n, C = g['proj_uv'].shape[:2]
    for c in range(C):
        uv = sm.project(g['proj_X'], g['K'][c], g['D'][c], g['R'][c], g['t'][c])
        np.testing.assert_allclose(uv, g['proj_uv'][:, c], rtol=0, atol=1e-9)
    uv5 = sm.project(g['proj_X'], g['K'][0], g['D'][0, :5], g['R'][0], g['t'][0])
    np.testing.assert_allclose(uv5, g['proj5_uv'], rtol=0, atol=1e-9)
    assert np.abs(uv5 - g['proj_uv'][:, 0]).max() > 1e-3   # k4..k6 do something


def test_helper_jacobian_matches_central_differences(g):
    rng = np.random.default_rng(0)
    X = g['proj_X'][::7]
    ci = rng.integers(0, 6, len(X))
    args = (g['K'][ci], g['D'][ci], g['R'][ci], g['t'][ci])
    _, J = sm.project_jac(X, *args)
    h = 1e-6
    for j in range(3):
        e = np.zeros(3)
        e[j] = h
        fd = (sm.project(X + e, *args) - sm.project(X - e, *args)) / (2 * h)
        np.testing.assert_allclose(J[:, :, j], fd, rtol=1e-7, atol=1e-6)


def test_helper_triangulation_matches_fixture(g):
    K, D, R, t = g['K'], g['D'], g['R'], g['t']
    xyz = sm.triangulate_pair(g['pair_a'], g['pair_b'], K[0], D[0], R[0], t[0], K[1], D[1], R[1], t[1])
    np.testing.assert_allclose(xyz, g['pair_xyz'], rtol=0, atol=1e-9)
    # five iterations are what OpenCV runs, not convergence: ten land elsewhere
    x5 = sm.undistort(g['pair_a'], K[0], D[0])
    x10 = sm.undistort(g['pair_a'], K[0], D[0], iters=10)
    gap = np.abs(x5 - x10).max()
    print('undistort, 5 against 10 iterations: %.3e (normalised)' % gap)
    assert 0 < gap < 1e-4


def test_oracle_with_standard_projection_matches_scipy(g, monkeypatch):
    osba = sm.patch_oracle(monkeypatch, g['D'])
    for tag in ('a', 'b'):
        p3 = g['a_points_3d'] if tag == 'a' else g['b_tri']
        ref, info = osba.sba_points(g[f'{tag}_points_2d'], p3, g[f'{tag}_point_indices'], g[f'{tag}_camera_indices'],
                                    g['K'], sm.oracle_stand_in(6), g['R'], g['t'], return_info=True)
        d = ref - g[f'{tag}_scipy']
        rms, mx = np.sqrt(np.mean(np.sum(d ** 2, 1))), np.abs(d).max()
        print('%s: oracle vs scipy %.3e m RMS, %.3e m max (generator: %.3e, %.3e)' % (
            tag, rms, mx, g[f'{tag}_oracle_rms'], g[f'{tag}_oracle_max']))
        assert rms < 1e-6 and mx < 1e-5
        assert info['iters'].max() <= 6
        assert set(np.unique(info['status'])) <= {osba.FTOL, osba.XTOL}
    # the residual vector at the start is the reference's own
    r = osba.cost_func_points_only(g['a_points_3d'].ravel(), len(g['a_points_3d']), g['a_point_indices'],
                                   g['a_camera_indices'], g['K'], sm.oracle_stand_in(6), g['R'], g['t'],
                                   g['a_points_2d'])
    np.testing.assert_allclose(r, g['a_resid_before'], rtol=0, atol=1e-9)


def test_pack_cameras_standard_layout_and_padding(g):
    K, D, R, t = g['K'], g['D'], g['R'], g['t']
    cams = _native.pack_cameras_standard(K, D, R, t)
    assert cams.shape == (6, _native.ACS_CAM_STRIDE_STD) == (6, 24)
    np.testing.assert_array_equal(cams[:, :4], np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], 1))
    np.testing.assert_array_equal(cams[:, 4:12], D)
    np.testing.assert_array_equal(cams[:, 12:21], R.reshape(6, 9))
    np.testing.assert_array_equal(cams[:, 21:], t.reshape(6, 3))
    for n in (4, 5):
        for shape in ((6, n), (6, n, 1), (6, 1, n)):
            c = _native.pack_cameras_standard(K, D[:, :n].reshape(shape), R, t.reshape(6, 3))
            np.testing.assert_array_equal(c[:, 4:4 + n], D[:, :n])
            np.testing.assert_array_equal(c[:, 4 + n:12], 0.0)
            np.testing.assert_array_equal(c[:, 12:], cams[:, 12:])
    for n in (12, 14):
        wide = np.zeros((6, n))
        wide[:, :8] = D
        np.testing.assert_array_equal(_native.pack_cameras_standard(K, wide, R, t), cams)
        wide[3, n - 1] = 1e-3
        with pytest.raises(ValueError, match='thin-prism.*tilt'):
            _native.pack_cameras_standard(K, wide, R, t)
    for n in (3, 6, 7, 9):
        with pytest.raises(ValueError, match='distortion coefficients'):
            _native.pack_cameras_standard(K, np.zeros((6, n)), R, t)


def test_record_width_selects_the_model():
    ok20, f20 = _native._cams_flags(np.zeros((2, 20)))
    ok24, f24 = _native._cams_flags(np.zeros((2, 24)))
    assert (f20, f24) == (0, _native.ACS_CAMS_STANDARD)
    for bad in (np.zeros((2, 21)), np.zeros(20), np.zeros((2, 3, 8))):
        with pytest.raises(ValueError, match='camera records'):
            _native._cams_flags(bad)


def test_header_declares_the_standard_model():
    with open(os.path.join(REPO, 'include', 'acinoset_hip.h')) as f:
        h = f.read()
    assert re.search(r'^#define\s+ACS_CAM_STRIDE_STD\s+24\b', h, re.M)
    assert re.search(r'^#define\s+ACS_CAMS_STANDARD\s+2u\b', h, re.M)
    assert re.search(r'^int\s+acs_project_standard\s*\(', h, re.M)
    assert re.search(r'^#define\s+ACS_ABI_VERSION\s+5\b', h, re.M)   # additive: the version stays
    assert 'acs_project_standard' in _native.SYMBOLS
    assert (_native.ACS_CAM_STRIDE_STD, _native.ACS_CAMS_STANDARD) == (24, 2)


def test_standard_functions_select_the_model():
    from acinoset_amd.lib import calib, sba
    assert sba.is_standard_model(calib.project_points) and sba.is_standard_model(calib.triangulate_points)
    for f in (None, calib.project_points_fisheye, calib.triangulate_points_fisheye, lambda *a: None):
        assert not sba.is_standard_model(f)
    with pytest.raises(NotImplementedError, match='standard camera model'):
        sba.bundle_adjust_points_and_extrinsics(None, None, None, None, None, None, None, None,
                                                project_func=calib.project_points)
