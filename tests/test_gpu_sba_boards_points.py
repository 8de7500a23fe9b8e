"""GPU: the rigid-board bundle adjustment with free points (acs_sba_boards_points) against its numpy
restatement (sba_boards_points_ref.py, the same LM iterate for iterate) at the tolerances
test_gpu_sba_boards.py uses: status, iterations and acceptances equal, lambda and both costs 1e-12
relative, rotations 1e-10, translations and points 1e-9 m, residuals before 1e-9 and after 1e-8 px,
R R^T = I to 1e-12, intrinsics untouched. The problems are sba_boards_points_ref.PROBLEMS: every decision
of the compared iterations is at least 1e-9 from a tie in the helper's trace
(test_sba_boards_points_cpu.py)."""
import json
import os

import numpy as np
import pytest

import sba_boards_points_ref as ref
import sba_ext_shapes as sh
from acinoset_amd import _native
from acinoset_amd.lib import sba as lsba
from acinoset_amd.lib import utils as lutils

pytestmark = pytest.mark.gpu

_HELPER = {}


def _cams0(rig, start):
    return _native.pack_cameras(rig['K'], rig['D'], start[0], start[1])


def _gpu(ctx, rig, start, **opts):
    R0, t0, bR0, bt0, X0 = start
    return ctx.sba_boards_points(_cams0(rig, start), rig['obj'], rig['uv'], rig['mask'], bR0, bt0, rig['pt_uv'],
                                 rig['pt_mask'], X0, ctx.sba_ext_opts(**opts))


def _helper(key, rig, start, **kw):
    """The helper's solve, computed once per (problem, options) and never changed."""
    k = (key, tuple(sorted(kw.items())))
    if k not in _HELPER:
        _HELPER[k] = ref.solve(rig, start, **kw)
    return _HELPER[k]


def _check_parity(ctx, key, rig, start, **kw):
    cams, bR, bt, X, rb, ra, rep = _gpu(ctx, rig, start, **kw)
    Ro, to, bRo, bto, Xo, info = _helper(key, rig, start, **kw)
    R0, t0, bR0, bt0, X0 = start
    K, D, obj, uv, mask, puv, pm = (rig[k] for k in ('K', 'D', 'obj', 'uv', 'mask', 'pt_uv', 'pt_mask'))
    R, t = cams[:, 8:17].reshape(-1, 3, 3), cams[:, 17:20]
    print(rep, info, 'max |dR| %.2e |dt| %.2e |dbR| %.2e |dbt| %.2e |dX| %.2e' % (
        np.abs(R - Ro).max(), np.abs(t - to).max(), np.abs(bR - bRo).max(), np.abs(bt - bto).max(),
        np.abs(X - Xo).max() if len(X) else 0.0))
    assert rep['status_name'] == info['status'] and rep['n_bad_pivots'] == 0
    assert rep['iters'] == info['iters'] and rep['n_accepted'] == info['n_accepted']
    assert abs(rep['lambda_final'] - info['lam']) <= 1e-12 * info['lam']
    assert abs(rep['cost_before'] - info['cost_before']) <= 1e-12 * info['cost_before']
    assert abs(rep['cost_after'] - info['cost_after']) <= 1e-12 * info['cost_after']
    np.testing.assert_allclose(R, Ro, rtol=0, atol=1e-10)
    np.testing.assert_allclose(bR, bRo, rtol=0, atol=1e-10)
    np.testing.assert_allclose(t, to, rtol=0, atol=1e-9)
    np.testing.assert_allclose(bt, bto, rtol=0, atol=1e-9)
    np.testing.assert_allclose(X, Xo, rtol=0, atol=1e-9)
    r0 = ref.residuals(R0, t0, K, D, obj, bR0, bt0, uv, mask, X0, puv, pm)
    assert len(rb) == len(r0) == 2 * (len(obj) * int(mask.sum()) + int(pm.sum())) and len(ra) == len(r0)
    np.testing.assert_allclose(rb, r0, rtol=0, atol=1e-9)
    np.testing.assert_allclose(ra, ref.residuals(Ro, to, K, D, obj, bRo, bto, uv, mask, Xo, puv, pm), rtol=0, atol=1e-8)
    for M in (R, bR):
        np.testing.assert_allclose(M @ np.swapaxes(M, 1, 2), np.broadcast_to(np.eye(3), M.shape), atol=1e-12)
    np.testing.assert_array_equal(cams[:, :8], _cams0(rig, start)[:, :8])  # intrinsics untouched
    return cams, bR, bt, X, rb, ra, rep


@pytest.mark.parametrize('name', list(ref.PROBLEMS))
def test_matches_the_helper_iterate_for_iterate(ctx, name):
    C, B, shape, views, n, pt_vis, seed = ref.PROBLEMS[name]
    plan = sh.plan(n, C)
    print(name, 'points:', plan, 'board chunk', _native.sba_boards_chunk(C))
    if name == 'c16_b40_nc54_n42':
        assert plan == dict(G=16, chunk=41, nchunk=2)
    if name in ('c3_b65_nc4_n65', 'c16_b20_nc4_n42'):
        assert plan['nchunk'] == 2 and B > _native.sba_boards_chunk(C)
    rig, start = ref.problem(name)
    _check_parity(ctx, name, rig, start, max_iters=ref.FIXED_ITERS)


@pytest.mark.parametrize('max_iters', [1, 4, 5, None])
def test_stops_inside_and_at_the_edge_of_a_status_group(ctx, max_iters):
    """max_iters None: the run to convergence, stopped by the ftol that sba_ext_shapes.choose_stop picks
    on the helper's trace (ref.CONVERGED; test_sba_boards_points_cpu.py recomputes it)."""
    rig, start = ref.problem('c3_b5_nc12_n7')
    kw = sh.stop_opts(ref.CONVERGED) if max_iters is None else dict(max_iters=max_iters)
    rep = _check_parity(ctx, 'c3_b5_nc12_n7', rig, start, **kw)[-1]
    if max_iters is None:
        assert rep['status_name'] == 'ftol' and rep['iters'] == ref.CONVERGED.iters


def test_no_points_is_sba_boards_bit_for_bit(ctx):
    rig, start = ref.problem('c3_b5_nc12_n7')
    R0, t0, bR0, bt0, _ = start
    for kw in (dict(max_iters=8), dict(ftol=1e-10)):
        a = ctx.sba_boards(_cams0(rig, start), rig['obj'], rig['uv'], rig['mask'], bR0, bt0, ctx.sba_ext_opts(**kw))
        b = ctx.sba_boards_points(_cams0(rig, start), rig['obj'], rig['uv'], rig['mask'], bR0, bt0, np.zeros((0, 3, 2)),
                                  np.zeros((0, 3), np.uint8), np.zeros((0, 3)), ctx.sba_ext_opts(**kw))
        assert b[3].shape == (0, 3)
        for x, y in zip(a[:5], b[:3] + b[4:6]):
            np.testing.assert_array_equal(x.view(np.uint64), y.view(np.uint64))
        assert a[5] == b[6] and a[5]['iters'] > 0


def test_point_without_an_observation_stays_put(ctx):
    rig, start = ref.problem('c3_b5_nc12_n7')
    base = _gpu(ctx, rig, start, max_iters=8)
    r2 = dict(rig, pt_uv=np.concatenate([rig['pt_uv'], np.zeros((1, 3, 2))]),
              pt_mask=np.concatenate([rig['pt_mask'], np.zeros((1, 3), np.uint8)]))
    lone = np.array([[0.3, -0.7, 1.1]])
    s2 = start[:4] + (np.concatenate([start[4], lone]),)
    cams, bR, bt, X, rb, ra, rep = _gpu(ctx, r2, s2, max_iters=8)
    np.testing.assert_array_equal(X[-1].view(np.uint64), lone[0].view(np.uint64))
    assert rep['iters'] == base[6]['iters'] and rep['n_accepted'] == base[6]['n_accepted'] and len(ra) == len(base[5])
    for a, b in zip((cams, bR, bt, X[:-1], rb, ra), base[:6]):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-9)


def test_two_runs_are_bit_identical_and_orders_do_not_matter(ctx):
    name = 'c16_b40_nc54_n42'
    rig, start = ref.problem(name)
    R0, t0, bR0, bt0, X0 = start
    a = _gpu(ctx, rig, start, max_iters=8)
    b = _gpu(ctx, rig, start, max_iters=8)
    for x, y in zip(a[:6], b[:6]):
        np.testing.assert_array_equal(x.view(np.uint64), y.view(np.uint64))
    assert a[6] == b[6]
    rng = np.random.default_rng(5)
    pb, pp = rng.permutation(40), rng.permutation(42)
    r2 = dict(rig, uv=rig['uv'][pb], mask=rig['mask'][pb])
    c = _gpu(ctx, r2, (R0, t0, bR0[pb], bt0[pb], X0), max_iters=8)
    assert c[6]['iters'] == a[6]['iters'] and c[6]['n_accepted'] == a[6]['n_accepted']
    for x, y in zip(c[:4], (a[0], a[1][pb], a[2][pb], a[3])):
        np.testing.assert_allclose(x, y, rtol=0, atol=1e-9)
    r3 = dict(rig, pt_uv=rig['pt_uv'][pp], pt_mask=rig['pt_mask'][pp])
    d = _gpu(ctx, r3, (R0, t0, bR0, bt0, X0[pp]), max_iters=8)
    assert d[6]['iters'] == a[6]['iters'] and d[6]['n_accepted'] == a[6]['n_accepted']
    for x, y in zip(d[:4], (a[0], a[1], a[2], a[3][pp])):
        np.testing.assert_allclose(x, y, rtol=0, atol=1e-9)


def test_split_rig_is_tied_together_by_the_points(ctx):
    """The case the feature exists for (test_sba_boards_points_cpu.py has the rig and the measured
    figures): parity with the helper over eight iterations, and the CPU test's two assertions on the
    converged solves: the boards-only solve leaves the cross-group centre distances off (measured on
    the helper 3.43e-2 m, asserted above a tenth of it), the mixed solve returns them to the noise level
    (measured 1.50e-2 m, predicted standard deviation 1.2e-2 m; asserted below ten times it)."""
    rig = ref.split_rig()
    start = ref.split_start(rig)
    _check_parity(ctx, 'split', rig, start, max_iters=ref.FIXED_ITERS)
    truth = ref.cross_distances(rig['R'], rig['t'])
    cb = ctx.sba_boards(_cams0(rig, start), rig['obj'], rig['uv'], rig['mask'], start[2], start[3])
    cm = _gpu(ctx, rig, start)
    eb, em = (np.abs(ref.cross_distances(c[0][:, 8:17], c[0][:, 17:20]) - truth).max() for c in (cb, cm))
    print('cross-group centre distances, largest error: boards alone %.3e, with points %.3e m' % (eb, em), cb[5], cm[6])
    assert cm[6]['status_name'] in ('ftol', 'xtol', 'gtol') and cb[5]['status_name'] in ('ftol', 'xtol', 'gtol')
    assert eb >= 3.43e-3
    assert em <= 1.50e-1


def test_bad_inputs_are_refused_before_anything_is_allocated(ctx):
    import ctypes as C_
    rig, start = ref.problem('c3_b5_nc12_n7')
    R0, t0, bR0, bt0, X0 = start
    cams = _cams0(rig, start)
    obj, uv, mask, puv, pm = (rig[k] for k in ('obj', 'uv', 'mask', 'pt_uv', 'pt_mask'))
    _gpu(ctx, rig, start, max_iters=1)
    before = _native.alloc_events()
    std = _native.pack_cameras_standard(rig['K'], np.zeros((3, 5)), R0, t0)
    poses = np.concatenate([bR0.reshape(-1, 9), bt0], 1)
    pts = np.ascontiguousarray(X0)
    p = lambda a: None if a is None else C_.c_void_p(a.ctypes.data)  # noqa: E731

    cams_io, poses_io = cams.copy(), poses.copy()  # in/out arguments of a call that must refuse

    def raw(n_pts, a_uv, a_mask, a_pts):
        rep, o = _native.SbaExtReport(), ctx.sba_ext_opts()
        ctx.check(ctx.lib.acs_sba_boards_points(ctx.h, p(cams_io), 3, p(obj), len(obj), p(uv), p(mask), 5, p(poses_io),
                                                p(a_uv), p(a_mask), n_pts, p(a_pts), C_.byref(o), None, None,
                                                C_.byref(rep), 0), 'acs_sba_boards_points')

    f = ctx.sba_boards_points
    cases = {
        'f_scale': lambda: f(cams, obj, uv, mask, bR0, bt0, puv, pm, X0, ctx.sba_ext_opts(f_scale=0.0)),
        'n_cams': lambda: f(np.tile(cams, (6, 1))[:17], obj, np.tile(uv, (1, 6, 1, 1))[:, :17],
                            np.tile(mask, (1, 6))[:, :17], bR0, bt0, np.tile(puv, (1, 6, 1))[:, :17],
                            np.tile(pm, (1, 6))[:, :17], X0),
        'n_corners low': lambda: f(cams, obj[:2], uv[:, :, :2], mask, bR0, bt0, puv, pm, X0),
        'n_corners high': lambda: f(cams, np.zeros((257, 3)), np.zeros((5, 3, 257, 2)), mask, bR0, bt0, puv, pm, X0),
        'n_boards': lambda: f(cams, obj, uv[:0], mask[:0], bR0[:0], bt0[:0], puv, pm, X0),
        'n_pts negative': lambda: raw(-1, puv, pm, pts),
        'null pt_uv': lambda: raw(7, None, pm, pts),
        'null pt_mask': lambda: raw(7, puv, None, pts),
        'null pts': lambda: raw(7, puv, pm, None),
        'standard': lambda: f(std, obj, uv, mask, bR0, bt0, puv, pm, X0),
    }
    for name, call in cases.items():
        with pytest.raises(RuntimeError) as e:
            call()
        assert 'acs_sba_boards_points' in str(e.value).split('): ', 1)[1] and '(-1)' in str(e.value), (name, str(e.value))
        if name == 'standard':
            assert 'the standard camera model' in str(e.value)
    assert _native.alloc_events() == before


def test_second_call_allocates_nothing_and_device_pointers_match(ctx):
    import torch
    rig, start = ref.problem('c3_b5_nc12_n7')
    R0, t0, bR0, bt0, X0 = start
    host = _gpu(ctx, rig, start, max_iters=8)
    before = _native.alloc_events()
    again = _gpu(ctx, rig, start, max_iters=8)
    assert _native.alloc_events() == before
    for x, y in zip(host[:6], again[:6]):
        np.testing.assert_array_equal(x.view(np.uint64), y.view(np.uint64))
    dev = torch.device('cuda', int(os.environ.get('ACINOSET_DEVICE', 0)))
    poses = np.concatenate([bR0.reshape(-1, 9), bt0], 1)
    n_res = 2 * (len(rig['obj']) * int(rig['mask'].sum()) + int(rig['pt_mask'].sum()))
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in dict(
        cams=_cams0(rig, start), obj=rig['obj'], uv=rig['uv'], mask=rig['mask'], poses=poses, puv=rig['pt_uv'],
        pm=rig['pt_mask'], pts=X0).items()}
    rb = torch.full((n_res,), float('nan'), dtype=torch.float64, device=dev)
    ra = torch.full((n_res,), float('nan'), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    rep = ctx.sba_boards_points_dev(d['cams'].data_ptr(), 3, d['obj'].data_ptr(), len(rig['obj']), d['uv'].data_ptr(),
                                    d['mask'].data_ptr(), 5, d['poses'].data_ptr(), d['puv'].data_ptr(),
                                    d['pm'].data_ptr(), 7, d['pts'].data_ptr(), ctx.sba_ext_opts(max_iters=8),
                                    rb.data_ptr(), ra.data_ptr())
    ctx.sync()
    assert rep == host[6]
    p = d['poses'].cpu().numpy()
    got = (d['cams'].cpu().numpy(), p[:, :9].reshape(-1, 3, 3), p[:, 9:], d['pts'].cpu().numpy(), rb.cpu().numpy(),
           ra.cpu().numpy())
    for x, y in zip(got, host[:6]):
        np.testing.assert_array_equal(np.ascontiguousarray(x).view(np.uint64), y.view(np.uint64))


# ---- the Python layer, on tests/golden/board.npz ---------------------------------------------------
G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'board.npz'))


def test_prepare_manual_points_dense(ctx):
    pt_uv, pt_mask, p3, kept = lsba.prepare_manual_points_dense(G['manual'], G['K'], G['D'], G['R0'], G['t0'])
    pi, ci = np.nonzero(pt_mask)
    np.testing.assert_array_equal(pi, G['manual_point_indices'])
    np.testing.assert_array_equal(ci, G['manual_camera_indices'])
    np.testing.assert_array_equal(pt_uv[pi, ci].astype(np.float32), G['manual_points_2d'])
    np.testing.assert_array_equal(pt_uv[pt_mask == 0], 0.0)
    np.testing.assert_allclose(p3, G['manual_points_3d'], atol=2e-6)
    seen = (~np.isnan(G['manual']).any(2)).sum(1)
    np.testing.assert_array_equal(kept, np.nonzero(seen >= 2)[0])
    assert pt_uv.shape == (len(kept), 3, 2) and pt_mask.dtype == np.uint8 and p3.shape == (len(kept), 3)
    with pytest.raises(ValueError):
        lsba.prepare_manual_points_dense(G['manual'][:, :2], G['K'], G['D'], G['R0'], G['t0'])


def _scene(tmp_path):
    pfs = []
    for c in range(len(G['K'])):
        f = tmp_path / f'points_cam{c}.json'
        f.write_text(str(G[f'points_cam{c}']))
        pfs.append(str(f))
    scene = str(tmp_path / 'scene.json')
    lutils.save_scene(scene, G['K'], G['D'], G['R0'], G['t0'], tuple(int(v) for v in G['res']))
    mf = tmp_path / 'manual_points.json'
    mf.write_text(str(G['manual_points_json']))
    return scene, pfs, str(mf)


def _read(path):
    with open(path, 'rb') as f:
        return f.read()


def test_board_poses_dropin_with_manual_points(ctx, tmp_path):
    from acinoset_amd.lib import app
    scene, pfs, mf = _scene(tmp_path)
    out = str(tmp_path / 'scene_sba.json')
    res = app.sba_board_poses_fisheye(scene, pfs, out, manual_points_fpath=mf)
    K, D, R, t, _ = lutils.load_scene(out, verbose=False)
    with open(str(tmp_path / 'scene_sba_boards.json')) as f:
        boards = json.load(f)
    pt_uv, pt_mask, p3, kept = lsba.prepare_manual_points_dense(G['manual'], G['K'], G['D'], G['R0'], G['t0'])
    mp = boards['manual_points']
    assert [m['index'] for m in mp] == kept.tolist() and [m['n_views'] for m in mp] == pt_mask.sum(1).tolist()
    np.testing.assert_array_equal(np.array([m['xyz'] for m in mp]), res['points_3d'])
    assert boards['report']['iters'] == res['report']['iters'] and len(boards['boards']) == len(res['names'])
    nb = res['n_board_residuals']
    assert nb == 2 * len(res['obj_pts']) * int(res['mask'].sum()) and len(res['after']) == nb + 2 * int(pt_mask.sum())
    # a direct call from the same start gives the same residuals, and the saved cameras are its cameras
    uv, mask, obj, br0, bt0, names = lsba.prepare_calib_boards_for_bundle_adjustment(
        *_board_inputs(pfs), G['K'], G['D'], G['R0'], G['t0'])
    cams0 = _native.pack_cameras(G['K'], G['D'].reshape(-1, 4), G['R0'], G['t0'].reshape(-1, 3))
    d = ctx.sba_boards_points(cams0, obj, uv, mask, br0, bt0, pt_uv, pt_mask, p3)
    np.testing.assert_allclose(res['before'], d[4], rtol=0, atol=1e-9)
    np.testing.assert_allclose(res['after'], d[5], rtol=0, atol=1e-9)
    np.testing.assert_allclose(_native.pack_cameras(K, D.reshape(-1, 4), R, t.reshape(-1, 3)), d[0], rtol=0, atol=1e-9)
    f2 = lambda v: 0.5 * np.log1p(np.asarray(v) ** 2).sum()  # noqa: E731
    assert f2(res['after']) < f2(res['before'])
    assert abs(f2(res['after']) - res['report']['cost_after']) <= 1e-9 * f2(res['after'])


def _board_inputs(pfs):
    img_pts, fnames, shape, square = [], [], None, None
    for p in pfs:
        pts, fn, shape, square, *_ = lutils.load_points(p)
        img_pts.append(pts)
        fnames.append(fn)
    return img_pts, fnames, shape, square


def test_without_the_file_every_output_is_byte_equal(ctx, tmp_path, monkeypatch):
    from acinoset_amd.lib import app

    class _Clock:  # the scene file carries the time it was written at
        @staticmethod
        def now():
            return '2000-01-01 00:00:00'
    monkeypatch.setattr(lutils, 'datetime', _Clock)
    scene, pfs, mf = _scene(tmp_path)
    a, b = str(tmp_path / 'a.json'), str(tmp_path / 'b.json')
    ra = app.sba_board_poses_fisheye(scene, pfs, a)
    rb = app.sba_board_poses_fisheye(scene, pfs, b, manual_points_fpath=None)
    assert _read(a) == _read(b)
    assert _read(str(tmp_path / 'a_boards.json')) == _read(str(tmp_path / 'b_boards.json'))
    assert sorted(ra) == sorted(rb) and 'points_3d' not in ra and 'manual_points' not in json.loads(
        _read(str(tmp_path / 'a_boards.json')))
    np.testing.assert_array_equal(ra['after'], rb['after'])


def test_covariance_with_manual_points_is_refused(ctx, tmp_path):
    from acinoset_amd.lib import app
    scene, pfs, mf = _scene(tmp_path)
    out = tmp_path / 'scene_sba.json'
    with pytest.raises(ValueError):
        app.sba_board_poses_fisheye(scene, pfs, str(out), covariance=True, manual_points_fpath=mf)
    assert not out.exists() and not (tmp_path / 'scene_sba_boards.json').exists()
    assert not (tmp_path / 'scene_sba_cov.json').exists()
    pt_uv, pt_mask, p3, _ = lsba.prepare_manual_points_dense(G['manual'], G['K'], G['D'], G['R0'], G['t0'])
    uv, mask, obj, br0, bt0, _ = lsba.prepare_calib_boards_for_bundle_adjustment(*_board_inputs(pfs), G['K'], G['D'],
                                                                                 G['R0'], G['t0'])
    with pytest.raises(ValueError):
        lsba.bundle_adjust_boards_and_extrinsics(uv, mask, obj, br0, bt0, G['K'], G['D'], G['R0'], G['t0'],
                                                 covariance=True, points_uv=pt_uv, points_mask=pt_mask, points_3d=p3)
