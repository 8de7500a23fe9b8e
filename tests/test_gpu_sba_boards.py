"""GPU: the rigid-board bundle adjustment (acs_sba_boards) against its numpy restatement
(sba_boards_ref.py, the same LM iterate for iterate) at the tolerances test_gpu_sba_ext.py uses against
its oracle: status, iterations and acceptances equal, lambda and both costs 1e-12 relative, rotations
1e-10, translations 1e-9 m, residuals before 1e-9 and after 1e-8 px, R R^T = I to 1e-12."""
import json
import os

import numpy as np
import pytest

import sba_boards_ref as ref
from acinoset_amd import _native
from acinoset_amd.lib import sba as lsba
from acinoset_amd.lib import utils as lutils

pytestmark = pytest.mark.gpu

_RIGS = {}


def _rig(C, B, shape, views, seed=0):
    """A noisy rig (0.5 px) and a perturbed start, built once per shape and never changed."""
    key = (C, B, shape, views, seed)
    if key not in _RIGS:
        rig = ref.make_rig(C, B, shape=shape, seed=seed, views=views, noise=0.5)
        _RIGS[key] = (rig, ref.perturb(rig, seed + 100))
    return _RIGS[key]


def _gpu(ctx, rig, start, **opts):
    R0, t0, bR0, bt0 = start
    cams = _native.pack_cameras(rig['K'], rig['D'], R0, t0)
    return ctx.sba_boards(cams, rig['obj'], rig['uv'], rig['mask'], bR0, bt0, ctx.sba_ext_opts(**opts))


def _check_parity(ctx, rig, start, max_iters):
    """max_iters None: the default 500, a run to convergence. There ftol is 1e-10, not the default
    1e-12: the last steps of a converged run lower the cost by ~1e-12 (4e-14 of it, measured on the
    3-camera rig), which is inside the rounding of the two cost sums, so whether such a step is accepted
    differs between numpy and the kernels by summation order alone (measured: 27 against 26
    iterations, the same 16 acceptances and the same cost to 2e-14). With ftol 1e-10 the run stops on
    a decrease of 1.8e-10, far above that rounding, and every decision before it is clear."""
    kw = dict(ftol=1e-10) if max_iters is None else dict(max_iters=max_iters)
    cams, bR, bt, rb, ra, rep = _gpu(ctx, rig, start, **kw)
    R0, t0, bR0, bt0 = start
    K, D, obj, uv, mask = (rig[k] for k in ('K', 'D', 'obj', 'uv', 'mask'))
    Ro, to, bRo, bto, info = ref.sba_boards(R0, t0, K, D, obj, bR0, bt0, uv, mask, **kw)
    R, t = cams[:, 8:17].reshape(-1, 3, 3), cams[:, 17:20]
    print(rep, info, 'max |dR| %.2e |dt| %.2e |dbR| %.2e |dbt| %.2e' % (
        np.abs(R - Ro).max(), np.abs(t - to).max(), np.abs(bR - bRo).max(), np.abs(bt - bto).max()))
    assert rep['status_name'] == info['status'] and rep['n_bad_pivots'] == 0
    assert rep['iters'] == info['iters'] and rep['n_accepted'] == info['n_accepted']
    assert abs(rep['lambda_final'] - info['lam']) <= 1e-12 * info['lam']
    assert abs(rep['cost_before'] - info['cost_before']) <= 1e-12 * info['cost_before']
    assert abs(rep['cost_after'] - info['cost_after']) <= 1e-12 * info['cost_after']
    np.testing.assert_allclose(R, Ro, rtol=0, atol=1e-10)
    np.testing.assert_allclose(bR, bRo, rtol=0, atol=1e-10)
    np.testing.assert_allclose(t, to, rtol=0, atol=1e-9)
    np.testing.assert_allclose(bt, bto, rtol=0, atol=1e-9)
    np.testing.assert_allclose(rb, ref.residuals(R0, t0, K, D, obj, bR0, bt0, uv, mask), rtol=0, atol=1e-9)
    np.testing.assert_allclose(ra, ref.residuals(Ro, to, K, D, obj, bRo, bto, uv, mask), rtol=0, atol=1e-8)
    for M in (R, bR):
        np.testing.assert_allclose(M @ np.swapaxes(M, 1, 2), np.broadcast_to(np.eye(3), M.shape), atol=1e-12)
    np.testing.assert_array_equal(cams[:, :8], _native.pack_cameras(K, D, R0, t0)[:, :8])  # intrinsics untouched


# (C, B, board shape, views per board): the smallest shapes that reach each path
SHAPES = {
    'c2_b2_nc4': (2, 2, (2, 2), None),
    'c3_b5_nc12': (3, 5, (4, 3), None),
    'c16_b40_nc54': (16, 40, (9, 6), (2, 16)),
    'nc70': (3, 4, (10, 7), (2, 3)),          # more than one corner per lane
    'nc256': (2, 3, (16, 16), None),          # four rounds of the wave
}


@pytest.mark.parametrize('name', list(SHAPES))
def test_matches_the_helper_iterate_for_iterate(ctx, name):
    C, B, shape, views = SHAPES[name]
    rig, start = _rig(C, B, shape, views)
    _check_parity(ctx, rig, start, 8)


@pytest.mark.parametrize('C', [3, 16])
def test_ragged_last_schur_chunk(ctx, C):
    chunk = _native.sba_boards_chunk(C)
    assert chunk == max(1, min(64, 96 * 1024 // (292 * C + 344)))
    rig, start = _rig(C, chunk + 1, (2, 2), (2, C))
    _check_parity(ctx, rig, start, 6)


@pytest.mark.parametrize('max_iters', [1, 4, 5, None])
def test_stops_inside_and_at_the_edge_of_a_status_group(ctx, max_iters):
    rig, start = _rig(3, 5, (4, 3), None)
    _check_parity(ctx, rig, start, max_iters)


def _with_extra_board(rig, start, n_views):
    """The rig and start with one more board (the last): a copy of board 0 seen by the first
    n_views cameras of board 0."""
    R0, t0, bR0, bt0 = start
    r2 = dict(rig)
    m = np.zeros((1, rig['mask'].shape[1]), np.uint8)
    m[0, np.nonzero(rig['mask'][0])[0][:n_views]] = 1
    r2['mask'] = np.concatenate([rig['mask'], m])
    r2['uv'] = np.concatenate([rig['uv'], rig['uv'][:1] * m[0][None, :, None, None]])
    return r2, (R0, t0, np.concatenate([bR0, bR0[:1]]), np.concatenate([bt0, bt0[:1]]))


def test_board_without_a_view_stays_put(ctx):
    rig, start = _rig(3, 5, (4, 3), None)
    base = _gpu(ctx, rig, start, max_iters=20)
    r2, s2 = _with_extra_board(rig, start, 0)
    cams, bR, bt, rb, ra, rep = _gpu(ctx, r2, s2, max_iters=20)
    np.testing.assert_array_equal(bR[-1].view(np.uint64), s2[2][-1].view(np.uint64))
    np.testing.assert_array_equal(bt[-1].view(np.uint64), s2[3][-1].view(np.uint64))
    assert rep['iters'] == base[5]['iters'] and len(ra) == len(base[4])
    for a, b in zip((cams, bR[:-1], bt[:-1], ra), (base[0], base[1], base[2], base[4])):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-9)


def _in_camera0_frame(cams, bR, bt):
    """Every camera and board pose relative to camera 0: the same poses with the free rigid gauge
    taken out. Returns (R_c R_0^T, t_c - R_c R_0^T t_0, R_0 R_b, R_0 t_b + t_0)."""
    R, t = cams[:, 8:17].reshape(-1, 3, 3), cams[:, 17:20]
    Rr = R @ R[0].T
    return Rr, t - Rr @ t[0], R[0] @ bR, bt @ R[0].T + t[0]


def test_board_with_one_view_leaves_the_rest_alone(ctx):
    """A board one camera sees determines its own pose and adds no constraint on the rest: the cameras
    and the other boards of the converged solve equal those of the solve without it to 1e-9, compared
    relative to camera 0. Compared raw they differ by a rigid motion of the whole scene (measured:
    3.3e-4 on the camera records): the gauge is free, the damping of every block decides how far an
    iteration drifts along it, and the extra board's block takes part in that."""
    rig, start = _rig(3, 5, (4, 3), None)
    base = _gpu(ctx, rig, start)
    r2, s2 = _with_extra_board(rig, start, 1)
    cams, bR, bt, rb, ra, rep = _gpu(ctx, r2, s2)
    a, b = _in_camera0_frame(cams, bR[:-1], bt[:-1]), _in_camera0_frame(base[0], base[1], base[2])
    print('one view: raw max |d cams| %.2e; relative to camera 0 max |d| %.2e' % (
        np.abs(cams - base[0]).max(), max(np.abs(x - y).max() for x, y in zip(a, b))), rep, base[5])
    assert rep['status_name'] in ('ftol', 'xtol', 'gtol') and base[5]['status_name'] in ('ftol', 'xtol', 'gtol')
    for x, y in zip(a, b):
        np.testing.assert_allclose(x, y, rtol=0, atol=1e-9)


def test_two_runs_are_bit_identical_and_orders_do_not_matter(ctx):
    rig, start = _rig(16, 40, (9, 6), (2, 16))
    R0, t0, bR0, bt0 = start
    a = _gpu(ctx, rig, start, max_iters=8)
    b = _gpu(ctx, rig, start, max_iters=8)
    for x, y in zip(a[:5], b[:5]):
        np.testing.assert_array_equal(x.view(np.uint64), y.view(np.uint64))
    assert a[5] == b[5]
    rng = np.random.default_rng(5)
    pb, pc = rng.permutation(40), rng.permutation(16)
    r2 = dict(rig, uv=rig['uv'][pb], mask=rig['mask'][pb])
    c = _gpu(ctx, r2, (R0, t0, bR0[pb], bt0[pb]), max_iters=8)
    assert c[5]['iters'] == a[5]['iters']
    np.testing.assert_allclose(c[0], a[0], rtol=0, atol=1e-9)
    np.testing.assert_allclose(c[1], a[1][pb], rtol=0, atol=1e-9)
    np.testing.assert_allclose(c[2], a[2][pb], rtol=0, atol=1e-9)
    r3 = dict(rig, uv=rig['uv'][:, pc], mask=rig['mask'][:, pc], K=rig['K'][pc], D=rig['D'][pc])
    d = _gpu(ctx, r3, (R0[pc], t0[pc], bR0, bt0), max_iters=8)
    assert d[5]['iters'] == a[5]['iters']
    np.testing.assert_allclose(d[0], a[0][pc], rtol=0, atol=1e-9)
    np.testing.assert_allclose(d[1], a[1], rtol=0, atol=1e-9)
    np.testing.assert_allclose(d[2], a[2], rtol=0, atol=1e-9)


def test_scale_is_recovered_where_free_corners_keep_the_error(ctx):
    """What the feature is for. Noiseless data, every camera and board translation of the start
    multiplied by 1.05: the rigid boards return every camera baseline (1e-6 relative); the free
    corners of the same data, started at the same scaled scene, keep the 5 % error."""
    rig = ref.make_rig(3, 5, seed=0)
    R, t, K, D, obj, bR, bt = (rig[k] for k in ('R', 't', 'K', 'D', 'obj', 'bR', 'bt'))
    truth = ref.centre_distances(R, t)
    br, btn, r_arr, t_arr, res = lsba.bundle_adjust_boards_and_extrinsics(rig['uv'], rig['mask'], obj, bR, 1.05 * bt, K, D,
                                                                          R, 1.05 * t)
    err = np.abs(ref.centre_distances(r_arr, t_arr) / truth - 1).max()
    print('rigid boards: max relative baseline error %.3e' % err, res['report'])
    assert err <= 1e-6
    assert r_arr.shape == (3, 3, 3) and t_arr.shape == (3, 3, 1) and br.shape == (5, 3, 3) and btn.shape == (5, 3)
    p2, X, pi, ci = ref.free_corners(rig, bR, bt)
    _, r_f, t_f, _ = lsba.bundle_adjust_points_and_extrinsics(p2, 1.05 * X, pi, ci, K, D, R, 1.05 * t)
    kept = np.abs(ref.centre_distances(r_f, t_f) / (1.05 * truth) - 1).max()
    print('free corners: baselines stay within %.3e of the scaled start' % kept)
    assert kept <= 1e-3


def test_bad_inputs_are_refused_before_anything_is_allocated(ctx):
    rig, start = _rig(3, 5, (4, 3), None)
    R0, t0, bR0, bt0 = start
    cams = _native.pack_cameras(rig['K'], rig['D'], R0, t0)
    obj, uv, mask = rig['obj'], rig['uv'], rig['mask']
    _gpu(ctx, rig, start, max_iters=1)
    before = _native.alloc_events()
    std = _native.pack_cameras_standard(rig['K'], np.zeros((3, 5)), R0, t0)
    cases = {
        'f_scale': lambda: ctx.sba_boards(cams, obj, uv, mask, bR0, bt0, ctx.sba_ext_opts(f_scale=0.0)),
        'n_cams': lambda: ctx.sba_boards(np.tile(cams, (6, 1))[:17], obj, np.tile(uv, (1, 6, 1, 1))[:, :17],
                                         np.tile(mask, (1, 6))[:, :17], bR0, bt0),
        'n_corners low': lambda: ctx.sba_boards(cams, obj[:2], uv[:, :, :2], mask, bR0, bt0),
        'n_corners high': lambda: ctx.sba_boards(cams, np.zeros((257, 3)), np.zeros((5, 3, 257, 2)), mask, bR0, bt0),
        'n_boards': lambda: ctx.sba_boards(cams, obj, uv[:0], mask[:0], bR0[:0], bt0[:0]),
        'standard': lambda: ctx.sba_boards(std, obj, uv, mask, bR0, bt0),
    }
    for name, call in cases.items():
        with pytest.raises(RuntimeError) as e:
            call()
        assert 'acs_sba_boards' in str(e.value).split('): ', 1)[1] and '(-1)' in str(e.value), (name, str(e.value))
        if name == 'standard':
            assert 'the standard camera model' in str(e.value)
    assert _native.alloc_events() == before


def test_second_call_allocates_nothing_and_device_pointers_match(ctx):
    import torch
    rig, start = _rig(3, 5, (4, 3), None)
    R0, t0, bR0, bt0 = start
    host = _gpu(ctx, rig, start, max_iters=8)
    before = _native.alloc_events()
    again = _gpu(ctx, rig, start, max_iters=8)
    assert _native.alloc_events() == before
    np.testing.assert_array_equal(host[0].view(np.uint64), again[0].view(np.uint64))
    dev = torch.device('cuda', int(os.environ.get('ACINOSET_DEVICE', 0)))
    poses = np.concatenate([bR0.reshape(-1, 9), bt0], 1)
    n_res = 2 * len(rig['obj']) * int(rig['mask'].sum())
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in dict(
        cams=_native.pack_cameras(rig['K'], rig['D'], R0, t0), obj=rig['obj'], uv=rig['uv'], mask=rig['mask'],
        poses=poses).items()}
    rb = torch.full((n_res,), float('nan'), dtype=torch.float64, device=dev)
    ra = torch.full((n_res,), float('nan'), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    rep = ctx.sba_boards_dev(d['cams'].data_ptr(), 3, d['obj'].data_ptr(), len(rig['obj']), d['uv'].data_ptr(),
                             d['mask'].data_ptr(), 5, d['poses'].data_ptr(), ctx.sba_ext_opts(max_iters=8),
                             rb.data_ptr(), ra.data_ptr())
    ctx.sync()
    assert rep == host[5]
    p = d['poses'].cpu().numpy()
    for x, y in zip((d['cams'].cpu().numpy(), p[:, :9].reshape(-1, 3, 3), p[:, 9:], rb.cpu().numpy(), ra.cpu().numpy()),
                    host[:5]):
        np.testing.assert_array_equal(np.ascontiguousarray(x).view(np.uint64), y.view(np.uint64))


def test_board_poses_dropin(ctx, tmp_path):
    from acinoset_amd.lib import app
    G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'board.npz'))
    C = len(G['K'])
    pfs, names = [], []
    for c in range(C):
        f = tmp_path / f'points_cam{c}.json'
        f.write_text(str(G[f'points_cam{c}']))
        pfs.append(str(f))
        names.append(set(json.loads(str(G[f'points_cam{c}']))['points']))
    scene = str(tmp_path / 'scene.json')
    lutils.save_scene(scene, G['K'], G['D'], G['R0'], G['t0'], tuple(int(v) for v in G['res']))
    out = str(tmp_path / 'scene_sba.json')
    res = app.sba_board_poses_fisheye(scene, pfs, out)
    K, D, R, t, _ = lutils.load_scene(out, verbose=False)
    with open(str(tmp_path / 'scene_sba_boards.json')) as f:
        boards = json.load(f)
    shared = sorted(n for n in set.union(*names) if sum(n in s for s in names) >= 2)
    assert [b['name'] for b in boards['boards']] == shared and len(shared) > 0
    assert [b['n_views'] for b in boards['boards']] == [sum(n in s for s in names) for n in shared]
    assert boards['board_square_len'] == float(G['square']) and boards['report']['iters'] == res['report']['iters']
    # the saved cameras reproduce the returned residuals on the posed corners
    bR = np.array([b['r'] for b in boards['boards']])
    bt = np.array([b['t'] for b in boards['boards']])
    p2, X, pi, ci = ref.free_corners(dict(obj=res['obj_pts'], mask=res['mask'], uv=res['uv']), bR, bt)
    r = ctx.sba_residuals(_native.pack_cameras(K, D.reshape(-1, 4), R, t.reshape(-1, 3)), p2, pi, ci, X)
    np.testing.assert_allclose(np.ravel(r), res['after'], rtol=0, atol=1e-9)
    f2 = lambda v: 0.5 * np.log1p(np.asarray(v) ** 2).sum()  # noqa: E731
    assert f2(res['after']) < f2(res['before'])
    assert abs(f2(res['after']) - res['report']['cost_after']) <= 1e-9 * f2(res['after'])
