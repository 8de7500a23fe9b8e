"""GPU: camera and board pose covariances of the rigid-board SBA (acs_sba_boards_covariance) against
the numpy restatement tests/sba_boards_cov_ref.py, evaluated at the GPU solver's own solution
(ctx.sba_boards, 8 iterations, 0.5 px noise, the `_rig` / `perturb` recipe of test_gpu_sba_boards.py,
the solver's default f_scale = 1).

Shapes (SHAPES of the solver's test): C2 / B2 / 2 x 2 (one tile, 12 rows), C3 / B5 / 4 x 3 (18 rows
cross the tile edge), C16 / B40 / 9 x 6 with 2..16 views (96 rows, several Schur chunks), nc = 70 and
nc = 256 (more than one round of the wave), and B = acs_sba_boards_chunk(C) + 1 for C = 3 and 16 (a
ragged last chunk).

Measure and bound (those of test_gpu_sba_ext_cov.py). cov_cams against the helper's R in the measure
max |S - R| / sqrt(diag R (x) diag R) over the entries whose variances are non-zero, bounded by
beta = C_BOUND cond2(Ah) 2.2e-16, C_BOUND = 10; Ah = S + mu Q Q^T scaled to unit diagonal is the
matrix both sides invert. A board's record cov_b = sigma^2 V^-1 + V^-1 W^T cov_cc W V^-1 entry by entry:
    |cov_b - R_b|_jk <= C_BOUND 2.2e-16 (cond2(Ah) u_j u_k + cond2(Vh_b) d_j d_k),
u = |V^-1| |W_b^T| s, s = sqrt(diag R), d = sqrt(diag R_b), Vh_b the unit-diagonal V_b. The measured
maxima of error / bound are printed and recorded in DESIGN §3.

The camera matrix is written as the mean of each entry and its transpose. Mirroring one triangle of
the refined inverse (unsymmetric by ~cond eps) put board_rot_sd_max of c3_b5_nc12 anchored at camera 2
1.43e-9 from the helper, against the 1e-9 asserted for sigma_hat and the four sd maxima.
"""
import json
import os

import numpy as np
import pytest

import sba_boards_cov_ref as cref
import sba_boards_ref as bref
import test_gpu_sba_boards as solver_test
from acinoset_amd import _native
from acinoset_amd.lib import sba as lsba, utils as lutils

pytestmark = pytest.mark.gpu

EPS = 2.2e-16
C_BOUND = 10.0
NAME = 'acs_sba_boards_covariance'
_cache = {}


def _shape(name):
    if name.startswith('ragged'):
        C = int(name[6:])
        return C, _native.sba_boards_chunk(C) + 1, (2, 2), (2, C)
    return solver_test.SHAPES[name]


def _problem(ctx, name):
    """The rig solved once on the GPU: dict with cams (solution records), R, t, bR, bt and the rig's data."""
    if name not in _cache:
        rig, start = solver_test._rig(*_shape(name))
        R0, t0, bR0, bt0 = start
        cams0 = _native.pack_cameras(rig['K'], rig['D'], R0, t0)
        cams, bR, bt, _, _, rep = ctx.sba_boards(cams0, rig['obj'], rig['uv'], rig['mask'], bR0, bt0,
                                                 ctx.sba_ext_opts(max_iters=8), residuals=False)
        _cache[name] = dict(cams=cams, R=cams[:, 8:17].reshape(-1, 3, 3).copy(), t=cams[:, 17:20].copy(), bR=bR, bt=bt,
                            K=rig['K'], D=rig['D'], obj=rig['obj'], uv=rig['uv'], mask=rig['mask'], ref={})
    return _cache[name]


def _ref(p, gauge='anchor', anchor=0, sigma_px=1.0, f_scale=1.0):
    key = (gauge, anchor, sigma_px, f_scale)
    if key not in p['ref']:
        p['ref'][key] = cref.covariance(p['R'], p['t'], p['K'], p['D'], p['obj'], p['bR'], p['bt'], p['uv'], p['mask'],
                                        f_scale, sigma_px, gauge, anchor)
    return p['ref'][key]


def _gpu(ctx, p, gauge='anchor', anchor=0, sigma_px=1.0, f_scale=1.0):
    return ctx.sba_boards_covariance(p['cams'], p['obj'], p['uv'], p['mask'], p['bR'], p['bt'], f_scale=f_scale,
                                     sigma_px=sigma_px, gauge=gauge, anchor=anchor)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _weight_rounding(p, f_scale=1.0):
    """gamma: the relative change of a Triggs weight under one unit in the last place of its pixel
    coordinate, the largest over the seen residuals: max |d wh / d r| ulp(|uv|) / wh. The residual
    r = project - uv carries the rounding of the projection, about an ulp of the coordinate whichever
    side computes it, and wh depends on r: at f_scale = 1 and r ~ 0.5 px, |d ln wh / d r| ~ 3 per px.
    With |delta wh| <= gamma wh for every residual, -gamma V <= delta V <= gamma V, so to first order
    |delta (V^-1)_jk| <= gamma d_j d_k. Computed from the helper's residuals alone."""
    r = bref.residuals(p['R'], p['t'], p['K'], p['D'], p['obj'], p['bR'], p['bt'], p['uv'], p['mask'] != 0)
    z = r * r / (f_scale * f_scale)
    w = 1.0 / (1.0 + z)
    triggs = (1.0 - z) * w * w
    wh = np.maximum(triggs, 0.1 * w)
    dz = np.where(triggs >= 0.1 * w, -w * w - 2.0 * (1.0 - z) * w ** 3, -0.1 * w * w)
    dr = np.abs(dz * 2.0 * r / (f_scale * f_scale))
    return float((dr / wh).max() * np.spacing(np.abs(p['uv'][p['mask'] != 0]).max()))


def _boards_worst(cb, ref, cond, other=None, gamma=0.0):
    """max over the OK boards and entries of |cb - R_b| / (2.2e-16 (cond2(Ah) u_j u_k + cond2(Vh_b) d_j d_k))
    (the module docstring's bound with C_BOUND = 1); R_b = `other` or the helper's records. gamma
    (_weight_rounding) adds gamma d_j d_k to that unit."""
    s = np.sqrt(ref['cov_cams'].diagonal())
    worst = 0.0
    for b in np.flatnonzero(ref['status'] == cref.OK):
        Vi = np.linalg.inv(ref['V'][b])
        u = np.abs(Vi) @ np.abs(ref['W'][b].T) @ s
        d = np.sqrt(ref['cov_boards'][b].diagonal())
        unit = EPS * (cond * np.outer(u, u) + np.linalg.cond(cref.unit_diagonal(ref['V'][b])[0]) * np.outer(d, d))
        unit = unit + gamma * np.outer(d, d)
        tgt = ref['cov_boards'][b] if other is None else other[b]
        worst = max(worst, float((np.abs(cb[b] - tgt) / unit).max()))
    return worst


def _check(got, ref, gauge, anchor, label, gamma=0.0):
    cc, cb, st, rep = got
    r = ref['report']
    assert rep['status'] == r['status'] == 0 and rep['status_name'] == 'ok'
    np.testing.assert_array_equal(st, ref['status'])
    for k in ('n_boards', 'n_ok', 'n_noobs', 'n_degenerate', 'dof'):
        assert rep[k] == r[k], k
    # exactly symmetric, the anchor camera exactly zero
    np.testing.assert_array_equal(_bits(cc), _bits(cc.T))
    np.testing.assert_array_equal(_bits(cb), _bits(np.swapaxes(cb, 1, 2)))
    if gauge == 'anchor':
        assert not cc[6 * anchor:6 * anchor + 6].any() and not cc[:, 6 * anchor:6 * anchor + 6].any()
        assert not ref['cov_cams'][6 * anchor:6 * anchor + 6].any()
    ok = st == cref.OK
    assert np.isnan(cb[~ok]).all() and np.isfinite(cb[ok]).all() and np.isfinite(cc).all()
    cond = np.linalg.cond(ref['Ah']) if ref['Ah'] is not None else 0.0
    err = cref.rel_error(cc, ref['cov_cams'])
    worst_b = _boards_worst(cb, ref, cond, gamma=gamma)
    print('%s %s %s: cond(Ah) %.4g, cameras error %.3g = %.3f cond eps; boards worst %.3f of the unit bound; '
          'min pivot %.4g' % (label, gauge, anchor, cond, err, err / (cond * EPS) if cond else 0.0, worst_b,
                              rep['min_pivot']))
    assert err <= C_BOUND * cond * EPS
    assert worst_b <= C_BOUND
    sd = np.sqrt(cc.diagonal()).reshape(-1, 6)
    assert rep['rot_sd_max'] == sd[:, :3].max() and rep['trans_sd_max'] == sd[:, 3:].max()
    bsd = np.sqrt(np.diagonal(cb[ok], axis1=1, axis2=2))
    assert rep['board_rot_sd_max'] == bsd[:, :3].max() and rep['board_trans_sd_max'] == bsd[:, 3:].max()
    if ref['Ah'] is not None:
        np.testing.assert_allclose(rep['min_pivot'], r['min_pivot'], rtol=1e-6)
    else:
        assert np.isnan(rep['min_pivot']) and np.isnan(r['min_pivot'])
    keys = ('sigma_hat_px', 'rot_sd_max', 'trans_sd_max', 'board_rot_sd_max', 'board_trans_sd_max')
    print('   relative to the helper: ' + ', '.join('%s %.2e' % (k, abs(rep[k] - r[k]) / r[k] if r[k] else abs(rep[k]))
                                                    for k in keys))
    for k in keys:
        np.testing.assert_allclose(rep[k], r[k], rtol=1e-9, err_msg=k)


CASES = [(n, g, a) for n, a in (('c2_b2_nc4', 1), ('c3_b5_nc12', 2), ('c16_b40_nc54', 11), ('nc70', 1), ('nc256', 1),
                                ('ragged3', 2), ('ragged16', 7))
         for g, a in (('free', 0), ('anchor', 0), ('anchor', a))]


@pytest.mark.parametrize('name,gauge,anchor', CASES)
def test_matches_helper(ctx, name, gauge, anchor):
    p = _problem(ctx, name)
    _check(_gpu(ctx, p, gauge, anchor), _ref(p, gauge, anchor), gauge, anchor, name)


def test_sigma_px_scales_by_its_square(ctx):
    p = _problem(ctx, 'c3_b5_nc12')
    one = _gpu(ctx, p)
    got = _gpu(ctx, p, sigma_px=0.7)
    _check(got, _ref(p, sigma_px=0.7), 'anchor', 0, 'c3 sigma 0.7')
    np.testing.assert_allclose(got[0], 0.7 * 0.7 * one[0], rtol=1e-14, atol=0)
    ref = _ref(p)
    assert _boards_worst(got[1] / (0.7 * 0.7), ref, np.linalg.cond(ref['Ah']), other=one[1]) <= C_BOUND
    assert got[3]['sigma_hat_px'] == one[3]['sigma_hat_px'] and got[3]['min_pivot'] == one[3]['min_pivot']


def test_f_scale_changes_the_result_as_the_helper_says(ctx):
    p = _problem(ctx, 'c3_b5_nc12')
    one = _gpu(ctx, p)
    got = _gpu(ctx, p, f_scale=50.0)
    _check(got, _ref(p, f_scale=50.0), 'anchor', 0, 'c3 f 50')
    assert cref.rel_error(got[0], one[0]) > 1e-3   # the Triggs weights at f = 1 differ visibly at 0.5 px


def _with_extra_boards(p):
    """Boards appended for the covariance call only: 5 without a view, 6 a copy of board 0 seen by
    camera 1 alone, 7 a copy of board 1 whose one view holds a NaN corner."""
    C = p['mask'].shape[1]
    m = np.zeros((3, C), np.uint8)
    m[1, 1] = 1
    m[2, 0] = 1
    uv = np.concatenate([p['uv'], np.zeros_like(p['uv'][:1]), p['uv'][:2]])
    uv[7, 0, 0, 0] = np.nan
    return dict(p, mask=np.concatenate([p['mask'], m]), uv=uv, bR=np.concatenate([p['bR'], p['bR'][:1], p['bR'][:2]]),
                bt=np.concatenate([p['bt'], p['bt'][:1], p['bt'][:2]]), ref={})


def test_mixed_statuses_and_s_unchanged_by_boards_left_out(ctx):
    p = _problem(ctx, 'c3_b5_nc12')
    base = _gpu(ctx, p, 'anchor', 2)
    q = _with_extra_boards(p)
    got = _gpu(ctx, q, 'anchor', 2)
    cc, cb, st, rep = got
    np.testing.assert_array_equal(st, [0, 0, 0, 0, 0, cref.NOOBS, cref.OK, cref.DEGENERATE])
    assert (rep['n_boards'], rep['n_ok'], rep['n_noobs'], rep['n_degenerate']) == (8, 6, 1, 1)
    assert np.isnan(cb[[5, 7]]).all() and np.isfinite(cb[:5]).all() and np.isfinite(cb[6]).all()
    # without the single-view board (which is OK and takes part) the boards left out change no bit
    keep = [0, 1, 2, 3, 4, 5, 7]
    q2 = dict(q, mask=q['mask'][keep], uv=q['uv'][keep], bR=q['bR'][keep], bt=q['bt'][keep], ref={})
    cc2, cb2, st2, rep2 = _gpu(ctx, q2, 'anchor', 2)
    np.testing.assert_array_equal(st2, [0, 0, 0, 0, 0, cref.NOOBS, cref.DEGENERATE])
    np.testing.assert_array_equal(_bits(cc2), _bits(base[0]))
    np.testing.assert_array_equal(_bits(cb2[:5]), _bits(base[1]))
    assert np.isnan(cb2[5:]).all()
    assert rep2['sigma_hat_px'] == base[3]['sigma_hat_px'] and rep2['min_pivot'] == base[3]['min_pivot']
    assert rep2['dof'] == base[3]['dof']
    # ... and the whole record, the single-view board's included, against the helper
    _check(got, _ref(q, 'anchor', 2), 'anchor', 2, 'c3 + noobs + single view + degenerate')


def test_degenerate_problem_is_not_an_error(ctx):
    p = _problem(ctx, 'c3_b5_nc12')
    mask = p['mask'].copy()
    mask[:, 2] = 0   # camera 2 is seen by no board
    q = dict(p, mask=mask, ref={})
    cc, cb, st, rep = _gpu(ctx, q)
    ref = _ref(q)
    print('min pivot %.3g (helper %.3g)' % (rep['min_pivot'], ref['report']['min_pivot']))
    np.testing.assert_array_equal(st, ref['status'])
    assert (st == cref.OK).all()
    assert rep['status'] == ref['report']['status'] == 1 and rep['status_name'] == 'degenerate'
    assert not rep['min_pivot'] > 1e-9
    assert np.isnan(cc).all() and np.isnan(cb).all()
    for k in ('rot_sd_max', 'trans_sd_max', 'board_rot_sd_max', 'board_trans_sd_max'):
        assert np.isnan(rep[k]), k
    assert rep['dof'] == ref['report']['dof']
    np.testing.assert_allclose(rep['sigma_hat_px'], ref['report']['sigma_hat_px'], rtol=1e-9)


@pytest.mark.parametrize('gauge', ['free', 'anchor'])
def test_one_camera(ctx, gauge):
    p = _problem(ctx, 'c3_b5_nc12')
    q = dict(p, cams=p['cams'][:1], R=p['R'][:1], t=p['t'][:1], K=p['K'][:1], D=p['D'][:1],
             uv=np.ascontiguousarray(p['uv'][:, :1]), mask=np.ascontiguousarray(p['mask'][:, :1]), ref={})
    got = _gpu(ctx, q, gauge, 0, sigma_px=0.5)
    cc, cb, st, rep = got
    assert cc.shape == (6, 6) and not cc.any() and rep['status'] == 0
    assert rep['rot_sd_max'] == 0.0 and rep['trans_sd_max'] == 0.0
    # With cov_cc = 0 the entrywise bound is 10 cond2(Vh_b) 2.2e-16 d_j d_k alone, and the helper does not
    # meet that against itself: one ulp of the pixel coordinates moves its own records by 44 cond2(Vh_b)
    # 2.2e-16 at f_scale = 1 (0.5 at f_scale = 50), through the weights. The bound's unit therefore
    # carries the weights' term here (_weight_rounding); the kernels measured 35.4 cond2(Vh_b) 2.2e-16.
    gamma = _weight_rounding(q)
    ref = _ref(q, gauge, 0, sigma_px=0.5)
    print('gamma %.3g = %.0f eps; plain measure %.1f cond eps' % (gamma, gamma / EPS, _boards_worst(cb, ref, 0.0)))
    _check(got, ref, gauge, 0, 'one camera', gamma=gamma)


def test_validation_errors_stage_nothing(ctx, monkeypatch):
    p = _problem(ctx, 'c3_b5_nc12')
    _gpu(ctx, p)
    std = np.zeros((3, _native.ACS_CAM_STRIDE_STD))
    big = np.tile(p['cams'][:1], (17, 1))
    cases = {
        'f_scale 0': dict(f_scale=0.0), 'f_scale < 0': dict(f_scale=-1.0), 'sigma_px 0': dict(sigma_px=0.0),
        'anchor 3': dict(anchor=3), 'anchor -1': dict(anchor=-1), 'standard': dict(cams=std),
        '17 cameras': dict(cams=big, mask=np.ones((5, 17), np.uint8), uv=np.zeros((5, 17, 12, 2))),
        '2 corners': dict(obj=p['obj'][:2], uv=np.ascontiguousarray(p['uv'][:, :, :2])),
        '257 corners': dict(obj=np.zeros((257, 3)), uv=np.zeros((5, 3, 257, 2))),
        'no board': dict(mask=p['mask'][:0], uv=p['uv'][:0], bR=p['bR'][:0], bt=p['bt'][:0]),
        'gauge 7': dict(gauge='bogus'),
    }
    monkeypatch.setitem(_native.GAUGES, 'bogus', 7)
    before = _native.alloc_events()
    for name, kw in cases.items():
        a = dict(cams=p['cams'], obj=p['obj'], uv=p['uv'], mask=p['mask'], bR=p['bR'], bt=p['bt'], f_scale=1.0,
                 sigma_px=1.0, gauge='anchor', anchor=0)
        a.update(kw)
        with pytest.raises(RuntimeError) as e:
            ctx.sba_boards_covariance(a['cams'], a['obj'], a['uv'], a['mask'], a['bR'], a['bt'], f_scale=a['f_scale'],
                                      sigma_px=a['sigma_px'], gauge=a['gauge'], anchor=a['anchor'])
        assert NAME in str(e.value).split('): ', 1)[1] and '(-1)' in str(e.value), (name, str(e.value))
    assert _native.alloc_events() == before
    monkeypatch.delitem(_native.GAUGES, 'bogus')
    with pytest.raises(ValueError):
        _gpu(ctx, p, 'fixed')
    # an anchor out of range is no error in the free gauge
    assert _gpu(ctx, p, 'free', 9)[3]['status'] == 0


def test_second_call_allocates_nothing_and_device_pointers_match(ctx):
    import torch
    p = _problem(ctx, 'c16_b40_nc54')
    first = _gpu(ctx, p, 'anchor', 11)
    before = _native.alloc_events()
    again = _gpu(ctx, p, 'anchor', 11)
    assert _native.alloc_events() == before
    for a, b in zip(first[:3], again[:3]):
        np.testing.assert_array_equal(_bits(a) if a.dtype == np.float64 else a, _bits(b) if b.dtype == np.float64 else b)
    assert json.dumps(first[3], sort_keys=True) == json.dumps(again[3], sort_keys=True)
    dev = torch.device('cuda', int(os.environ.get('ACINOSET_DEVICE', 0)))
    B, C = p['mask'].shape
    poses = np.concatenate([p['bR'].reshape(-1, 9), p['bt']], 1)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in dict(
        cams=p['cams'], obj=p['obj'], uv=p['uv'], mask=p['mask'], poses=poses).items()}
    cc = torch.full((6 * C, 6 * C), float('nan'), dtype=torch.float64, device=dev)
    cb = torch.full((B, 6, 6), float('nan'), dtype=torch.float64, device=dev)
    st = torch.full((B,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    rep = ctx.sba_boards_covariance_dev(d['cams'].data_ptr(), C, d['obj'].data_ptr(), len(p['obj']), d['uv'].data_ptr(),
                                        d['mask'].data_ptr(), B, d['poses'].data_ptr(), cc.data_ptr(), cb.data_ptr(),
                                        st.data_ptr(), gauge='anchor', anchor=11)
    assert json.dumps(rep, sort_keys=True) == json.dumps(first[3], sort_keys=True)
    np.testing.assert_array_equal(_bits(cc.cpu().numpy()), _bits(first[0]))
    np.testing.assert_array_equal(_bits(cb.cpu().numpy()), _bits(first[1]))
    np.testing.assert_array_equal(st.cpu().numpy(), first[2])
    # the optional outputs left out: the same cameras and report
    cc2 = torch.full((6 * C, 6 * C), float('nan'), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    rep2 = ctx.sba_boards_covariance_dev(d['cams'].data_ptr(), C, d['obj'].data_ptr(), len(p['obj']),
                                         d['uv'].data_ptr(), d['mask'].data_ptr(), B, d['poses'].data_ptr(),
                                         cc2.data_ptr(), gauge='anchor', anchor=11)
    assert json.dumps(rep2, sort_keys=True) == json.dumps(first[3], sort_keys=True)
    np.testing.assert_array_equal(_bits(cc2.cpu().numpy()), _bits(first[0]))


@pytest.mark.parametrize('name,anchor', [('c3_b5_nc12', 0), ('c16_b40_nc54', 11)])
def test_board_order_invariance(ctx, name, anchor):
    """A permutation of the boards permutes cov_boards and changes only the summation order of S: the
    cameras stay within the helper comparison's bound, a board's record within its own."""
    p = _problem(ctx, name)
    base = _gpu(ctx, p, 'anchor', anchor)
    perm = np.random.default_rng(1).permutation(len(p['bR']))
    q = dict(p, mask=p['mask'][perm], uv=p['uv'][perm], bR=p['bR'][perm], bt=p['bt'][perm])
    got = _gpu(ctx, q, 'anchor', anchor)
    ref = _ref(p, 'anchor', anchor)
    cond = np.linalg.cond(ref['Ah'])
    ec = cref.rel_error(got[0], base[0])
    back = np.empty_like(got[1])
    back[perm] = got[1]
    worst = _boards_worst(back, ref, cond, other=base[1])
    print('%s: cameras %.3g (%.3f cond eps), boards %.3f of the unit bound' % (name, ec, ec / (cond * EPS), worst))
    np.testing.assert_array_equal(got[2], base[2][perm])
    assert ec <= C_BOUND * cond * EPS and worst <= C_BOUND
    assert got[3]['dof'] == base[3]['dof'] and got[3]['n_ok'] == base[3]['n_ok']


def _lib_args(p_rig, start):
    R0, t0, bR0, bt0 = start
    return (p_rig['uv'], p_rig['mask'], p_rig['obj'], bR0, bt0, p_rig['K'], p_rig['D'], R0, t0)


def test_lib_default_is_byte_equal_and_covariance_adds_keys(ctx):
    rig, start = solver_test._rig(*solver_test.SHAPES['c3_b5_nc12'])
    args = _lib_args(rig, start)
    plain = lsba.bundle_adjust_boards_and_extrinsics(*args, max_iters=8)
    off = lsba.bundle_adjust_boards_and_extrinsics(*args, max_iters=8, covariance=False)
    on = lsba.bundle_adjust_boards_and_extrinsics(*args, max_iters=8, covariance=True, sigma_px=0.5)
    assert set(plain[4]) == set(off[4]) == {'before', 'after', 'report'}
    for other in (off, on):
        for a, b in zip(plain[:4], other[:4]):
            assert a.tobytes() == b.tobytes()
        for k in ('before', 'after'):
            assert plain[4][k].tobytes() == other[4][k].tobytes()
        assert plain[4]['report'] == other[4]['report']
    res = on[4]
    assert res['cov_cams'].shape == (18, 18) and res['cov_cam_blocks'].shape == (3, 6, 6)
    assert res['cov_boards'].shape == (5, 6, 6) and res['cov_status'].shape == (5,)
    assert res['cov_report']['gauge'] == 'anchor' and res['cov_report']['anchor'] == 0
    np.testing.assert_array_equal(res['cov_cam_blocks'][2], res['cov_cams'][12:18, 12:18])
    assert not res['cov_cam_blocks'][0].any()
    ref = cref.covariance(on[2], on[3].reshape(-1, 3), rig['K'], rig['D'], rig['obj'], on[0], on[1], rig['uv'],
                          rig['mask'], 1.0, 0.5, 'anchor', 0)
    assert cref.rel_error(res['cov_cams'], ref['cov_cams']) <= C_BOUND * np.linalg.cond(ref['Ah']) * EPS
    free = lsba.bundle_adjust_boards_and_extrinsics(*args, max_iters=8, covariance=True, gauge='free')[4]
    assert free['cov_report']['anchor'] is None and free['cov_cam_blocks'][0].any()
    two = lsba.bundle_adjust_boards_and_extrinsics(*args, max_iters=8, covariance=True, anchor=2)[4]
    assert two['cov_report']['anchor'] == 2 and not two['cov_cam_blocks'][2].any() and two['cov_cam_blocks'][0].any()


def test_board_poses_dropin_writes_the_covariances_and_the_same_scene(ctx, tmp_path, monkeypatch):
    from acinoset_amd.lib import app

    class _Clock:   # save_scene stamps the wall clock into the scene JSON: hold it still
        @staticmethod
        def now():
            return '2000-01-01 00:00:00'
    monkeypatch.setattr(lutils, 'datetime', _Clock)
    G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'board.npz'))
    C = len(G['K'])
    pfs = []
    for c in range(C):
        f = tmp_path / f'points_cam{c}.json'
        f.write_text(str(G[f'points_cam{c}']))
        pfs.append(str(f))
    scene = str(tmp_path / 'scene.json')
    lutils.save_scene(scene, G['K'], G['D'], G['R0'], G['t0'], tuple(int(v) for v in G['res']))
    out_a, out_b = str(tmp_path / 'a' / 'scene_sba.json'), str(tmp_path / 'b' / 'scene_sba.json')
    os.makedirs(os.path.dirname(out_a))
    os.makedirs(os.path.dirname(out_b))
    app.sba_board_poses_fisheye(scene, pfs, out_a)
    res = app.sba_board_poses_fisheye(scene, pfs, out_b, covariance=True, sigma_px=1.0)
    assert open(out_a, 'rb').read() == open(out_b, 'rb').read()
    assert sorted(os.listdir(os.path.dirname(out_a))) == ['scene_sba.json', 'scene_sba_boards.json']
    assert sorted(os.listdir(os.path.dirname(out_b))) == ['scene_sba.json', 'scene_sba_boards.json',
                                                          'scene_sba_cov.json']
    with open(os.path.join(os.path.dirname(out_b), 'scene_sba_cov.json')) as f:
        cov = json.load(f)
    assert cov['status'] == 'ok' and cov['gauge'] == 'anchor' and cov['anchor'] == 0
    assert len(cov['cameras']) == C and cov['sigma_hat_px'] > 0
    _, _, R, t, _ = lutils.load_scene(out_b, verbose=False)
    for c, cam in enumerate(cov['cameras']):
        blk = np.array(cam['cov'])
        np.testing.assert_array_equal(blk, res['cov_cam_blocks'][c])
        np.testing.assert_allclose(cam['rotation_sd'], np.sqrt(blk.diagonal()[:3]))
        np.testing.assert_allclose(cam['translation_sd'], np.sqrt(blk.diagonal()[3:]))
        np.testing.assert_allclose(cam['centre_cov'], lsba.camera_centre_covariance(blk, R[c], t[c]), rtol=1e-6,
                                   atol=1e-18)
    assert not np.array(cov['cameras'][0]['cov']).any()
    with open(os.path.join(os.path.dirname(out_a), 'scene_sba_boards.json')) as f:
        plain = json.load(f)
    with open(os.path.join(os.path.dirname(out_b), 'scene_sba_boards.json')) as f:
        boards = json.load(f)
    new = {'cov', 'rotation_sd', 'translation_sd', 'status'}
    assert len(boards['boards']) == len(plain['boards']) > 0
    for b, (x, y) in enumerate(zip(plain['boards'], boards['boards'])):
        assert set(y) - set(x) == new and {k: y[k] for k in x} == x
        assert y['status'] == 'ok'
        np.testing.assert_array_equal(np.array(y['cov']), res['cov_boards'][b])
        np.testing.assert_allclose(y['rotation_sd'], np.sqrt(res['cov_boards'][b].diagonal()[:3]))
        np.testing.assert_allclose(y['translation_sd'], np.sqrt(res['cov_boards'][b].diagonal()[3:]))
    assert {k: v for k, v in boards.items() if k != 'boards'} == {k: v for k, v in plain.items() if k != 'boards'}
