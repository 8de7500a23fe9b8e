"""GPU parity: projection, residual vector, loss, FK and points-only SBA through the
C ABI, against the oracle and the reference's golden vectors.

Tolerances (float64 on both sides):
  * projection / residuals: 1e-9 px; loss: 1e-12; FK: 1e-12 m; FK Jacobian: 1e-10
  * SBA points vs oracle: 1e-7 m max (same LM spec and minimiser; slowly converging
    outlier points stop on xtol at slightly different iterates, most agree to 1e-15)
  * SBA points vs reference (scipy TRF, stops at xtol=1e-8): 1e-5 m max, 1e-6 m RMS
    (north_star contract: 1e-4 m RMS)
"""
import numpy as np
import pytest

from conftest import golden
from oracle import fisheye, kinematics as okin, sba as osba
from acinoset_amd import _native, kinematics as pkin, synth

pytestmark = pytest.mark.gpu


def _cams(g):
    return _native.pack_cameras(g['K'], g['D'], g['R'], g['t'])


def test_projection_matches_oracle(ctx):
    g = golden('sba_cfg2')
    rng = np.random.default_rng(0)
    X = g['points_3d'] + rng.normal(0, 0.05, g['points_3d'].shape)
    ci = rng.integers(0, 6, len(X)).astype(np.int32)
    uv = ctx.project(_cams(g), X, ci)
    ref = fisheye.project(X, g['K'][ci], g['D'][ci], g['R'][ci], g['t'][ci])
    np.testing.assert_allclose(uv, ref, rtol=0, atol=1e-9)
    uvf = ctx.project(_cams(g), X, ci, fte_form=True)
    reff = fisheye.project(X, g['K'][ci], g['D'][ci], g['R'][ci], g['t'][ci], fte_form=True)
    np.testing.assert_allclose(uvf, reff, rtol=0, atol=1e-9)


@pytest.mark.parametrize('name', ['sba_cfg1', 'sba_cfg2'])
def test_residuals_match_reference(ctx, name):
    g = golden(name)
    r = ctx.sba_residuals(_cams(g), g['points_2d'], g['point_indices'], g['camera_indices'], g['points_3d'])
    np.testing.assert_allclose(r, g['resid_before'], rtol=0, atol=1e-9)


def test_loss_matches_reference(ctx):
    g = golden('loss')
    v, d = ctx.redescending_loss(g['err'], 3.0, 10.0, 20.0, deriv=True)
    np.testing.assert_allclose(v, g['loss'], rtol=1e-13, atol=1e-13)
    d1, _ = okin.loss_derivs(g['err'])
    np.testing.assert_allclose(d, d1, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('mode', ['default', 'head', 'upper_body', 'head_stabilize'])
@pytest.mark.parametrize('inter', ['pos', 'vel', 'acc'])
@pytest.mark.parametrize('dirs', [0, 1])
def test_fk_matches_reference(ctx, mode, inter, dirs):
    g = golden('fk')
    t = pkin.build_table(mode)
    im = {'pos': 0, 'vel': 1, 'acc': 2}[inter]
    out = ctx.fk(t, g[f'{mode}_x'], g[f'{mode}_dx'], g[f'{mode}_ddx'], g[f'{mode}_tau'], intermode=im,
                 directions=bool(dirs))
    np.testing.assert_allclose(out, g[f'{mode}_{inter}_{dirs}'], rtol=0, atol=1e-12)


@pytest.mark.parametrize('mode', ['default', 'default_nolure', 'head', 'upper_body', 'head_stabilize'])
def test_fk_jacobian_matches_complex_step(ctx, mode):
    t = pkin.build_table(mode)
    rng = np.random.default_rng(3)
    x = rng.normal(0, 0.5, (32, t.P))
    x[:, :3] += [1.9, 6.4, 0.6]
    pos, J = ctx.fk(t, x, jac=True)
    np.testing.assert_allclose(pos, okin.marker_positions(mode, x), atol=1e-12)
    np.testing.assert_allclose(J, okin.marker_jacobian(mode, x), atol=1e-10)


@pytest.mark.parametrize('name', ['sba_cfg1', 'sba_cfg2'])
def test_sba_points_matches_reference_and_oracle(ctx, name):
    g = golden(name)
    pts, rb, ra, rep = ctx.sba_points(_cams(g), g['points_2d'], g['point_indices'], g['camera_indices'],
                                      g['points_3d'])
    np.testing.assert_allclose(rb, g['resid_before'], rtol=0, atol=1e-9)
    d_ref = np.linalg.norm(pts - g['pts_out'], axis=1)
    assert np.sqrt(np.mean(d_ref ** 2)) < 1e-6 and d_ref.max() < 1e-5
    x_or, info = osba.sba_points(g['points_2d'], g['points_3d'], g['point_indices'], g['camera_indices'],
                                 g['K'], g['D'], g['R'], g['t'], return_info=True)
    assert np.abs(pts - x_or).max() < 1e-7
    np.testing.assert_allclose(ra, g['resid_after'], atol=1e-3)
    assert rep['n_problems'] == len(pts)
    assert rep['status_counts']['maxiter'] == 0 and rep['status_counts']['stalled'] == 0
    np.testing.assert_allclose(rep['cost_before'], info['cost_before'].sum(), rtol=1e-12)
    np.testing.assert_allclose(rep['cost_after'], info['cost_after'].sum(), rtol=1e-12)


def test_sba_dense_matches_oracle_12cam(ctx):
    scene = synth.ring_scene(12)
    seq = synth.make_sequence(120, scene, seed=5)
    uv, mask, pts0, truth, _ = synth.dense_sba_problem(seq)
    cams = _native.pack_cameras(scene.K, scene.D, scene.R, scene.t)
    pts, rep = ctx.sba_points_dense(cams, uv, mask, pts0)
    pi, ci = np.nonzero(mask)
    x_or = osba.sba_points(uv[pi, ci], pts0, pi, ci, scene.K, scene.D, scene.R, scene.t)
    assert np.abs(pts - x_or).max() < 1e-7
    assert np.sqrt(np.mean(np.sum((pts - truth) ** 2, 1))) < 0.01  # 1 px noise at ~6 m
    # the list API on the same problem (compacted slots, different lane order)
    pts2, _, _, _ = ctx.sba_points(cams, uv[pi, ci], pi, ci, pts0, residuals=False)
    assert np.abs(pts - pts2).max() < 1e-7  # xtol 1e-9 stops differ by summation order


def test_sba_deterministic(ctx):
    g = golden('sba_cfg2')
    a = ctx.sba_points(_cams(g), g['points_2d'], g['point_indices'], g['camera_indices'], g['points_3d'])
    b = ctx.sba_points(_cams(g), g['points_2d'], g['point_indices'], g['camera_indices'], g['points_3d'])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])


def test_sba_edge_cases(ctx):
    g = golden('sba_cfg1')
    cams = _cams(g)
    # empty observation list
    pts, rb, ra, rep = ctx.sba_points(cams, np.zeros((0, 2)), np.zeros(0, np.int32), np.zeros(0, np.int32),
                                      g['points_3d'])
    assert np.array_equal(pts, g['points_3d'])
    # a point with no observations keeps its value; a duplicated observation is allowed
    p2 = np.concatenate([g['points_2d'], g['points_2d'][:1]])
    pi = np.concatenate([g['point_indices'], g['point_indices'][:1]])
    ci = np.concatenate([g['camera_indices'], g['camera_indices'][:1]])
    p3 = np.concatenate([g['points_3d'], [[1.0, 2.0, 3.0]]])
    pts, rb, ra, rep = ctx.sba_points(cams, p2, pi, ci, p3)
    assert np.array_equal(pts[-1], [1.0, 2.0, 3.0])
    assert rep['status_counts']['noobs'] == 1
    x_or = osba.sba_points(p2, p3, pi, ci, g['K'], g['D'], g['R'], g['t'])
    assert np.abs(pts - x_or).max() < 1e-7
    # out-of-range point index -> error, not a crash
    with pytest.raises(RuntimeError):
        ctx.sba_points(cams, g['points_2d'], g['point_indices'] + 10 ** 6, g['camera_indices'], g['points_3d'])


def test_sba_single_observation_points(ctx):
    """Degenerate points seen by one camera (rank-2 Gauss-Newton matrix): the solve must
    follow the oracle (a damped matrix that is not positive definite raises lambda instead
    of stopping on a zero step) and reproject onto the observation."""
    g = golden('sba_cfg1')
    rng = np.random.default_rng(0)
    n = 64
    X = g['points_3d'][:n] + rng.normal(0, 0.05, (n, 3))
    ci = (np.arange(n) % 2).astype(np.int32)
    pi = np.arange(n, dtype=np.int32)
    uv = fisheye.project(g['points_3d'][:n], g['K'][ci], g['D'][ci], g['R'][ci], g['t'][ci]) + 1.0
    pts, rb, ra, rep = ctx.sba_points(_cams(g), uv, pi, ci, X)
    x_or, info = osba.sba_points(uv, X, pi, ci, g['K'], g['D'], g['R'], g['t'], return_info=True)
    counts = np.bincount(info['status'], minlength=7)
    names = ['running', 'gtol', 'ftol', 'xtol', 'stalled', 'maxiter', 'noobs']
    ref = dict(zip(names, counts.tolist()))
    got = {k: rep['status_counts'][k] for k in names}
    # gtol vs xtol may swap on one point: the oracle's point 20 stops with its gradient between
    # 5e-11 and 1e-10 (gtol = 1e-10 stops it, 5e-11 lets it take one more step to xtol at the
    # same position, 6e-15 apart), i.e. the gradient of a free-depth point is rounding noise at
    # the gtol boundary and the rounding decides. Every other status count is exact.
    assert {k: v for k, v in got.items() if k not in ('gtol', 'xtol')} == \
        {k: v for k, v in ref.items() if k not in ('gtol', 'xtol')}
    assert got['gtol'] + got['xtol'] == ref['gtol'] + ref['xtol'] and abs(got['gtol'] - ref['gtol']) <= 1, (got, ref)
    assert np.abs(ra).max() < 1e-9  # reprojects exactly (the depth along the ray is free)
    assert np.abs(pts - x_or).max() < 1e-6
    # Point by point: each of the 64 solved alone (a point's place in the wave does not change its
    # result: test_gpu_sba_lanes.py) must end with the oracle's status. Only the boundary point may
    # differ, between gtol and xtol and at the oracle's position; the aggregate is then the oracle's
    # with that one point's label exchanged, exactly.
    BOUNDARY = 20
    alone = np.empty(n, np.int64)
    for p in range(n):
        one, _, _, rp = ctx.sba_points(_cams(g), uv[p:p + 1], np.zeros(1, np.int32), ci[p:p + 1], X[p:p + 1],
                                       residuals=False)
        hit = [k for k in names if rp['status_counts'][k]]
        assert len(hit) == 1 and rp['n_problems'] == 1, rp
        alone[p] = names.index(hit[0])
        np.testing.assert_array_equal(one[0].view(np.uint64), pts[p].view(np.uint64))
    others = np.arange(n) != BOUNDARY
    np.testing.assert_array_equal(alone[others], info['status'][others])
    assert info['status'][BOUNDARY] in (osba.GTOL, osba.XTOL) and alone[BOUNDARY] in (osba.GTOL, osba.XTOL)
    assert np.abs(pts[BOUNDARY] - x_or[BOUNDARY]).max() < 1e-12
    want = np.bincount(np.where(others, info['status'], alone[BOUNDARY]), minlength=7)
    assert got == dict(zip(names, want.tolist())), (got, ref)
    print('single-observation points: boundary point %d is %s on the GPU, %s in the oracle' % (
        BOUNDARY, names[alone[BOUNDARY]], names[info['status'][BOUNDARY]]))


def test_sba_dense_io_matches_inplace(ctx):
    """acs_sba_points_dense_io: separate initial/solution buffers give the in-place result
    bit for bit and leave the initial points untouched (incl. a point with no views)."""
    import torch
    scene = synth.load_scene_file()
    seq = synth.make_sequence(50, scene, seed=11)
    uv, mask, pts0, _, _ = synth.dense_sba_problem(seq)
    mask = mask.copy()
    mask[3] = 0  # no observations: passes through
    cams = _native.pack_cameras(scene.K, scene.D, scene.R, scene.t)
    ref, _ = ctx.sba_points_dense(cams, uv, mask, pts0)
    dev = torch.device('cuda', 0)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
         dict(cams=cams, uv=uv, mask=mask, pts0=pts0).items()}
    out = torch.full_like(d['pts0'], float('nan'))
    ctx.sba_points_dense_dev(d['cams'].data_ptr(), len(cams), d['uv'].data_ptr(), d['mask'].data_ptr(), len(pts0),
                             out.data_ptr(), pts_in_p=d['pts0'].data_ptr())
    ctx.sync()
    np.testing.assert_array_equal(out.cpu().numpy(), ref)
    np.testing.assert_array_equal(d['pts0'].cpu().numpy(), pts0)
    np.testing.assert_array_equal(ref[3], pts0[3])


def test_context_keeps_caller_device(ctx):
    """Every entry point makes the context's device current for its own work and restores
    the caller's current device (torch shares the HIP runtime's current device)."""
    import torch
    n = torch.cuda.device_count()
    dev = n - 1
    torch.cuda.set_device(0)
    c = _native.Context(dev)
    g = golden('sba_cfg1')
    a = c.sba_points(_cams(g), g['points_2d'], g['point_indices'], g['camera_indices'], g['points_3d'])[0]
    assert torch.cuda.current_device() == 0
    b = ctx.sba_points(_cams(g), g['points_2d'], g['point_indices'], g['camera_indices'], g['points_3d'])[0]
    np.testing.assert_array_equal(a, b)
    if n > 1:
        # two contexts on two devices, used alternately from a thread whose current device
        # is neither's: workspace and launches follow each context
        torch.cuda.set_device(0)
        c0 = _native.Context(0)
        for _ in range(2):
            np.testing.assert_array_equal(c.sba_points(_cams(g), g['points_2d'], g['point_indices'],
                                                       g['camera_indices'], g['points_3d'])[0], b)
            np.testing.assert_array_equal(c0.sba_points(_cams(g), g['points_2d'], g['point_indices'],
                                                        g['camera_indices'], g['points_3d'])[0], b)
        assert torch.cuda.current_device() == 0
