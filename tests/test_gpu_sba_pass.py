"""Points-only SBA: what one LM pass of k_sba_lm must keep, whatever its instruction stream.

* Every group width. Dense problems of 37 points seen by C = 2 ... 64 ring cameras take the
  lane groups G = 2, 4, 8, 16, 32, 64 with one slot per lane (the register-resident camera
  records up to G = 16); the same observations as a list take the camera-id instances. The
  positions agree with the oracle to 1e-7 m (same LM spec and minimiser, as test_gpu_core.py),
  and the LM takes the oracle's decisions: equal status counts, iteration and evaluation sums.
* The throughput-grid instances: 16,392 points are one wave more than the grid that still keeps
  the camera records in registers (6 cameras: 8-lane groups reading the records from LDS) and
  one more than 4 waves per SIMD (12 cameras: 4 lanes x 3 slots). A fixed random sample of 256
  points against the oracle, as in test_gpu_fullsize.py.
* A group decides as one: the headline problem's longest chain (point 251: six accepted
  passes) and a point that ends on a rejected pass, 64 copies each, so that every group position
  of a wave holds it. All copies end with identical bits after the oracle's number of passes.
* pts_in == pts_out and separate buffers give identical bits.
"""
import os

import numpy as np
import pytest

from acinoset_amd import _native, synth, workloads
from oracle import sba as osba

pytestmark = pytest.mark.gpu

WIDTHS = (2, 3, 4, 6, 8, 12, 16, 20, 33, 64)
N_SMALL = 37
# a seed at which kernel and oracle label every point alike at every width: a point whose last
# pass meets the ftol and the xtol bound within rounding may be reported as either (seed 11 has
# one at C = 8, seed 12 one at C = 12, with equal iteration and evaluation sums)
SEED = 13
N_GRID = 16392
STATUS = {'gtol': osba.GTOL, 'ftol': osba.FTOL, 'xtol': osba.XTOL, 'stalled': osba.STALLED,
          'maxiter': osba.MAXITER, 'noobs': osba.NOOBS, 'running': osba.RUNNING}


def _oracle(scene, uv, mask, pts0, **kw):
    pi, ci = np.nonzero(mask)
    return osba.sba_points(uv[pi, ci], pts0, pi, ci, scene.K, scene.D, scene.R, scene.t, return_info=True, **kw)


def _check_counts(rep, info, n):
    assert rep['n_problems'] == n
    for name, code in STATUS.items():
        assert rep['status_counts'][name] == int((info['status'] == code).sum()), (name, rep['status_counts'])
    assert rep['iters_sum'] == int(info['iters'].sum())
    assert rep['iters_max'] == int(info['iters'].max())
    assert rep['nfev_sum'] == int(info['nfev'].sum())


@pytest.fixture(scope='module')
def widths():
    """C -> (scene, cams, uv, mask, pts0, oracle solution, oracle info) of the 37-point problems."""
    out = {}
    for C in WIDTHS:
        # two cameras: a quarter of a ring apart (two cameras facing each other leave the depth
        # along their baseline nearly free: 25 passes and a status decided by the last bit)
        scene = synth.ring_scene(4).subset([0, 1]) if C == 2 else synth.ring_scene(C)
        seq = synth.make_sequence(6, scene, seed=SEED)
        uv, mask, pts0, _, _ = synth.dense_sba_problem(seq)
        assert len(pts0) >= N_SMALL
        uv, mask, pts0 = uv[:N_SMALL].copy(), mask[:N_SMALL].copy(), pts0[:N_SMALL].copy()
        ref, info = _oracle(scene, uv, mask, pts0)
        out[C] = (scene, _native.pack_cameras(scene.K, scene.D, scene.R, scene.t), uv, mask, pts0, ref, info)
    return out


@pytest.mark.parametrize('C', WIDTHS)
def test_dense_width_matches_oracle(ctx, widths, C):
    scene, cams, uv, mask, pts0, ref, info = widths[C]
    pts, rep = ctx.sba_points_dense(cams, uv, mask, pts0)
    err = float(np.abs(pts - ref).max())
    print('C = %d dense: max |gpu - oracle| %.3e m, iters_sum %d (oracle %d), nfev_sum %d (oracle %d)' % (
        C, err, rep['iters_sum'], info['iters'].sum(), rep['nfev_sum'], info['nfev'].sum()))
    assert err < 1e-7
    _check_counts(rep, info, N_SMALL)


@pytest.mark.parametrize('C', WIDTHS)
def test_list_width_matches_oracle(ctx, widths, C):
    scene, cams, uv, mask, pts0, ref, info = widths[C]
    pi, ci = np.nonzero(mask)
    pts, _, _, rep = ctx.sba_points(cams, uv[pi, ci], pi.astype(np.int32), ci.astype(np.int32), pts0,
                                    residuals=False)
    err = float(np.abs(pts - ref).max())
    print('C = %d list: max |gpu - oracle| %.3e m, iters_sum %d (oracle %d), nfev_sum %d (oracle %d)' % (
        C, err, rep['iters_sum'], info['iters'].sum(), rep['nfev_sum'], info['nfev'].sum()))
    assert err < 1e-7
    _check_counts(rep, info, N_SMALL)


@pytest.mark.parametrize('C', [6, 12])
def test_throughput_grid_sample_matches_oracle(ctx, C):
    scene = synth.load_scene_file() if C == 6 else synth.ring_scene(12)
    assert scene.n_cams == C
    seq = synth.make_sequence(900, scene, mode='default_nolure', seed=5)
    uv, mask, pts0, _, _ = synth.dense_sba_problem(seq)
    assert len(pts0) >= N_GRID
    uv, mask, pts0 = uv[:N_GRID].copy(), mask[:N_GRID].copy(), pts0[:N_GRID].copy()
    cams = _native.pack_cameras(scene.K, scene.D, scene.R, scene.t)
    pts, rep = ctx.sba_points_dense(cams, uv, mask, pts0)
    st = rep['status_counts']
    assert st['running'] == st['stalled'] == st['maxiter'] == st['noobs'] == 0, st
    sel = np.sort(np.random.default_rng(9).choice(N_GRID, 256, replace=False))
    ref, info = _oracle(scene, uv[sel], mask[sel], pts0[sel])
    err = float(np.abs(pts[sel] - ref).max())
    print('C = %d, %d points: max |gpu - oracle| over the sample %.3e m' % (C, N_GRID, err))
    assert err < 1e-7


@pytest.fixture(scope='module')
def headline():
    """The benchmark's problem, the oracle's pass counts, and which points end on a rejection."""
    wl = workloads.sba_reference_workload()
    scene = synth.Scene(wl.K, wl.D, wl.R, wl.t, (0, 0))
    ref, info = _oracle(scene, wl.uv, wl.mask, wl.pts0)
    two = _oracle(scene, wl.uv, wl.mask, wl.pts0, max_iters=2)[0]
    # three passes, and the third moved nothing: accepted, accepted, rejected
    aar = np.nonzero((info['iters'] == 3) & (two == ref).all(1))[0]
    return wl, ref, info, aar


@pytest.mark.parametrize('which', ['six_accepted', 'ends_rejected'])
def test_group_decides_as_one(ctx, headline, which):
    wl, ref, info, aar = headline
    assert int(np.argmax(info['iters'])) == 251 and info['iters'][251] == 6 and info['nfev'][251] == 7
    assert len(aar) > 0
    p = 251 if which == 'six_accepted' else int(aar[0])
    rep_n = 64
    uv = np.ascontiguousarray(np.repeat(wl.uv[p:p + 1], rep_n, 0))
    mask = np.ascontiguousarray(np.repeat(wl.mask[p:p + 1], rep_n, 0))
    pts0 = np.ascontiguousarray(np.repeat(wl.pts0[p:p + 1], rep_n, 0))
    pts, rep = ctx.sba_points_dense(wl.cams, uv, mask, pts0)
    print('point %d x %d: iters_sum %d (oracle %d each), max |gpu - oracle| %.3e m' % (
        p, rep_n, rep['iters_sum'], info['iters'][p], np.abs(pts - ref[p]).max()))
    np.testing.assert_array_equal(pts.view(np.uint64), np.repeat(pts[:1], rep_n, 0).view(np.uint64))
    assert rep['iters_sum'] == rep_n * int(info['iters'][p]) and rep['iters_max'] == int(info['iters'][p])
    assert rep['nfev_sum'] == rep_n * int(info['nfev'][p])
    assert float(np.abs(pts - ref[p]).max()) < 1e-7


@pytest.mark.parametrize('n', [1, 9])
def test_in_place_equals_out_of_place(ctx, widths, n):
    import torch
    _, cams, uv, mask, pts0, ref, _ = widths[6]
    dev = torch.device('cuda', int(os.environ.get('ACINOSET_DEVICE', 0)))
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
         dict(cams=cams, uv=uv[:n], mask=mask[:n], pts0=pts0[:n]).items()}
    inplace = d['pts0'].clone()
    ctx.sba_points_dense_dev(d['cams'].data_ptr(), 6, d['uv'].data_ptr(), d['mask'].data_ptr(), n, inplace.data_ptr())
    out = torch.full((n, 3), float('nan'), dtype=torch.float64, device=dev)
    ctx.sba_points_dense_dev(d['cams'].data_ptr(), 6, d['uv'].data_ptr(), d['mask'].data_ptr(), n, out.data_ptr(),
                             pts_in_p=d['pts0'].data_ptr())
    ctx.sync()
    a, b = inplace.cpu().numpy(), out.cpu().numpy()
    np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64))
    assert float(np.abs(a - ref[:n]).max()) < 1e-7
    np.testing.assert_array_equal(d['pts0'].cpu().numpy(), pts0[:n])
