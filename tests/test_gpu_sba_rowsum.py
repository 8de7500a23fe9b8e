"""Points-only SBA: the row instance of k_sba_lm (one point per 16-lane DPP row, group sums by
row broadcast) against the butterfly instance, on one build (Context.sba_set_lm_layout).

* The instances agree in every bit: C = 3 ... 8 cameras (the three broadcast trees: 2, 3 and 4 lane
  pairs, each with its last slot empty and filled) at 1, 3, 4, 5 and 37 points (four points fill a
  wave; five leave a wave with one live row). Equal positions as uint64, equal status counts,
  iteration and evaluation sums, and both within 1e-7 m of the oracle (the bound of
  test_gpu_sba_pass.py).
* Mask edge cases at C = 6 and 8: a point without any observation, with slot 0 only, with slot
  K - 1 only, with one odd slot only (a pair whose partner is empty). The same equalities, and
  the oracle's NOOBS count. A point seen by one camera is rank deficient (two residuals, three
  unknowns: the damping alone decides its steps), so the oracle bound is asserted on the rows
  left as they were and printed for the four overwritten ones.
* Selection: 16 n_cu points (one wave per SIMD at 4 points per wave) take the row instance, one
  point more takes the butterfly; both equal the forced butterfly run bit for bit, and a fixed
  sample of 64 points is within 1e-7 m of the oracle.
* pts_in == pts_out and separate buffers give identical bits on the row instance (n = 5).
"""
import os

import numpy as np
import pytest

from acinoset_amd import _native, synth
from oracle import sba as osba

pytestmark = pytest.mark.gpu

CAMS = (3, 4, 5, 6, 7, 8)
SIZES = (1, 3, 4, 5, 37)
N_SMALL = 37
SEED = 13
REP_KEYS = ('status_counts', 'iters_sum', 'iters_max', 'nfev_sum')


def _oracle(scene, uv, mask, pts0):
    pi, ci = np.nonzero(mask)
    return osba.sba_points(uv[pi, ci], pts0, pi, ci, scene.K, scene.D, scene.R, scene.t, return_info=True)


def _scene(C):
    return synth.load_scene_file() if C == 6 else synth.ring_scene(C)


@pytest.fixture(scope='module')
def problems():
    """C -> (scene, cams, uv, mask, pts0, oracle solution, oracle info) of the 37-point problems.
    The points are independent, so the first n rows are the n-point problem and its solution."""
    out = {}
    for C in CAMS:
        scene = _scene(C)
        assert scene.n_cams == C
        seq = synth.make_sequence(6, scene, seed=SEED)
        uv, mask, pts0, _, _ = synth.dense_sba_problem(seq)
        assert len(pts0) >= N_SMALL
        uv, mask, pts0 = uv[:N_SMALL].copy(), mask[:N_SMALL].copy(), pts0[:N_SMALL].copy()
        ref, info = _oracle(scene, uv, mask, pts0)
        out[C] = (scene, _native.pack_cameras(scene.K, scene.D, scene.R, scene.t), uv, mask, pts0, ref, info)
    return out


def _solve(ctx, layout, expect, cams, uv, mask, pts0):
    """One dense solve under `layout`, after asserting that it launches the `expect` instance."""
    ctx.sba_set_lm_layout(layout)
    try:
        assert ctx.sba_lm_layout(mask.shape[1], len(pts0))[0] == expect
        return ctx.sba_points_dense(cams, uv, mask, pts0)
    finally:
        ctx.sba_set_lm_layout('auto')


def _assert_same(a, b):
    (pa, ra), (pb, rb) = a, b
    np.testing.assert_array_equal(pa.view(np.uint64), pb.view(np.uint64))
    for k in REP_KEYS:
        assert ra[k] == rb[k], (k, ra[k], rb[k])


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('C', CAMS)
def test_row_equals_butterfly(ctx, problems, C, n):
    _, cams, uv, mask, pts0, ref, _ = problems[C]
    uv, mask, pts0 = uv[:n].copy(), mask[:n].copy(), pts0[:n].copy()
    fly = _solve(ctx, 'butterfly', 'butterfly', cams, uv, mask, pts0)
    row = _solve(ctx, 'row', 'row', cams, uv, mask, pts0)
    eb, er = float(np.abs(fly[0] - ref[:n]).max()), float(np.abs(row[0] - ref[:n]).max())
    print('C = %d, n = %d: max |butterfly - oracle| %.3e m, |row - oracle| %.3e m, iters_sum %d / %d' % (
        C, n, eb, er, fly[1]['iters_sum'], row[1]['iters_sum']))
    _assert_same(fly, row)
    assert eb < 1e-7 and er < 1e-7


@pytest.mark.parametrize('C', [6, 8])
def test_mask_edges(ctx, problems, C):
    scene, cams, uv, mask, pts0, _, _ = problems[C]
    mask = mask.copy()
    mask[:4] = 0
    mask[1, 0] = 1      # slot 0 only
    mask[2, C - 1] = 1  # slot K - 1 only
    mask[3, 3] = 1      # an odd slot only: its pair partner (slot 2) is empty
    ref, info = _oracle(scene, uv, mask, pts0)
    fly = _solve(ctx, 'butterfly', 'butterfly', cams, uv, mask, pts0)
    row = _solve(ctx, 'row', 'row', cams, uv, mask, pts0)
    for name, (pts, rep) in (('butterfly', fly), ('row', row)):
        print('C = %d %s: max |gpu - oracle| rows 4.. %.3e m, one-camera rows 1-3 %.3e m, noobs %d (oracle %d)' % (
            C, name, np.abs(pts[4:] - ref[4:]).max(), np.abs(pts[1:4] - ref[1:4]).max(), rep['status_counts']['noobs'],
            (info['status'] == osba.NOOBS).sum()))
    _assert_same(fly, row)
    for pts, rep in (fly, row):
        assert rep['status_counts']['noobs'] == int((info['status'] == osba.NOOBS).sum()) == 1
        np.testing.assert_array_equal(pts[0], pts0[0])  # no observation: untouched
        assert float(np.abs(pts[4:] - ref[4:]).max()) < 1e-7


def test_selection_boundary(ctx):
    scene = synth.load_scene_file()
    C = scene.n_cams
    assert C == 6
    n_cu = ctx.sba_lm_layout(C, 1)[1]
    n_row = 16 * n_cu
    seq = synth.make_sequence((n_row + 1) // 20 + 30, scene, mode='default_nolure', seed=5)
    uv, mask, pts0, _, _ = synth.dense_sba_problem(seq)
    assert len(pts0) >= n_row + 1
    cams = _native.pack_cameras(scene.K, scene.D, scene.R, scene.t)
    sel = np.sort(np.random.default_rng(9).choice(n_row, 64, replace=False))
    ref, _ = _oracle(scene, uv[sel], mask[sel], pts0[sel])
    for n, expect in ((n_row, 'row'), (n_row + 1, 'butterfly')):
        a = (uv[:n].copy(), mask[:n].copy(), pts0[:n].copy())
        auto = _solve(ctx, 'auto', expect, cams, *a)
        fly = _solve(ctx, 'butterfly', 'butterfly', cams, *a)
        err = float(np.abs(auto[0][sel] - ref).max())
        print('%d points (%d CUs): %s instance, max |gpu - oracle| over the sample %.3e m' % (n, n_cu, expect, err))
        _assert_same(auto, fly)
        assert err < 1e-7


def test_row_in_place_equals_out_of_place(ctx, problems):
    import torch
    n = 5
    _, cams, uv, mask, pts0, ref, _ = problems[6]
    dev = torch.device('cuda', int(os.environ.get('ACINOSET_DEVICE', 0)))
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
         dict(cams=cams, uv=uv[:n], mask=mask[:n], pts0=pts0[:n]).items()}
    inplace = d['pts0'].clone()
    out = torch.full((n, 3), float('nan'), dtype=torch.float64, device=dev)
    ctx.sba_set_lm_layout('row')
    try:
        assert ctx.sba_lm_layout(6, n)[0] == 'row'
        ctx.sba_points_dense_dev(d['cams'].data_ptr(), 6, d['uv'].data_ptr(), d['mask'].data_ptr(), n,
                                 inplace.data_ptr())
        ctx.sba_points_dense_dev(d['cams'].data_ptr(), 6, d['uv'].data_ptr(), d['mask'].data_ptr(), n, out.data_ptr(),
                                 pts_in_p=d['pts0'].data_ptr())
        ctx.sync()
    finally:
        ctx.sba_set_lm_layout('auto')
    a, b = inplace.cpu().numpy(), out.cpu().numpy()
    np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64))
    assert float(np.abs(a - ref[:n]).max()) < 1e-7
    np.testing.assert_array_equal(d['pts0'].cpu().numpy(), pts0[:n])
