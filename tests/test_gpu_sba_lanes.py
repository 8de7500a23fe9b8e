"""Points-only SBA: every observation mask of a lane group, and independence of where in the
batch (which lanes of which wave) a point sits.

The 6-camera problem has 67 points: one per subset of the six cameras (64 masks: the empty
one, six single-camera ones, ...) and three more with every camera. Every camera's observation
is the projection of the true point + N(0, 1 px); the start is the truth + N(0, 0.05 m). The
oracle solves all of it in at most 8 iterations (one NOOBS, the rest XTOL / FTOL).

Tolerances, as in test_gpu_core.py: 1e-7 m against the oracle for points with two or more
observations (same LM spec and minimiser), 1e-6 m for the single-camera points (rank-2
Gauss-Newton matrix: the depth along the ray is free). A point's lanes sum in a fixed order
whatever its neighbours are, so rolling the batch must not change a single bit of its result.
"""
import os

import numpy as np
import pytest

from oracle import fisheye, sba as osba
from acinoset_amd import _native, synth

pytestmark = pytest.mark.gpu

ROLLS = (1, 3, 8)


def _observe(scene, truth, rng):
    """(n, C, 2) observations of every point by every camera, 1 px noise."""
    n, C = len(truth), scene.n_cams
    pi, ci = np.repeat(np.arange(n), C), np.tile(np.arange(C), n)
    uv = fisheye.project(truth[pi], scene.K[ci], scene.D[ci], scene.R[ci], scene.t[ci]).reshape(n, C, 2)
    return uv + rng.normal(0.0, 1.0, uv.shape)


class Problem:
    def __init__(self, scene, truth, mask, rng):
        self.scene = scene
        self.cams = _native.pack_cameras(scene.K, scene.D, scene.R, scene.t)
        self.uv = np.ascontiguousarray(_observe(scene, truth, rng))
        self.pts0 = truth + rng.normal(0.0, 0.05, truth.shape)
        self.mask = np.ascontiguousarray(mask, np.uint8)
        self.nobs = self.mask.sum(1)
        self.ref, self.info = self.oracle(self.mask)

    def oracle(self, mask, n=None):
        n = len(mask) if n is None else n
        pi, ci = np.nonzero(mask[:n])
        s = self.scene
        return osba.sba_points(self.uv[pi, ci], self.pts0[:n], pi, ci, s.K, s.D, s.R, s.t, return_info=True)

    def obs_list(self, order):
        """The observation list of the points in `order` (point ids renumbered to that order)."""
        pi, ci = np.nonzero(self.mask[order])
        return self.uv[order][pi, ci], pi.astype(np.int32), ci.astype(np.int32)


@pytest.fixture(scope='module')
def six():
    scene = synth.load_scene_file()
    seq = synth.make_sequence(4, scene, seed=11)
    truth = synth.dense_sba_problem(seq)[3][:67]
    assert len(truth) == 67
    mask = np.ones((67, 6), np.uint8)
    mask[:64] = (np.arange(64)[:, None] >> np.arange(6)) & 1
    return Problem(scene, truth, mask, np.random.default_rng(3))


@pytest.fixture(scope='module')
def ring():
    scene = synth.ring_scene(12)
    seq = synth.make_sequence(2, scene, seed=11)
    truth = synth.dense_sba_problem(seq)[3][:24]
    assert len(truth) == 24
    rng = np.random.default_rng(3)
    # two to twelve cameras per point, every camera slot both used and unused; the last rows full
    mask = (rng.random((24, 12)) < 0.5).astype(np.uint8)
    mask[:, :2] |= (mask.sum(1) < 2)[:, None].astype(np.uint8)
    mask[21:] = 1
    return Problem(scene, truth, mask, rng)


def _check_oracle(prob, pts, rep):
    many, one, none = prob.nobs >= 2, prob.nobs == 1, prob.nobs == 0
    print('max |gpu - oracle|: >= 2 obs %.3e m, 1 obs %.3e m' % (
        np.abs(pts - prob.ref)[many].max(), np.abs(pts - prob.ref)[one].max() if one.any() else 0.0))
    assert prob.info['iters'].max() <= 8
    assert np.abs(pts - prob.ref)[many].max() < 1e-7
    if one.any():
        assert np.abs(pts - prob.ref)[one].max() < 1e-6
    np.testing.assert_array_equal(pts[none], prob.pts0[none])
    assert rep['status_counts']['noobs'] == int(none.sum())
    assert rep['status_counts']['maxiter'] == 0 and rep['status_counts']['stalled'] == 0
    assert rep['n_problems'] == len(pts)


def _check_rolls(solve, n):
    base = solve(np.arange(n))
    for k in ROLLS:
        order = np.roll(np.arange(n), k)
        back = np.empty_like(base)
        back[order] = solve(order)
        np.testing.assert_array_equal(back.view(np.uint64), base.view(np.uint64), err_msg=f'roll by {k}')


@pytest.mark.parametrize('name', ['six', 'ring'])
def test_dense_matches_oracle(ctx, request, name):
    prob = request.getfixturevalue(name)
    pts, rep = ctx.sba_points_dense(prob.cams, prob.uv, prob.mask, prob.pts0)
    _check_oracle(prob, pts, rep)


@pytest.mark.parametrize('name', ['six', 'ring'])
def test_dense_is_lane_position_independent(ctx, request, name):
    prob = request.getfixturevalue(name)
    _check_rolls(lambda o: ctx.sba_points_dense(prob.cams, prob.uv[o], prob.mask[o], prob.pts0[o])[0], len(prob.pts0))


def test_list_matches_oracle(ctx, six):
    uv, pi, ci = six.obs_list(np.arange(67))
    pts, _, _, rep = ctx.sba_points(six.cams, uv, pi, ci, six.pts0, residuals=False)
    _check_oracle(six, pts, rep)


def test_list_is_lane_position_independent(ctx, six):
    def solve(order):
        uv, pi, ci = six.obs_list(order)
        return ctx.sba_points(six.cams, uv, pi, ci, six.pts0[order], residuals=False)[0]
    _check_rolls(solve, 67)


@pytest.fixture(scope='module')
def full9(six):
    """The first nine points seen by every camera, and the oracle's solution of them."""
    mask = np.ones((9, 6), np.uint8)
    return mask, six.oracle(mask, 9)[0]


@pytest.mark.parametrize('n', [1, 7, 8, 9])
def test_sizes_in_place(ctx, six, full9, n):
    mask, ref = full9
    pts, rep = ctx.sba_points_dense(six.cams, six.uv[:n], mask[:n], six.pts0[:n])
    print('n = %d: max |gpu - oracle| %.3e m' % (n, np.abs(pts - ref[:n]).max()))
    assert pts.shape == (n, 3) and rep['n_problems'] == n
    assert np.abs(pts - ref[:n]).max() < 1e-7


@pytest.mark.parametrize('n', [1, 7, 8, 9])
def test_sizes_separate_buffers(ctx, six, full9, n):
    import torch
    mask, ref = full9
    dev = torch.device('cuda', int(os.environ.get('ACINOSET_DEVICE', 0)))
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
         dict(cams=six.cams, uv=six.uv[:n], mask=mask[:n], pts0=six.pts0[:n]).items()}
    # one more row than the solve may write, to see that it stops at n
    out = torch.full((n + 1, 3), float('nan'), dtype=torch.float64, device=dev)
    ctx.sba_points_dense_dev(d['cams'].data_ptr(), 6, d['uv'].data_ptr(), d['mask'].data_ptr(), n, out.data_ptr(),
                             pts_in_p=d['pts0'].data_ptr())
    ctx.sync()
    got = out.cpu().numpy()
    assert np.abs(got[:n] - ref[:n]).max() < 1e-7
    assert np.isnan(got[n]).all()
    np.testing.assert_array_equal(d['pts0'].cpu().numpy(), six.pts0[:n])
