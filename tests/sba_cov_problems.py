"""The test problems of the SBA covariance tests (CPU and GPU), not a conftest.

`six` and `ring` are the problems of tests/test_gpu_sba_lanes.py (fisheye) and
tests/test_gpu_standard.py (standard model, `sm.jittered_coeffs`), same construction and seeds:
67 points with every mask of six cameras (the empty one, six single-camera ones, ...) plus three
seen by all, and 24 points seen by two to twelve cameras of a ring of twelve. Observations are
the projection of the truth + N(0, 1 px). Everything is evaluated at the oracle's solution `ref`.
Each problem is built (and solved by the oracle) once per process.
"""
import contextlib
import functools

import numpy as np

import sba_cov_ref as cref
import standard_model as sm
from oracle import fisheye, sba as osba
from acinoset_amd import _native, synth

COEFF_SEEDS = {'six': 60, 'ring': 120}


@contextlib.contextmanager
def _patched():
    """What `sm.patch_oracle` needs of a monkeypatch: setattr, undone on exit."""
    undo = []

    class Patch:
        @staticmethod
        def setattr(obj, name, value):
            undo.append((obj, name, getattr(obj, name)))
            setattr(obj, name, value)
    try:
        yield Patch
    finally:
        for obj, name, old in reversed(undo):
            setattr(obj, name, old)


class Problem:
    def __init__(self, name, model, scene, truth, mask, rng):
        self.name, self.model, self.scene, self.truth = name, model, scene, truth
        n, C = len(truth), scene.n_cams
        pi, ci = np.repeat(np.arange(n), C), np.tile(np.arange(C), n)
        if model == 'standard':
            self.D = sm.jittered_coeffs(C, COEFF_SEEDS[name])
            self.cams = _native.pack_cameras_standard(scene.K, self.D, scene.R, scene.t)
            self.project, self.project_jac = sm.project, sm.project_jac
        else:
            self.D = scene.D
            self.cams = _native.pack_cameras(scene.K, scene.D, scene.R, scene.t)
            self.project, self.project_jac = fisheye.project, fisheye.project_jac
        uv = self.project(truth[pi], scene.K[ci], self.D[ci], scene.R[ci], scene.t[ci]).reshape(n, C, 2)
        self.uv = np.ascontiguousarray(uv + rng.normal(0.0, 1.0, uv.shape))
        self.pts0 = truth + rng.normal(0.0, 0.05, truth.shape)
        self.mask = np.ascontiguousarray(mask, np.uint8)
        self.nobs = self.mask.sum(1)
        self.ref = self.solve(self.uv, self.mask, self.pts0)

    def solve(self, uv, mask, pts0):
        """The oracle's LM solution of the dense problem (uv, mask) from pts0."""
        pi, ci = np.nonzero(mask)
        s = self.scene
        if self.model == 'standard':
            with _patched() as mp:
                o = sm.patch_oracle(mp, self.D)
                return o.sba_points(uv[pi, ci], pts0, pi, ci, s.K, sm.oracle_stand_in(s.n_cams), s.R, s.t)
        return osba.sba_points(uv[pi, ci], pts0, pi, ci, s.K, s.D, s.R, s.t)

    def obs_list(self, order=None, uv=None, mask=None):
        """The observation list of the points in `order` (point ids renumbered to that order)."""
        uv = self.uv if uv is None else uv
        mask = self.mask if mask is None else mask
        order = np.arange(len(mask)) if order is None else order
        pi, ci = np.nonzero(mask[order])
        return uv[order][pi, ci], pi.astype(np.int32), ci.astype(np.int32)

    def reference(self, pts=None, uv=None, mask=None, f_scale=50.0, sigma_px=1.0):
        """The numpy helper's covariance of the dense problem (default: at the oracle's solution)."""
        uv = self.uv if uv is None else uv
        mask = self.mask if mask is None else mask
        pts = self.ref if pts is None else pts
        pi, ci = np.nonzero(mask)
        s = self.scene
        return cref.covariance(self.project_jac, uv[pi, ci], pi, ci, pts, s.K, self.D, s.R, s.t, f_scale, sigma_px)


@functools.lru_cache(maxsize=None)
def six(model='fisheye'):
    scene = synth.load_scene_file()
    truth = synth.dense_sba_problem(synth.make_sequence(4, scene, seed=11))[3][:67]
    assert len(truth) == 67
    mask = np.ones((67, 6), np.uint8)
    mask[:64] = (np.arange(64)[:, None] >> np.arange(6)) & 1
    return Problem('six', model, scene, truth, mask, np.random.default_rng(3))


@functools.lru_cache(maxsize=None)
def ring(model='fisheye'):
    scene = synth.ring_scene(12)
    truth = synth.dense_sba_problem(synth.make_sequence(2, scene, seed=11))[3][:24]
    assert len(truth) == 24
    rng = np.random.default_rng(3)
    # two to twelve cameras per point, every camera slot both used and unused; the last rows full
    mask = (rng.random((24, 12)) < 0.5).astype(np.uint8)
    mask[:, :2] |= (mask.sum(1) < 2)[:, None].astype(np.uint8)
    mask[21:] = 1
    return Problem('ring', model, scene, truth, mask, rng)


def get(name, model='fisheye'):
    return {'six': six, 'ring': ring}[name](model)


# ---- Monte-Carlo: does H^-1 predict the solver's scatter? ---------------------------------
MC_DRAWS = 2000
MC_CAMERA_SETS = ((0, 1, 2, 3, 4, 5), (0, 1), (2, 5))
MC_POINTS = (0, 1, 2)          # of six's truth


def mc_case(k):
    """Case k = 3 * camera set + point: MC_DRAWS noise draws (1 px, seed 100 + k) of one point of
    the dummy scene seen by one camera set -> (uv (n, 6, 2), mask (n, 6), pts0 (n, 3))."""
    prob = six()
    cams, X = MC_CAMERA_SETS[k // 3], prob.truth[MC_POINTS[k % 3]]
    s = prob.scene
    rng = np.random.default_rng(100 + k)
    clean = fisheye.project(np.repeat(X[None], 6, 0), s.K, s.D, s.R, s.t)
    uv = clean[None] + rng.normal(0.0, 1.0, (MC_DRAWS, 6, 2))
    mask = np.zeros((MC_DRAWS, 6), np.uint8)
    mask[:, list(cams)] = 1
    return np.ascontiguousarray(uv), mask, np.repeat(X[None], MC_DRAWS, 0)


def variance_ratios(sol, cov):
    """Sample variance of the solutions `sol` (n, 3) over the predicted one, along the
    eigenvectors of the mean predicted covariance `cov` (n, 3, 3) -> (ratios (3,), predicted sd (3,))."""
    lam, V = np.linalg.eigh(cov.mean(0))
    S = np.cov((sol - sol.mean(0)).T)
    return np.einsum('ia,ij,ja->a', V, S, V) / lam, np.sqrt(lam)
