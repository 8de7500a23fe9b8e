"""GPU parity of acs_sba_extrinsics with oracle/sba_ext.py at every lane group, Schur chunking and stop
path that test_gpu_sba_ext.py does not reach (it has G = 8 and 16, K <= C, the maxiter and ftol stops).
The problems, the table of shapes and the rules they are chosen by are in sba_ext_shapes.py;
test_sba_ext_shapes_cpu.py checks on the oracle alone that these runs may be compared at these
tolerances (no decision near a tie, no stop on its threshold). Every test asserts through
acs_sba_ext_plan the lane group, chunk and chunk count it claims to reach.

Tolerances: those of test_sba_ext_matches_oracle. Status, iterations and acceptances equal; lambda and
both costs 1e-12 relative; points and translations 1e-9 m; rotations 1e-10; resid_before 1e-9 px,
resid_after 1e-8 px; R R^T = I to 1e-12; intrinsics untouched; no bad pivot.

  - 8 iterations on every shape: G = 2, 4, 32, 64; K = 1, 2, 3, 4, 17, 20, 33, 40, 64 = EXT_MAXK; cameras
    repeated within a point (K > C: ext_schur_entry sums several slots of one camera); one chunk, two
    full chunks, several with a ragged last one; one camera. The point without observation comes back
    bit-equal, the point one camera sees is held to the full tolerance.
  - max_iters = 0..5 on the smallest and the largest lane group: a stop at every position of the
    four-iteration replay, and no step at all.
  - to convergence on the same two, one run each for the ftol, xtol and gtol stop, at the tolerance
    sba_ext_shapes.STOPS records. The depth of the point one camera sees is free there, so its
    position (and only its) is left out; its residuals are compared.
  - two runs bit-identical; 65 observations of a point refused; the rank solve on the new shapes.
"""
import numpy as np
import pytest

import sba_ext_shapes as S
from acinoset_amd import _native, dist

pytestmark = pytest.mark.gpu

IDS = [S.shape_id(s) for s in S.SHAPES]
CONV = sorted(S.STOPS, key=lambda k: (k[0].K, k[1]))
CONV_IDS = [f'{S.shape_id(s)}-{kind}' for s, kind in CONV]
REPORT = ('status', 'iters', 'n_accepted', 'n_bad_pivots', 'cost_before', 'cost_after', 'grad_max', 'lambda_final')


def _cams(p):
    return _native.pack_cameras(p.K, p.D, p.R0, p.t0)


def _solve(ctx, s, **opts):
    p = S.problem(s)
    assert _native.sba_ext_plan(s.n, int(np.bincount(p.pi).max())) == dict(G=s.G, chunk=s.chunk, nchunk=s.nchunk)
    return ctx.sba_extrinsics(_cams(p), p.uv, p.pi, p.ci, p.X0, ctx.sba_ext_opts(**opts))


def _check_parity(s, got, ref, skip_point=None):
    p = S.problem(s)
    cams, X, rb, ra, rep = got
    info = ref.info
    R, t = cams[:, 8:17].reshape(-1, 3, 3), cams[:, 17:20]
    keep = np.arange(s.n) != skip_point
    start = ref._replace(X=p.X0, R=p.R0, t=p.t0)
    diffs = dict(points=np.abs(X - ref.X)[keep].max(), translations=np.abs(t - ref.t).max(),
                 rotations=np.abs(R - ref.R).max(), resid_before=np.abs(rb - S.residuals(p, start)).max(),
                 resid_after=np.abs(ra - S.residuals(p, ref)).max(),
                 cost_before=abs(rep['cost_before'] / info['cost_before'] - 1),
                 cost_after=abs(rep['cost_after'] / info['cost_after'] - 1),
                 lam=abs(rep['lambda_final'] / info['lam'] - 1),
                 orthogonality=np.abs(R @ np.swapaxes(R, 1, 2) - np.eye(3)).max())
    print(f'\n{S.shape_id(s)} {rep["status_name"]} {rep["iters"]}/{rep["n_accepted"]} (oracle {info["status"]} '
          f'{info["iters"]}/{info["n_accepted"]}) ' + ' '.join(f'{k} {v:.1e}' for k, v in diffs.items()))
    assert rep['status_name'] == info['status']
    assert rep['iters'] == info['iters'] and rep['n_accepted'] == info['n_accepted']
    assert rep['n_bad_pivots'] == 0
    assert diffs['lam'] <= 1e-12 and diffs['cost_before'] <= 1e-12 and diffs['cost_after'] <= 1e-12
    assert diffs['points'] <= 1e-9 and diffs['translations'] <= 1e-9 and diffs['rotations'] <= 1e-10
    assert diffs['resid_before'] <= 1e-9 and diffs['resid_after'] <= 1e-8
    assert diffs['orthogonality'] <= 1e-12
    np.testing.assert_array_equal(cams[:, :8], _cams(p)[:, :8])  # intrinsics untouched
    np.testing.assert_array_equal(X[s.n - 1], p.X0[s.n - 1])  # no observation: bit-equal to the start


@pytest.mark.parametrize('s', S.SHAPES, ids=IDS)
def test_sba_ext_shape_matches_oracle(ctx, s):
    """8 iterations, the one-view point included (the ulp probe moves it by 2e-14 m)."""
    _check_parity(s, _solve(ctx, s, max_iters=S.FIXED_ITERS), S.run(s, max_iters=S.FIXED_ITERS))


@pytest.mark.parametrize('max_iters', range(6))
@pytest.mark.parametrize('s', [S.SMALL, S.LARGE], ids=S.shape_id)
def test_sba_ext_stop_inside_the_replay(ctx, s, max_iters):
    """The LM loop replays a graph of four iterations and reads the status between replays: a stop
    at each of its positions and one past it; max_iters = 0 takes no step."""
    got = _solve(ctx, s, max_iters=max_iters)
    _check_parity(s, got, S.run(s, max_iters=max_iters))
    cams, X, rb, ra, rep = got
    assert rep['iters'] == max_iters and rep['status_name'] == 'maxiter'
    if max_iters == 0:
        p = S.problem(s)
        np.testing.assert_array_equal(X, p.X0)
        np.testing.assert_array_equal(cams, _cams(p))
        np.testing.assert_array_equal(ra, rb)
        assert rep['cost_after'] == rep['cost_before'] and rep['n_accepted'] == 0 and rep['lambda_final'] == 1e-3


@pytest.mark.parametrize('s,kind', CONV, ids=CONV_IDS)
def test_sba_ext_converges_as_the_oracle(ctx, s, kind):
    stop = S.STOPS[s, kind]
    opts = S.stop_opts(stop)
    ref = S.run(s, **opts)
    assert ref.info['status'] == kind and ref.info['iters'] == stop.iters
    one_view = np.nonzero(np.bincount(S.problem(s).pi, minlength=s.n) == 1)[0]
    assert list(one_view) == [s.n - 2]
    _check_parity(s, _solve(ctx, s, **opts), ref, skip_point=s.n - 2)


def test_sba_ext_is_deterministic(ctx):
    a, b = (_solve(ctx, S.LARGE, max_iters=S.FIXED_ITERS) for _ in range(2))
    for x, y in zip(a[:4], b[:4]):
        np.testing.assert_array_equal(x.view(np.uint64), y.view(np.uint64))
    for f in REPORT:
        assert np.array([a[4][f]]).tobytes() == np.array([b[4][f]]).tobytes(), f


def test_sba_ext_refuses_65_observations(ctx):
    """EXT_MAXK = 64 observations of a point is the limit. The refusal names the entry point and
    allocates nothing that an accepted problem of the same size does not."""
    s = S.LARGE
    p = S.problem(s)
    extra = np.nonzero(p.pi == 0)[0][:1]
    uv, ci = np.concatenate([p.uv, p.uv[extra]]), np.concatenate([p.ci, p.ci[extra]])
    ok = ctx.sba_extrinsics(_cams(p), uv, np.concatenate([p.pi, [s.n - 1]]).astype(np.int32), ci, p.X0,
                            ctx.sba_ext_opts(max_iters=1))
    assert ok[4]['iters'] == 1
    pi65 = np.concatenate([p.pi, [0]]).astype(np.int32)
    assert np.bincount(pi65).max() == S.EXT_MAXK + 1
    before = _native.alloc_events()
    with pytest.raises(RuntimeError, match=r'acs_sba_extrinsics: a point has 65 observations \(max 64\)'):
        ctx.sba_extrinsics(_cams(p), uv, pi65, ci, p.X0, ctx.sba_ext_opts(max_iters=1))
    assert _native.alloc_events() == before
    with pytest.raises(ValueError):
        _native.sba_ext_plan(s.n, S.EXT_MAXK + 1)
    _check_parity(s, _solve(ctx, s, max_iters=1), S.run(s, max_iters=1))  # and the context still solves


@pytest.mark.parametrize('world', [2, 3])
@pytest.mark.parametrize('s', S.DIST_SHAPES, ids=S.shape_id)
def test_sba_ext_dist_virtual_on_the_shapes(ctx, s, world):
    """The rank solve against the single-GPU one, at test_sba_ext_dist_virtual_matches_single's
    tolerances; three ranks get unequal shards of the 70 points."""
    p = S.problem(s)
    sizes = [hi - lo for lo, hi, _, _ in dist.split_points(p.pi, s.n, world)]
    assert sum(sizes) == s.n and (world != 3 or len(set(sizes)) > 1)
    c1, X1, _, _, r1 = _solve(ctx, s, max_iters=S.FIXED_ITERS)
    cd, Xd, rd = dist.sba_extrinsics_virtual(ctx, _cams(p), p.uv, p.pi, p.ci, p.X0,
                                             ctx.sba_ext_opts(max_iters=S.FIXED_ITERS), world=world)
    print(f'\n{S.shape_id(s)} world {world} shards {sizes} points {np.abs(Xd - X1).max():.1e} '
          f'rotations {np.abs(cd[:, 8:17] - c1[:, 8:17]).max():.1e} '
          f'translations {np.abs(cd[:, 17:] - c1[:, 17:]).max():.1e} '
          f'cost {abs(rd["cost_after"] / r1["cost_after"] - 1):.1e}')
    assert rd['iters'] == r1['iters'] and rd['n_accepted'] == r1['n_accepted'] and rd['status'] == r1['status']
    assert abs(rd['cost_after'] - r1['cost_after']) <= 1e-12 * r1['cost_after']
    np.testing.assert_allclose(Xd, X1, rtol=0, atol=1e-9)
    np.testing.assert_allclose(cd[:, 8:17], c1[:, 8:17], rtol=0, atol=1e-10)
    np.testing.assert_allclose(cd[:, 17:], c1[:, 17:], rtol=0, atol=1e-9)
    np.testing.assert_array_equal(Xd[s.n - 1], p.X0[s.n - 1])
