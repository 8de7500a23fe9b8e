"""Bitwise A/B of two builds of the extrinsics SBA, its covariance and the points-only covariance.

    ACINOSET_HIP_LIB=<library> python tools/sba_ext_bitcheck.py run TAG [DIR]      # one process per library
    python tools/sba_ext_bitcheck.py compare TAG_A TAG_B [DIR]                    # exit status 1 on a difference

`run` solves small seeded problems with the library named by ACINOSET_HIP_LIB and saves every output
as DIR/sba_ext_bits_TAG.npz (DIR: build/sba_ext_bits unless given); `compare` views every float
array as uint64 and asks for equal bits (integers for equal values). No oracle: the observations are the numpy projection of
synth.ring_scene plus noise, so a point may be seen more than once by a camera (the way past K = 16).

Extrinsics shapes (C cameras, largest K, n points -> lane group, Schur chunk): (2, 2, 70) -> 2, 64 and
a ragged 6; (3, 3, 70) -> 4; the sba_extrinsics golden (6, 6, 80) -> 8; (16, 16, 70) -> 16, 41;
(16, 20, 70) -> 32, 32; (16, 40, 70) -> 64, 16 with a ragged 6. Each synthetic one has a point without
observation and a point one camera sees. Per shape: acs_sba_extrinsics (8 iterations; cameras,
points, both residual vectors, report), acs_sba_extrinsics_covariance in both gauges, and on the
G = 8 and G = 64 shapes dist.sba_extrinsics_virtual with world 2. Points-only covariance, list and
dense form, at K = 1, 2, 3, 6, 12, 20, 40 and 100 (the strided slots of G = 64); both camera models
at K = 6 (the standard records see the fisheye measurements: large residuals, the same arithmetic).
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np  # noqa: E402

OUT = os.path.join('build', 'sba_ext_bits')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden', 'sba_extrinsics.npz')
EXT_SHAPES = [(2, 2, 70), (3, 3, 70), (16, 16, 70), (16, 20, 70), (16, 40, 70)]
COV_K = [1, 2, 3, 6, 12, 20, 40, 100]


def _uv(sc, X, pi, ci, rng):
    from acinoset_amd import synth
    uv = np.empty((len(pi), 2))
    for c in range(len(sc.K)):
        m = ci == c
        uv[m] = synth.project_numpy(X[pi[m]], sc.K[c], sc.D[c], sc.R[c], sc.t[c])
    return uv + rng.normal(0, 0.5, uv.shape)


def ext_problem(C, K, n, seed):
    """Point 0 has K observations, point n - 2 one, point n - 1 none, the others 2..K; more than C
    observations of a point repeat cameras. Observations in shuffled order, a perturbed start."""
    from acinoset_amd import _native, synth
    rng = np.random.default_rng(seed)
    sc = synth.ring_scene(C)
    X = rng.uniform(-2, 2, (n, 3)) * [1, 1, 0.3] + [1.9, 6.4, 0.5]
    sizes = rng.integers(2, K + 1, n)
    sizes[0], sizes[n - 2], sizes[n - 1] = K, 1, 0
    pi = np.repeat(np.arange(n), sizes).astype(np.int32)
    ci = np.concatenate([np.concatenate([rng.permutation(C)[:min(s, C)], rng.integers(0, C, max(s - C, 0))])
                         for s in sizes]).astype(np.int32)
    order = rng.permutation(len(pi))
    pi, ci = pi[order], ci[order]
    uv = _uv(sc, X, pi, ci, rng)
    t0 = sc.t.reshape(-1, 3) + rng.normal(0, 5e-3, (C, 3)) * (np.arange(C) > 0)[:, None]
    return _native.pack_cameras(sc.K, sc.D, sc.R, t0), uv, pi, ci, X + rng.normal(0, 5e-3, X.shape)


def cov_problem(K, n, seed):
    """Dense (n, K) slots over K cameras: point 0 seen by all, point n - 2 by one, point n - 1 by none."""
    from acinoset_amd import synth
    rng = np.random.default_rng(seed)
    sc = synth.ring_scene(K)
    X = rng.uniform(-2, 2, (n, 3)) * [1, 1, 0.3] + [1.9, 6.4, 0.5]
    mask = rng.random((n, K)) < 0.8
    mask[0], mask[n - 2], mask[n - 1] = True, False, False
    mask[n - 2, 0] = True
    pi, ci = (a.astype(np.int32) for a in np.nonzero(mask))
    uv = np.zeros((n, K, 2))
    uv[pi, ci] = _uv(sc, X, pi, ci, rng)
    return sc, uv, mask.astype(np.uint8), pi, ci, X + rng.normal(0, 5e-3, X.shape)


def _put(out, name, **arrays):
    for k, v in arrays.items():
        if isinstance(v, dict):  # a report: numbers only (the names are derived from them)
            for f, x in v.items():
                if isinstance(x, (int, float)):
                    out[f'{name}/{k}.{f}'] = np.array([x], np.float64 if isinstance(x, float) else np.int64)
        elif v is not None:
            out[f'{name}/{k}'] = np.ascontiguousarray(v)


def run(tag):
    from acinoset_amd import _native, dist
    ctx = _native.Context(int(os.environ.get('ACINOSET_DEVICE', 0)))
    out = {}
    g = np.load(GOLDEN, allow_pickle=False)
    probs = [('golden_c6', (_native.pack_cameras(g['K'], g['D'], g['R0'], g['t0']), g['points_2d'],
                            g['point_indices'], g['camera_indices'], g['points_3d']))]
    probs += [(f'c{C}_k{K}', ext_problem(C, K, n, 100 + K)) for C, K, n in EXT_SHAPES]
    for name, (cams, uv, pi, ci, X0) in probs:
        opts = ctx.sba_ext_opts(max_iters=8)
        c, p, rb, ra, rep = ctx.sba_extrinsics(cams, uv, pi, ci, X0, opts)
        _put(out, name + '/solve', cams=c, pts=p, resid_before=rb, resid_after=ra, report=rep)
        if name in ('golden_c6', 'c16_k40'):
            c, p, rep = dist.sba_extrinsics_virtual(ctx, cams, uv, pi, ci, X0, ctx.sba_ext_opts(max_iters=8), world=2)
            _put(out, name + '/dist', cams=c, pts=p, report=rep)
        for gauge in ('free', 'anchor'):
            cc, cp, st, rep = ctx.sba_extrinsics_covariance(cams, uv, pi, ci, X0, gauge=gauge, anchor=(0, len(cams) // 2))
            _put(out, f'{name}/cov_{gauge}', cov_cams=cc, cov_points=cp, status=st, report=rep)
        print(tag, name, 'done', flush=True)
    for K in COV_K:
        sc, uv, mask, pi, ci, X = cov_problem(K, 70, 200 + K)
        models = [('fisheye', _native.pack_cameras(sc.K, sc.D, sc.R, sc.t))]
        if K == 6:
            models.append(('standard', _native.pack_cameras_standard(sc.K, np.zeros((K, 5)), sc.R, sc.t)))
        for model, cams in models:
            cov, st, rep = ctx.sba_points_covariance(cams, uv[pi, ci], pi, ci, X)
            _put(out, f'ptcov_k{K}_{model}/list', cov=cov, status=st, report=rep)
            cov, st, rep = ctx.sba_points_dense_covariance(cams, uv, mask, X)
            _put(out, f'ptcov_k{K}_{model}/dense', cov=cov, status=st, report=rep)
        print(tag, f'ptcov K={K}', 'done', flush=True)
    os.makedirs(OUT, exist_ok=True)
    np.savez(os.path.join(OUT, f'sba_ext_bits_{tag}.npz'), **out)
    print(tag, 'library', _native.LIB_PATH, 'saved', len(out), 'arrays', flush=True)


def compare(ta, tb):
    a, b = (np.load(os.path.join(OUT, f'sba_ext_bits_{t}.npz')) for t in (ta, tb))
    bad = sorted(set(a.files) ^ set(b.files))
    for k in bad:
        print(k, 'MISSING on one side')
    for k in sorted(set(a.files) & set(b.files)):
        x, y = a[k], b[k]
        if x.dtype == np.float64:
            x, y = x.view(np.uint64), y.view(np.uint64)
        same = x.shape == y.shape and np.array_equal(x, y)
        if not same:
            bad.append(k)
        print(f'{k:44s} {str(a[k].dtype):8s} {str(a[k].shape):14s}', 'bit-identical' if same else 'DIFFER')
    print(f'{ta} vs {tb}: {len(a.files)} arrays,', 'ALL bit-identical' if not bad else f'{len(bad)} DIFFER: {bad}')
    return 1 if bad else 0


if __name__ == '__main__':
    args = sys.argv[1:]
    n_fixed = {'run': 2, 'compare': 3}.get(args[0] if args else None)
    if n_fixed and len(args) == n_fixed + 1:
        OUT = args.pop()
    if n_fixed == 2 and len(args) == 2:
        run(args[1])
    elif n_fixed == 3 and len(args) == 3:
        sys.exit(compare(args[1], args[2]))
    else:
        sys.exit(__doc__)
