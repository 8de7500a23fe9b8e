"""Bitwise A/B of two builds of the extrinsics SBA, its covariance, the points-only covariance and the
rigid-board solves (boards, boards with free points, board covariance).

    ACINOSET_HIP_LIB=<library> python tools/sba_ext_bitcheck.py run TAG [DIR]      # one process per library
    python tools/sba_ext_bitcheck.py compare TAG_A TAG_B [DIR]                    # exit status 1 on a difference

`run` solves small seeded problems with the library named by ACINOSET_HIP_LIB and saves every output
as DIR/sba_ext_bits_TAG.npz (DIR: build/sba_ext_bits unless given); `compare` views every float
array as uint64 and asks for equal bits (integers for equal values), printing one line per problem and one per
array that differs. No oracle: the observations are the numpy projection of
synth.ring_scene plus noise, so a point may be seen more than once by a camera (the way past K = 16).

Extrinsics shapes (C cameras, largest K, n points -> lane group, Schur chunk): (2, 2, 70) -> 2, 64 and
a ragged 6; (3, 3, 70) -> 4; the sba_extrinsics golden (6, 6, 80) -> 8; (16, 16, 70) -> 16, 41;
(16, 20, 70) -> 32, 32; (16, 40, 70) -> 64, 16 with a ragged 6. Each synthetic one has a point without
observation and a point one camera sees. Per shape: acs_sba_extrinsics (8 iterations; cameras,
points, both residual vectors, report), acs_sba_extrinsics_covariance in both gauges, and on the
G = 8 and G = 64 shapes dist.sba_extrinsics_virtual with world 2. Points-only covariance, list and
dense form, at K = 1, 2, 3, 6, 12, 20, 40 and 100 (the strided slots of G = 64); both camera models
at K = 6 (the standard records see the fisheye measurements: large residuals, the same arithmetic).

Rigid boards (rigs of tests/sba_boards_ref.py and tests/sba_boards_points_ref.py, as the GPU tests build
them): the five shapes of tests/test_gpu_sba_boards.py, the ragged last Schur chunk at C = 3 and 16, and
c3_b5_nc12 with a further board without a view and with a single view. Per shape acs_sba_boards with
max_iters 0, 5 and 8 (cameras, board poses, both residual vectors, report) and
acs_sba_boards_covariance at the start state in the free gauge, anchored at camera 0 and at a nonzero
camera; a one-camera rig for the covariance. Per problem of sba_boards_points_ref.PROBLEMS
acs_sba_boards_points with 8 iterations, and once without its points. c3_b5_nc12 once more through the
three device-pointer bindings.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests'))  # the boards' rigs
import numpy as np  # noqa: E402

OUT = os.path.join('build', 'sba_ext_bits')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden', 'sba_extrinsics.npz')
EXT_SHAPES = [(2, 2, 70), (3, 3, 70), (16, 16, 70), (16, 20, 70), (16, 40, 70)]
COV_K = [1, 2, 3, 6, 12, 20, 40, 100]
# the rigid-board shapes (C, B, board shape, views per board) of tests/test_gpu_sba_boards.py and the
# nonzero anchor camera tests/test_gpu_sba_boards_cov.py takes on each (2 on the others)
BOARD_SHAPES = {'c2_b2_nc4': (2, 2, (2, 2), None), 'c3_b5_nc12': (3, 5, (4, 3), None),
                'c16_b40_nc54': (16, 40, (9, 6), (2, 16)), 'nc70': (3, 4, (10, 7), (2, 3)),
                'nc256': (2, 3, (16, 16), None)}
BOARD_ANCHOR = {'c2_b2_nc4': 1, 'c16_b40_nc54': 11, 'nc70': 1, 'nc256': 1, 'ragged16': 7}


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


def board_rigs():
    """{name: (rig, start)} of the board solve: tests/test_gpu_sba_boards.py's shapes, its two ragged
    last Schur chunks and, on c3_b5_nc12, a further board without a view and one with a single view."""
    import sba_boards_ref as ref
    from acinoset_amd import _native

    def make(C, B, shape, views):
        rig = ref.make_rig(C, B, shape=shape, seed=0, views=views, noise=0.5)
        return rig, ref.perturb(rig, 100)

    def extra_board(rig, start, n_views):  # a copy of board 0 seen by the first n_views cameras of board 0
        R0, t0, bR0, bt0 = start
        m = np.zeros((1, rig['mask'].shape[1]), np.uint8)
        m[0, np.nonzero(rig['mask'][0])[0][:n_views]] = 1
        r2 = dict(rig, mask=np.concatenate([rig['mask'], m]),
                  uv=np.concatenate([rig['uv'], rig['uv'][:1] * m[0][None, :, None, None]]))
        return r2, (R0, t0, np.concatenate([bR0, bR0[:1]]), np.concatenate([bt0, bt0[:1]]))

    rigs = {name: make(*shape) for name, shape in BOARD_SHAPES.items()}
    for C in (3, 16):
        rigs[f'ragged{C}'] = make(C, _native.sba_boards_chunk(C) + 1, (2, 2), (2, C))
    for n_views in (0, 1):
        rigs[f'c3_b5_nc12_extra{n_views}'] = extra_board(*rigs['c3_b5_nc12'], n_views)
    return rigs


def _dev_arrays(**arrays):
    import torch
    dev = torch.device('cuda', int(os.environ.get('ACINOSET_DEVICE', 0)))
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in arrays.items()}
    torch.cuda.synchronize(dev)
    return d


def run_boards(ctx, tag, out):
    """acs_sba_boards (0, 5 and 8 iterations), acs_sba_boards_covariance at the start state (free gauge,
    anchor 0 and a nonzero anchor; one camera too) and acs_sba_boards_points (8 iterations, and without
    its points); c3_b5_nc12 once more through the device-pointer bindings."""
    import sba_boards_points_ref as pref
    from acinoset_amd import _native
    rigs = board_rigs()
    for name, (rig, (R0, t0, bR0, bt0)) in rigs.items():
        cams = _native.pack_cameras(rig['K'], rig['D'], R0, t0)
        for it in (0, 5, 8):
            c, bR, bt, rb, ra, rep = ctx.sba_boards(cams, rig['obj'], rig['uv'], rig['mask'], bR0, bt0,
                                                    ctx.sba_ext_opts(max_iters=it))
            _put(out, f'boards_{name}/solve{it}', cams=c, board_r=bR, board_t=bt, resid_before=rb, resid_after=ra,
                 report=rep)
        anchors = [('free', 0), ('anchor', 0), ('anchor', BOARD_ANCHOR.get(name, 2))]
        for gauge, a in anchors:
            cc, cb, st, rep = ctx.sba_boards_covariance(cams, rig['obj'], rig['uv'], rig['mask'], bR0, bt0, gauge=gauge,
                                                        anchor=a)
            _put(out, f'boards_{name}/cov_{gauge}{a}', cov_cams=cc, cov_boards=cb, status=st, report=rep)
        if name == 'c3_b5_nc12':
            for gauge in ('free', 'anchor'):
                cc, cb, st, rep = ctx.sba_boards_covariance(cams[:1], rig['obj'], rig['uv'][:, :1], rig['mask'][:, :1],
                                                            bR0, bt0, gauge=gauge, anchor=0, sigma_px=0.5)
                _put(out, f'boards_one_camera/cov_{gauge}', cov_cams=cc, cov_boards=cb, status=st, report=rep)
            poses = np.concatenate([bR0.reshape(-1, 9), bt0], 1)
            n_res = 2 * len(rig['obj']) * int(rig['mask'].sum())
            d = _dev_arrays(cams=cams, obj=rig['obj'], uv=rig['uv'], mask=rig['mask'], poses=poses, rb=np.zeros(n_res),
                            ra=np.zeros(n_res), cc=np.zeros((18, 18)), cb=np.zeros((5, 6, 6)), st=np.zeros(5, np.int32))
            p = {k: v.data_ptr() for k, v in d.items()}
            rep = ctx.sba_boards_covariance_dev(p['cams'], 3, p['obj'], len(rig['obj']), p['uv'], p['mask'], 5, p['poses'],
                                                p['cc'], p['cb'], p['st'], gauge='anchor', anchor=2)
            ctx.sync()
            _put(out, f'boards_{name}/cov_dev', cov_cams=d['cc'].cpu().numpy(), cov_boards=d['cb'].cpu().numpy(),
                 status=d['st'].cpu().numpy(), report=rep)
            rep = ctx.sba_boards_dev(p['cams'], 3, p['obj'], len(rig['obj']), p['uv'], p['mask'], 5, p['poses'],
                                     ctx.sba_ext_opts(max_iters=8), p['rb'], p['ra'])
            ctx.sync()
            _put(out, f'boards_{name}/solve_dev', cams=d['cams'].cpu().numpy(), poses=d['poses'].cpu().numpy(),
                 resid_before=d['rb'].cpu().numpy(), resid_after=d['ra'].cpu().numpy(), report=rep)
        print(tag, 'boards', name, 'done', flush=True)
    for name in pref.PROBLEMS:
        rig, (R0, t0, bR0, bt0, X0) = pref.problem(name)
        cams = _native.pack_cameras(rig['K'], rig['D'], R0, t0)
        n, C = rig['pt_mask'].shape
        for label, k in (('points', n), ('no_points', 0)):
            c, bR, bt, X, rb, ra, rep = ctx.sba_boards_points(cams, rig['obj'], rig['uv'], rig['mask'], bR0, bt0,
                                                              rig['pt_uv'][:k], rig['pt_mask'][:k], X0[:k],
                                                              ctx.sba_ext_opts(max_iters=8))
            _put(out, f'boards_points_{name}/{label}', cams=c, board_r=bR, board_t=bt, pts=X, resid_before=rb,
                 resid_after=ra, report=rep)
        if name == 'c3_b5_nc12_n7':
            poses = np.concatenate([bR0.reshape(-1, 9), bt0], 1)
            n_res = 2 * (len(rig['obj']) * int(rig['mask'].sum()) + int(rig['pt_mask'].sum()))
            d = _dev_arrays(cams=cams, obj=rig['obj'], uv=rig['uv'], mask=rig['mask'], poses=poses, puv=rig['pt_uv'],
                            pmask=np.asarray(rig['pt_mask'] != 0, np.uint8), pts=X0, rb=np.zeros(n_res), ra=np.zeros(n_res))
            p = {k: v.data_ptr() for k, v in d.items()}
            rep = ctx.sba_boards_points_dev(p['cams'], C, p['obj'], len(rig['obj']), p['uv'], p['mask'], len(bR0),
                                            p['poses'], p['puv'], p['pmask'], n, p['pts'], ctx.sba_ext_opts(max_iters=8),
                                            p['rb'], p['ra'])
            ctx.sync()
            _put(out, f'boards_points_{name}/dev', cams=d['cams'].cpu().numpy(), poses=d['poses'].cpu().numpy(),
                 pts=d['pts'].cpu().numpy(), resid_before=d['rb'].cpu().numpy(), resid_after=d['ra'].cpu().numpy(),
                 report=rep)
        print(tag, 'boards + points', name, 'done', flush=True)


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
    run_boards(ctx, tag, out)
    os.makedirs(OUT, exist_ok=True)
    np.savez(os.path.join(OUT, f'sba_ext_bits_{tag}.npz'), **out)
    print(tag, 'library', _native.LIB_PATH, 'saved', len(out), 'arrays', flush=True)


def compare(ta, tb):
    a, b = (np.load(os.path.join(OUT, f'sba_ext_bits_{t}.npz')) for t in (ta, tb))
    bad = sorted(set(a.files) ^ set(b.files))
    for k in bad:
        print(k, 'MISSING on one side')
    count = {}  # per problem (the name up to the first '/'): arrays compared, arrays that differ
    for k in sorted(set(a.files) & set(b.files)):
        x, y = a[k], b[k]
        if x.dtype == np.float64:
            x, y = x.view(np.uint64), y.view(np.uint64)
        same = x.shape == y.shape and np.array_equal(x, y)
        n = count.setdefault(k.split('/')[0], [0, 0])
        n[0] += 1
        if not same:
            n[1] += 1
            bad.append(k)
            print(f'{k:44s} {str(a[k].dtype):8s} {str(a[k].shape):14s} DIFFER')
    for name, (n, d) in count.items():
        print(f'{name:36s} {n:4d} arrays', 'bit-identical' if not d else f'{d} DIFFER')
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
