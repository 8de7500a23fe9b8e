"""ctypes binding of libacinoset_hip.so (the C ABI in include/acinoset_hip.h).

There is no CPU fallback: if the shared library is missing, or no gfx950 device is
visible, every call raises `NativeUnavailable` loudly.

`torch` is imported (if installed) BEFORE the library is loaded, so that the process
has a single HIP runtime: torch bundles its own libamdhip64.so.7 and the library's
NEEDED entry then binds to that already-loaded copy.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Optional

import numpy as np

try:  # one HIP runtime per process (see module docstring)
    import torch  # noqa: F401
except Exception:  # pragma: no cover - torch is optional for the product
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('ACINOSET_HIP_LIB', os.path.join(_HERE, 'libacinoset_hip.so'))

ACS_DEVICE_PTRS = 1
ACS_CAMS_STANDARD = 2      # flags bit: `cams` holds standard-model records
ACS_CAM_STRIDE = 20
ACS_CAM_STRIDE_STD = 24    # [fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 R(9) t(3)]
CAMERA_MODELS = {'fisheye': ACS_CAM_STRIDE, 'standard': ACS_CAM_STRIDE_STD}
STATUS_NAMES = ('running', 'gtol', 'ftol', 'xtol', 'stalled', 'maxiter', 'noobs')
ACS_COV_OK, ACS_COV_NOOBS, ACS_COV_DEGENERATE = 0, 1, 2   # per-point status of the SBA covariance
SD_MODES = {'const': 0, 'variable': 1}        # src/core/fte.py:35 shutter_delay_mode

SBA_LM_LAYOUTS = {'auto': 0, 'butterfly': 1, 'row': 2}   # ACS_SBA_LM_* of the header

# exported symbols (checked by tests against include/acinoset_hip.h)
SYMBOLS = (
    'acs_ctx_create', 'acs_ctx_destroy', 'acs_last_error', 'acs_ctx_set_stream', 'acs_ctx_sync',
    'acs_abi_version', 'acs_device_count', 'acs_sba_default_opts', 'acs_project_fisheye',
    'acs_sba_residuals', 'acs_sba_points', 'acs_sba_points_dense', 'acs_redescending_loss', 'acs_fk',
    'acs_fte_default_opts', 'acs_fte_solve', 'acs_fte_eval', 'acs_triangulate_pairs', 'acs_triangulate_dense',
    'acs_sba_ext_default_opts', 'acs_sba_extrinsics', 'acs_sba_points_dense_io',
    'acs_fte_dist_create', 'acs_fte_dist_init', 'acs_fte_dist_round', 'acs_fte_dist_poll',
    'acs_fte_dist_gather', 'acs_fte_dist_scatter', 'acs_fte_dist_result',
    'acs_fte_dist_destroy', 'acs_fte_dist_reset', 'acs_alloc_events', 'acs_ekf_singular_count',
    'acs_fte_debug_blocks', 'acs_fte_debug_plan', 'acs_ekf_debug_plan',
    'acs_sba_ext_dist_create', 'acs_sba_ext_dist_init', 'acs_sba_ext_dist_round', 'acs_sba_ext_dist_poll',
    'acs_sba_ext_dist_result', 'acs_sba_ext_dist_destroy', 'acs_ekf_run',
    'acs_sba_ekf_pipeline', 'acs_fte_covariance', 'acs_sba_set_lm_layout', 'acs_sba_lm_layout',
    'acs_project_standard', 'acs_sba_lm_layout_flags',
    'acs_sba_points_covariance', 'acs_sba_points_dense_covariance',
    'acs_sba_ext_cov_default_opts', 'acs_sba_extrinsics_covariance',
    'acs_sba_boards', 'acs_sba_boards_chunk', 'acs_sba_boards_covariance', 'acs_sba_ext_plan',
    'acs_sba_boards_points',
)


class NativeUnavailable(RuntimeError):
    pass


class SbaOpts(C.Structure):
    _fields_ = [('max_iters', C.c_int32), ('reserved', C.c_int32), ('f_scale', C.c_double),
                ('ftol', C.c_double), ('xtol', C.c_double), ('gtol', C.c_double)]


class Report(C.Structure):
    _fields_ = [('n_problems', C.c_int64), ('status_counts', C.c_int64 * 7), ('iters_max', C.c_int64),
                ('iters_sum', C.c_int64), ('nfev_sum', C.c_int64), ('cost_before', C.c_double),
                ('cost_after', C.c_double)]

    def as_dict(self):
        return dict(n_problems=self.n_problems,
                    status_counts={STATUS_NAMES[i]: int(self.status_counts[i]) for i in range(7)},
                    iters_max=self.iters_max, iters_sum=self.iters_sum, nfev_sum=self.nfev_sum,
                    cost_before=self.cost_before, cost_after=self.cost_after)


class EkfInitSpec(C.Structure):
    """acs_ekf_init_spec: what the EKF's initial state is fitted on (src/core/ekf.py:121-157)."""
    _fields_ = [(k, C.c_int32) for k in ('nose', 'lure', 'x0', 'y0', 'psi0', 'xl', 'yl', 'from_sba')]


def ekf_numerics_mode(ref_numerics, jacobian):
    """The C ABI's EKF measurement-model mode: 1 = the reference's float32 numerics with the
    forward-difference H, 0 = the same H in float64, ACS_EKF_ANALYTIC_H (2) = the analytic H
    (float64 only)."""
    if jacobian == 'analytic':
        if ref_numerics:
            raise ValueError("jacobian='analytic' runs in float64: pass ref_numerics=False")
        return 2
    if jacobian != 'fd':
        raise ValueError(f"jacobian must be 'fd' or 'analytic', not {jacobian!r}")
    return int(bool(ref_numerics))


def ekf_init_spec(table, obs_markers, from_sba=False):
    """The pipeline's init descriptor for EKF skeleton `table` on observations whose marker
    order is `obs_markers`."""
    obs = list(obs_markers)
    pidx = {p: i for i, p in enumerate(table.params)}
    lure = obs.index('lure') if ('lure' in table.markers and 'lure' in obs) else -1
    return EkfInitSpec(obs.index('nose'), lure, pidx['x_0'], pidx['y_0'], pidx['psi_0'], pidx.get('x_l', -1),
                       pidx.get('y_l', -1), int(bool(from_sba)))


class FteOpts(C.Structure):
    _fields_ = [('max_iters', C.c_int32), ('window', C.c_int32), ('ftol', C.c_double), ('xtol', C.c_double),
                ('gtol', C.c_double), ('lambda0', C.c_double), ('redesc_a', C.c_double),
                ('redesc_b', C.c_double), ('redesc_c', C.c_double)]


class FteReport(C.Structure):
    _fields_ = [('status', C.c_int32), ('iters', C.c_int32), ('n_accepted', C.c_int32), ('n_bad_pivots', C.c_int32),
                ('cost_before', C.c_double), ('cost_after', C.c_double), ('cost_meas', C.c_double),
                ('cost_model', C.c_double), ('grad_max', C.c_double), ('lambda_final', C.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d['status_name'] = STATUS_NAMES[self.status] if 0 <= self.status < 7 else str(self.status)
        return d


class FteCovReport(C.Structure):
    _fields_ = [('n_bad_pivots', C.c_int32), ('n_tau_free', C.c_int32), ('var_min', C.c_double),
                ('var_max', C.c_double)]


class SbaCovReport(C.Structure):
    _fields_ = [('n_points', C.c_int64), ('n_ok', C.c_int64), ('n_noobs', C.c_int64), ('n_degenerate', C.c_int64),
                ('var_min', C.c_double), ('var_max', C.c_double), ('sigma_hat_px', C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SbaExtOpts(C.Structure):
    _fields_ = [('max_iters', C.c_int32), ('reserved', C.c_int32), ('f_scale', C.c_double), ('ftol', C.c_double),
                ('xtol', C.c_double), ('gtol', C.c_double), ('lambda0', C.c_double)]


class SbaExtReport(C.Structure):
    _fields_ = [('status', C.c_int32), ('iters', C.c_int32), ('n_accepted', C.c_int32), ('n_bad_pivots', C.c_int32),
                ('cost_before', C.c_double), ('cost_after', C.c_double), ('grad_max', C.c_double),
                ('lambda_final', C.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d['status_name'] = STATUS_NAMES[self.status] if 0 <= self.status < 7 else str(self.status)
        return d


GAUGES = {'free': 0, 'anchor': 1}   # ACS_GAUGE_* of the header


class SbaExtCovOpts(C.Structure):
    _fields_ = [('gauge', C.c_int32), ('anchor_cam', C.c_int32), ('scale_cam', C.c_int32), ('reserved', C.c_int32),
                ('f_scale', C.c_double), ('sigma_px', C.c_double)]


class SbaExtCovReport(C.Structure):
    _fields_ = [('status', C.c_int32), ('reserved', C.c_int32), ('n_points', C.c_int64), ('n_ok', C.c_int64),
                ('n_noobs', C.c_int64), ('n_degenerate', C.c_int64), ('dof', C.c_int64), ('min_pivot', C.c_double),
                ('sigma_hat_px', C.c_double), ('rot_sd_max', C.c_double), ('trans_sd_max', C.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != 'reserved'}
        d['status_name'] = 'degenerate' if self.status else 'ok'
        return d


class SbaBoardsCovReport(C.Structure):
    _fields_ = [('status', C.c_int32), ('reserved', C.c_int32), ('n_boards', C.c_int64), ('n_ok', C.c_int64),
                ('n_noobs', C.c_int64), ('n_degenerate', C.c_int64), ('dof', C.c_int64), ('min_pivot', C.c_double),
                ('sigma_hat_px', C.c_double), ('rot_sd_max', C.c_double), ('trans_sd_max', C.c_double),
                ('board_rot_sd_max', C.c_double), ('board_trans_sd_max', C.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != 'reserved'}
        d['status_name'] = 'degenerate' if self.status else 'ok'
        return d


# must equal ACS_ABI_VERSION in include/acinoset_hip.h (checked when the library loads)
ABI_VERSION = 5
_lib = None
_lock = threading.Lock()
_P = C.c_void_p
_D = C.POINTER(C.c_double)


def _declare(lib):
    i32, i64, u32, dbl = C.c_int32, C.c_int64, C.c_uint32, C.c_double
    sig = {
        'acs_ctx_create': (C.c_int, [C.c_int, C.POINTER(_P)]),
        'acs_ctx_destroy': (C.c_int, [_P]),
        'acs_last_error': (C.c_char_p, [_P]),
        'acs_ctx_set_stream': (C.c_int, [_P, _P]),
        'acs_ctx_sync': (C.c_int, [_P]),
        'acs_abi_version': (C.c_int, []),
        'acs_device_count': (C.c_int, [C.POINTER(C.c_int)]),
        'acs_sba_default_opts': (None, [C.POINTER(SbaOpts)]),
        'acs_project_fisheye': (C.c_int, [_P, _P, i32, _P, _P, i64, i32, _P, u32]),
        'acs_project_standard': (C.c_int, [_P, _P, i32, _P, _P, i64, _P, u32]),
        'acs_sba_residuals': (C.c_int, [_P, _P, i32, _P, _P, _P, i64, _P, i64, _P, u32]),
        'acs_sba_points': (C.c_int, [_P, _P, i32, _P, _P, _P, i64, _P, i64, C.POINTER(SbaOpts), _P, _P,
                                     C.POINTER(Report), u32]),
        'acs_sba_points_dense': (C.c_int, [_P, _P, i32, _P, _P, i64, _P, C.POINTER(SbaOpts), C.POINTER(Report),
                                           u32]),
        'acs_sba_points_dense_io': (C.c_int, [_P, _P, i32, _P, _P, i64, _P, _P, C.POINTER(SbaOpts),
                                              C.POINTER(Report), u32]),
        'acs_sba_points_covariance': (C.c_int, [_P, _P, i32, _P, _P, _P, i64, _P, i64, dbl, dbl, _P, _P,
                                                C.POINTER(SbaCovReport), u32]),
        'acs_sba_points_dense_covariance': (C.c_int, [_P, _P, i32, _P, _P, i64, _P, dbl, dbl, _P, _P,
                                                      C.POINTER(SbaCovReport), u32]),
        'acs_sba_ext_cov_default_opts': (None, [C.POINTER(SbaExtCovOpts)]),
        'acs_sba_extrinsics_covariance': (C.c_int, [_P, _P, i32, _P, _P, _P, i64, _P, i64, C.POINTER(SbaExtCovOpts),
                                                    _P, _P, _P, C.POINTER(SbaExtCovReport), u32]),
        'acs_sba_set_lm_layout': (C.c_int, [_P, i32]),
        'acs_sba_lm_layout': (C.c_int, [_P, i32, i64, i32, C.POINTER(i32)]),
        'acs_sba_lm_layout_flags': (C.c_int, [_P, i32, i64, i32, C.POINTER(i32), u32]),
        'acs_redescending_loss': (C.c_int, [_P, _P, i64, dbl, dbl, dbl, _P, _P, u32]),
        'acs_fk': (C.c_int, [_P, _P, i64, _P, i64, _P, _P, _P, _P, i64, i32, i32, _P, _P, u32]),
        'acs_fte_default_opts': (None, [C.POINTER(FteOpts)]),
        'acs_fte_solve': (C.c_int, [_P, _P, i64, _P, i64, _P, i32, _P, _P, i32, i32, dbl, _P, i32, i32, _P, _P,
                                    C.POINTER(FteOpts), C.POINTER(FteReport), u32]),
        'acs_fte_eval': (C.c_int, [_P, _P, i64, _P, i64, _P, i32, _P, _P, i32, i32, dbl, _P, i32, i32, _P, _P,
                                   _P, _P, _P, u32]),
        'acs_fte_covariance': (C.c_int, [_P, _P, i64, _P, i64, _P, i32, _P, _P, i32, i32, dbl, _P, i32, i32, _P, _P,
                                         _P, _P, _P, C.POINTER(FteCovReport), u32]),
        'acs_fte_debug_blocks': (C.c_int, [_P, _P, i64, _P, i64, _P, i32, _P, _P, i32, i32, dbl, _P, i32, i32, _P, _P,
                                           dbl, i32, _P, C.POINTER(i64), u32]),
        'acs_fte_debug_plan': (C.c_int, [_P, i32, i32, i32, i32, i32, i32, C.POINTER(i32), C.POINTER(i32), i32]),
        'acs_ekf_debug_plan': (C.c_int, [i32, i32, i32, i32, i32, i32, i32, C.POINTER(i32)]),
        'acs_triangulate_pairs': (C.c_int, [_P, _P, i32, _P, _P, _P, _P, i64, _P, u32]),
        'acs_triangulate_dense': (C.c_int, [_P, _P, i32, _P, _P, i64, _P, _P, u32]),
        'acs_sba_ext_default_opts': (None, [C.POINTER(SbaExtOpts)]),
        'acs_fte_dist_create': (C.c_int, [_P, _P, i64, _P, i64, _P, i32, _P, _P, i32, i32, dbl, _P, i32, i32, _P, _P,
                                          C.POINTER(FteOpts), i32, i32, C.POINTER(_P), C.POINTER(i64), u32]),
        'acs_fte_dist_init': (C.c_int, [_P, _P]),
        'acs_fte_dist_round': (C.c_int, [_P, _P, _P]),
        'acs_fte_dist_poll': (C.c_int, [_P, i64, C.POINTER(i32)]),
        'acs_fte_dist_gather': (C.c_int, [_P, _P]),
        'acs_fte_dist_scatter': (C.c_int, [_P, _P]),
        'acs_fte_dist_result': (C.c_int, [_P, _P, _P, C.POINTER(FteReport), u32]),
        'acs_fte_dist_destroy': (C.c_int, [_P]),
        'acs_fte_dist_reset': (C.c_int, [_P, _P, _P, u32]),
        'acs_alloc_events': (C.c_int64, []),
        'acs_ekf_singular_count': (C.c_int, [_P, C.POINTER(i32)]),
        'acs_sba_ext_dist_create': (C.c_int, [_P, _P, i32, _P, _P, _P, i64, _P, i64, C.POINTER(SbaExtOpts), i32, i32,
                                              C.POINTER(_P), C.POINTER(i64), u32]),
        'acs_sba_ext_dist_init': (C.c_int, [_P, _P]),
        'acs_sba_ext_dist_round': (C.c_int, [_P, _P, _P]),
        'acs_sba_ext_dist_poll': (C.c_int, [_P, C.c_int64, C.POINTER(i32)]),
        'acs_sba_ext_dist_result': (C.c_int, [_P, _P, _P, C.POINTER(SbaExtReport), u32]),
        'acs_sba_ext_dist_destroy': (C.c_int, [_P]),
        'acs_ekf_run': (C.c_int, [_P, _P, i64, _P, i64, _P, i32, _P, _P, i32, i32, dbl, dbl, dbl, _P, _P, _P, _P, i32,
                                  dbl, _P, _P, _P, _P, _P, _P, u32]),
        'acs_sba_ekf_pipeline': (C.c_int, [_P, _P, i64, _P, i64, _P, i32, _P, _P, i32, i32, i32, _P, dbl, dbl, dbl,
                                           _P, _P, _P, C.POINTER(SbaOpts), C.POINTER(EkfInitSpec), i32, dbl, _P, _P,
                                           _P, _P, C.POINTER(Report), u32]),
        'acs_sba_extrinsics': (C.c_int, [_P, _P, i32, _P, _P, _P, i64, _P, i64, C.POINTER(SbaExtOpts), _P, _P,
                                         C.POINTER(SbaExtReport), u32]),
        'acs_sba_boards': (C.c_int, [_P, _P, i32, _P, i32, _P, _P, i32, _P, C.POINTER(SbaExtOpts), _P, _P,
                                     C.POINTER(SbaExtReport), u32]),
        'acs_sba_boards_points': (C.c_int, [_P, _P, i32, _P, i32, _P, _P, i32, _P, _P, _P, i32, _P,
                                            C.POINTER(SbaExtOpts), _P, _P, C.POINTER(SbaExtReport), u32]),
        'acs_sba_boards_chunk': (i32, [i32]),
        'acs_sba_ext_plan': (C.c_int, [i64, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        'acs_sba_boards_covariance': (C.c_int, [_P, _P, i32, _P, i32, _P, _P, i32, _P, C.POINTER(SbaExtCovOpts), _P, _P,
                                                _P, C.POINTER(SbaBoardsCovReport), u32]),
    }
    for name, (res, args) in sig.items():
        if not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args


def fte_debug_plan(n_frames, P, n_cams, shutter_delay=True, sd_mode='const', n_cu=None, ctx=None):
    """acs_fte_debug_plan (test hook, no GPU needed with n_cu): the kernels and grids acs_fte_solve
    picks for this problem size on a device of n_cu CUs (None: the device of `ctx`). Returns a dict:
    nblk, nlev, BP, GR, Cg, asm (512 / 1024 threads of k_cr_assemble_build, 0: k_cr_build), lin
    (k_fte_linearize instance), d_upper, and levels = [(ne, ns, nsplit, deep)] per reduction level."""
    if n_cu is None and ctx is None:
        raise ValueError('fte_debug_plan: give n_cu or ctx')
    lib = load_library()
    head = (C.c_int32 * 8)()
    lv = (C.c_int32 * (4 * 32))()
    rc = lib.acs_fte_debug_plan(ctx.h if n_cu is None else None, 0 if n_cu is None else int(n_cu), int(n_frames),
                                int(P), int(n_cams), int(bool(shutter_delay)), int(SD_MODES.get(sd_mode, sd_mode)),
                                head, lv, 32)
    if rc != 0:
        raise ValueError(f'acs_fte_debug_plan: bad arguments (rc {rc})')
    keys = ('nblk', 'nlev', 'BP', 'GR', 'Cg', 'asm', 'lin', 'd_upper')
    plan = {k: int(head[i]) for i, k in enumerate(keys)}
    plan['levels'] = [(int(lv[4 * l]), int(lv[4 * l + 1]), int(lv[4 * l + 2]), bool(lv[4 * l + 3]))
                      for l in range(plan['nlev'])]
    return plan


EKF_FILTERS = ('k_ekf_filter', 'k_ekf_filter_w1')
EKF_GAINS = ('none', 'k_ekf_gain_w', 'k_ekf_gain', 'k_ekf_gain_t<3>', 'k_ekf_gain_t<4>', 'k_ekf_gain_t<5>',
             'k_ekf_gain_t<6>')
EKF_SMOOTHERS = ('k_ekf_smooth', 'k_ekf_smooth_xs<18,8>', 'k_ekf_smooth_xs<87,2>', 'k_ekf_smooth_x')


def ekf_debug_plan(P, n_cams, L, n_frames, covariances=False, n_joints=None, n_nodes=None):
    """acs_ekf_debug_plan (test hook, no GPU): the kernels acs_ekf_run picks for a table of P
    parameters, L markers, n_joints joints and n_nodes nodes (P may be a SkeletonTable, which
    gives all four; the counts default to one joint and L nodes, the smallest table), n_cams
    cameras and n_frames frames, with (covariances) or without P_smooth. Returns a dict: filter,
    gains, smoother (kernel names, EKF_FILTERS / EKF_GAINS / EKF_SMOOTHERS), waves, npad, lds."""
    if hasattr(P, 'ints'):
        P, L, n_joints, n_nodes = P.P, P.L, P.n_joints, P.n_nodes
    n_joints = 1 if n_joints is None else n_joints
    n_nodes = L if n_nodes is None else n_nodes
    plan = (C.c_int32 * 6)()
    rc = load_library().acs_ekf_debug_plan(int(P), int(n_joints), int(n_nodes), int(n_cams), int(L), int(n_frames),
                                           int(bool(covariances)), plan)
    if rc != 0:
        raise ValueError(f'acs_ekf_debug_plan: shape refused (rc {rc})')
    return dict(filter=EKF_FILTERS[plan[0]], waves=int(plan[1]), gains=EKF_GAINS[plan[2]],
                smoother=EKF_SMOOTHERS[plan[3]], npad=int(plan[4]), lds=int(plan[5]))


def alloc_events():
    """acs_alloc_events: device / pinned-host allocations + frees the library has made in this
    process (no GPU needed)."""
    return int(load_library().acs_alloc_events())


def sba_boards_chunk(n_cams):
    """acs_sba_boards_chunk: boards per Schur block of acs_sba_boards for n_cams cameras (no GPU
    needed)."""
    return int(load_library().acs_sba_boards_chunk(int(n_cams)))


def sba_ext_plan(n_pts, K):
    """acs_sba_ext_plan (test hook, no GPU needed): what acs_sba_extrinsics selects for n_pts points
    whose largest observation count is K. Returns a dict: G (lanes per point), chunk (points per
    Schur block), nchunk (Schur blocks)."""
    g, chunk, nchunk = C.c_int32(), C.c_int32(), C.c_int32()
    rc = load_library().acs_sba_ext_plan(int(n_pts), int(K), C.byref(g), C.byref(chunk), C.byref(nchunk))
    if rc != 0:
        raise ValueError(f'acs_sba_ext_plan: shape refused (rc {rc})')
    return dict(G=g.value, chunk=chunk.value, nchunk=nchunk.value)


def load_library():
    """Load libacinoset_hip.so (no GPU needed). Raises NativeUnavailable if missing."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise NativeUnavailable(
                    f'{LIB_PATH} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                    '(hipcc --offload-arch=gfx950). There is no CPU fallback.')
            lib = C.CDLL(LIB_PATH)
            _declare(lib)
            got = lib.acs_abi_version()
            if got != ABI_VERSION:
                raise NativeUnavailable(f'{LIB_PATH} has C ABI version {got}, this package needs {ABI_VERSION} '
                                        '(include/acinoset_hip.h ACS_ABI_VERSION): rebuild the library')
            _lib = lib
    return _lib


def _ptr(a: Optional[np.ndarray]):
    if a is None:
        return None
    return C.c_void_p(a.ctypes.data)


def _c64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def pack_cameras(K, D, R, t) -> np.ndarray:
    """(C,3,3),(C,4[,1]),(C,3,3),(C,3[,1]) -> (C, 20) camera records (header: camera block)."""
    K = np.asarray(K, np.float64).reshape(-1, 3, 3)
    n = len(K)
    D = np.asarray(D, np.float64).reshape(n, 4)
    R = np.asarray(R, np.float64).reshape(n, 3, 3)
    t = np.asarray(t, np.float64).reshape(n, 3)
    cams = np.empty((n, ACS_CAM_STRIDE))
    cams[:, 0] = K[:, 0, 0]
    cams[:, 1] = K[:, 1, 1]
    cams[:, 2] = K[:, 0, 2]
    cams[:, 3] = K[:, 1, 2]
    cams[:, 4:8] = D
    cams[:, 8:17] = R.reshape(n, 9)
    cams[:, 17:20] = t
    return cams


def pack_cameras_standard(K, D, R, t) -> np.ndarray:
    """(C,3,3), D, (C,3,3), (C,3[,1]) -> (C, 24) standard-model camera records (header:
    ACS_CAMS_STANDARD). D holds OpenCV's (k1, k2, p1, p2[, k3[, k4, k5, k6]]) per camera: 4, 5
    or 8 coefficients as (C, n), (C, n, 1) or (C, 1, n), zero-padded to 8. The 12- and
    14-coefficient forms are taken only if their extra (thin-prism, tilt) terms are zero."""
    K = np.asarray(K, np.float64).reshape(-1, 3, 3)
    n = len(K)
    D = np.asarray(D, np.float64).reshape(n, -1)
    nd = D.shape[1]
    if nd in (12, 14):
        if np.any(D[:, 8:] != 0.0):
            raise ValueError('pack_cameras_standard: the thin-prism (s1..s4) and tilt (tau_x, tau_y) coefficients '
                             'of the 12- / 14-coefficient model are not supported (they must be zero)')
        D, nd = D[:, :8], 8
    if nd not in (4, 5, 8):
        raise ValueError(f'pack_cameras_standard: {nd} distortion coefficients per camera (4, 5 or 8 expected)')
    R = np.asarray(R, np.float64).reshape(n, 3, 3)
    t = np.asarray(t, np.float64).reshape(n, 3)
    cams = np.zeros((n, ACS_CAM_STRIDE_STD))
    cams[:, 0] = K[:, 0, 0]
    cams[:, 1] = K[:, 1, 1]
    cams[:, 2] = K[:, 0, 2]
    cams[:, 3] = K[:, 1, 2]
    cams[:, 4:4 + nd] = D
    cams[:, 12:21] = R.reshape(n, 9)
    cams[:, 21:24] = t
    return cams


def _cams_flags(cams):
    """Camera records as a contiguous (C, 20 | 24) float64 array and the flags bit of their
    model, taken from the record width."""
    cams = np.ascontiguousarray(cams, dtype=np.float64)
    if cams.ndim != 2 or cams.shape[1] not in (ACS_CAM_STRIDE, ACS_CAM_STRIDE_STD):
        raise ValueError(f'camera records of shape {cams.shape}: (C, {ACS_CAM_STRIDE}) fisheye (pack_cameras) or '
                         f'(C, {ACS_CAM_STRIDE_STD}) standard (pack_cameras_standard) expected')
    return cams, (ACS_CAMS_STANDARD if cams.shape[1] == ACS_CAM_STRIDE_STD else 0)


def _std_flag(cams):
    """ACS_CAMS_STANDARD for (C, 24) records, else 0: passed on by the bindings of the fisheye-only
    entry points, so that the library refuses standard records by name instead of reading them
    with the wrong stride."""
    return ACS_CAMS_STANDARD if np.ndim(cams) == 2 and np.shape(cams)[1] == ACS_CAM_STRIDE_STD else 0


def _model_flags(camera_model):
    if camera_model not in CAMERA_MODELS:
        raise ValueError(f"camera_model must be 'fisheye' or 'standard', not {camera_model!r}")
    return ACS_CAMS_STANDARD if camera_model == 'standard' else 0


class Context:
    """One HIP device + stream (acs_ctx). Methods take numpy arrays (host pointers)
    unless `device_ptrs=True`, in which case they take raw device addresses (ints)."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        h = _P()
        rc = self.lib.acs_ctx_create(int(device), C.byref(h))
        if rc != 0:
            n = C.c_int(0)
            self.lib.acs_device_count(C.byref(n))
            raise NativeUnavailable(f'acs_ctx_create(device={device}) failed with {rc}: {n.value} HIP device(s) '
                                    'visible; a gfx950 (MI355X) device is required and there is no CPU fallback.')
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, 'h', None):
            self.lib.acs_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc, what):
        if rc != 0:
            msg = self.lib.acs_last_error(self.h)
            raise RuntimeError(f'{what} failed ({rc}): {msg.decode() if msg else ""}')

    def set_stream(self, stream_handle: int):
        self.check(self.lib.acs_ctx_set_stream(self.h, C.c_void_p(stream_handle or 0)), 'acs_ctx_set_stream')

    def sync(self):
        self.check(self.lib.acs_ctx_sync(self.h), 'acs_ctx_sync')

    # ---- a1 -------------------------------------------------------------------------
    def project(self, cams, pts, cam_idx=None, fte_form=False):
        """Projection through (C, 20) fisheye or (C, 24) standard records (the width selects)."""
        cams, mf = _cams_flags(cams)
        pts = _c64(pts).reshape(-1, 3)
        n = len(pts)
        ci = None if cam_idx is None else np.ascontiguousarray(np.broadcast_to(cam_idx, (n,)), np.int32)
        out = np.empty((n, 2))
        if mf:
            if fte_form:
                raise ValueError('project: fte_form is the FTE restatement of the fisheye model; standard records '
                                 'have none')
            self.check(self.lib.acs_project_standard(self.h, _ptr(cams), len(cams), _ptr(pts), _ptr(ci), n, _ptr(out),
                                                     mf), 'acs_project_standard')
            return out
        self.check(self.lib.acs_project_fisheye(self.h, _ptr(cams), len(cams), _ptr(pts), _ptr(ci), n,
                                                int(bool(fte_form)), _ptr(out), 0), 'acs_project_fisheye')
        return out

    # ---- a2 -------------------------------------------------------------------------
    def sba_residuals(self, cams, uv, pt_idx, cam_idx, pts):
        cams, mf = _cams_flags(cams)
        uv = _c64(uv).reshape(-1, 2)
        pi = np.ascontiguousarray(pt_idx, np.int32)
        ci = np.ascontiguousarray(cam_idx, np.int32)
        pts = _c64(pts).reshape(-1, 3)
        out = np.empty(2 * len(uv))
        self.check(self.lib.acs_sba_residuals(self.h, _ptr(cams), len(cams), _ptr(uv), _ptr(pi), _ptr(ci), len(uv),
                                              _ptr(pts), len(pts), _ptr(out), mf), 'acs_sba_residuals')
        return out

    # ---- a4 -------------------------------------------------------------------------
    @staticmethod
    def sba_opts(f_scale=50.0, max_iters=100, ftol=1e-15, xtol=1e-9, gtol=1e-10):
        return SbaOpts(int(max_iters), 0, float(f_scale), float(ftol), float(xtol), float(gtol))

    def sba_points(self, cams, uv, pt_idx, cam_idx, pts0, opts=None, residuals=True):
        cams, mf = _cams_flags(cams)
        uv = _c64(uv).reshape(-1, 2)
        pi = np.ascontiguousarray(pt_idx, np.int32)
        ci = np.ascontiguousarray(cam_idx, np.int32)
        pts = _c64(pts0).reshape(-1, 3).copy()
        rb = np.empty(2 * len(uv)) if residuals else None
        ra = np.empty(2 * len(uv)) if residuals else None
        rep = Report()
        opts = opts or self.sba_opts()
        self.check(self.lib.acs_sba_points(self.h, _ptr(cams), len(cams), _ptr(uv), _ptr(pi), _ptr(ci), len(uv),
                                           _ptr(pts), len(pts), C.byref(opts), _ptr(rb), _ptr(ra), C.byref(rep), mf),
                   'acs_sba_points')
        return pts, rb, ra, rep.as_dict()

    def sba_set_lm_layout(self, layout='auto'):
        """acs_sba_set_lm_layout (test hook): which LM kernel instance the points-only solves of this
        context launch where both are legal (3..8 slots, no camera ids): 'auto', 'butterfly' or 'row'."""
        self.check(self.lib.acs_sba_set_lm_layout(self.h, SBA_LM_LAYOUTS[layout]), 'acs_sba_set_lm_layout')

    def sba_lm_layout(self, n_slots, n_pts, cam_ids=False, camera_model='fisheye'):
        """acs_sba_lm_layout[_flags] -> ('butterfly' | 'row', n_cu): what a solve of this size would
        launch under the current setting, and the CU count the selection works with. The standard
        model always reports 'butterfly' (it has no row instance)."""
        n_cu = C.c_int32(0)
        rc = self.lib.acs_sba_lm_layout_flags(self.h, int(n_slots), int(n_pts), int(bool(cam_ids)), C.byref(n_cu),
                                              _model_flags(camera_model))
        if rc < 0:
            raise ValueError('acs_sba_lm_layout: bad arguments')
        return {v: k for k, v in SBA_LM_LAYOUTS.items()}[rc], int(n_cu.value)

    def sba_points_dense(self, cams, uv, mask, pts0, opts=None):
        cams, mf = _cams_flags(cams)
        C_ = len(cams)
        uv = _c64(uv).reshape(-1, C_, 2)
        mask = np.ascontiguousarray(mask, np.uint8).reshape(-1, C_)
        pts = _c64(pts0).reshape(-1, 3).copy()
        rep = Report()
        opts = opts or self.sba_opts()
        self.check(self.lib.acs_sba_points_dense(self.h, _ptr(cams), C_, _ptr(uv), _ptr(mask), len(pts), _ptr(pts),
                                                 C.byref(opts), C.byref(rep), mf), 'acs_sba_points_dense')
        return pts, rep.as_dict()

    def sba_points_dense_dev(self, cams_p, n_cams, uv_p, mask_p, n_pts, pts_p, opts=None, report=False,
                             pts_in_p=None, camera_model='fisheye'):
        """Device-pointer variant (inputs resident in HBM; asynchronous unless report).
        With `pts_in_p` the initial points are read from there and the solution written
        to `pts_p` (acs_sba_points_dense_io); otherwise `pts_p` is in/out. `camera_model` says
        what the records at `cams_p` are: 'fisheye' (20 doubles) or 'standard' (24)."""
        flags = ACS_DEVICE_PTRS | _model_flags(camera_model)
        opts = opts or self.sba_opts()
        rep = Report() if report else None
        rp = C.byref(rep) if rep is not None else None
        if pts_in_p is None:
            rc = self.lib.acs_sba_points_dense(self.h, C.c_void_p(cams_p), n_cams, C.c_void_p(uv_p),
                                               C.c_void_p(mask_p), n_pts, C.c_void_p(pts_p), C.byref(opts), rp,
                                               flags)
        else:
            rc = self.lib.acs_sba_points_dense_io(self.h, C.c_void_p(cams_p), n_cams, C.c_void_p(uv_p),
                                                  C.c_void_p(mask_p), n_pts, C.c_void_p(pts_in_p),
                                                  C.c_void_p(pts_p), C.byref(opts), rp, flags)
        self.check(rc, 'acs_sba_points_dense')
        return rep.as_dict() if rep is not None else None

    # ---- per-point position covariance of the points-only SBA ---------------------------
    def sba_points_covariance(self, cams, uv, pt_idx, cam_idx, pts, f_scale=50.0, sigma_px=1.0):
        """acs_sba_points_covariance at `pts` (nothing is solved): cov (n, 3, 3) = sigma_px^2 times
        the inverse of each point's undamped Triggs-weighted GN matrix, status (n,) int32
        (ACS_COV_OK 0 / NOOBS 1 / DEGENERATE 2; cov is NaN unless OK) and the report dict
        (n_points, n_ok, n_noobs, n_degenerate, var_min, var_max, sigma_hat_px). Observation
        list as sba_points; the record width selects the camera model."""
        cams, mf = _cams_flags(cams)
        uv = _c64(uv).reshape(-1, 2)
        pi = np.ascontiguousarray(pt_idx, np.int32)
        ci = np.ascontiguousarray(cam_idx, np.int32)
        pts = _c64(pts).reshape(-1, 3)
        n = len(pts)
        cov = np.empty((n, 3, 3))
        status = np.empty(n, np.int32)
        rep = SbaCovReport()
        self.check(self.lib.acs_sba_points_covariance(self.h, _ptr(cams), len(cams), _ptr(uv), _ptr(pi), _ptr(ci),
                                                      len(uv), _ptr(pts), n, float(f_scale), float(sigma_px),
                                                      _ptr(cov), _ptr(status), C.byref(rep), mf),
                   'acs_sba_points_covariance')
        return cov, status, rep.as_dict()

    def sba_points_dense_covariance(self, cams, uv, mask, pts, f_scale=50.0, sigma_px=1.0):
        """The dense form (uv (n, C, 2), mask (n, C)) of sba_points_covariance."""
        cams, mf = _cams_flags(cams)
        C_ = len(cams)
        uv = _c64(uv).reshape(-1, C_, 2)
        mask = np.ascontiguousarray(mask, np.uint8).reshape(-1, C_)
        pts = _c64(pts).reshape(-1, 3)
        n = len(pts)
        cov = np.empty((n, 3, 3))
        status = np.empty(n, np.int32)
        rep = SbaCovReport()
        self.check(self.lib.acs_sba_points_dense_covariance(self.h, _ptr(cams), C_, _ptr(uv), _ptr(mask), n, _ptr(pts),
                                                            float(f_scale), float(sigma_px), _ptr(cov), _ptr(status),
                                                            C.byref(rep), mf), 'acs_sba_points_dense_covariance')
        return cov, status, rep.as_dict()

    def sba_points_dense_covariance_dev(self, cams_p, n_cams, uv_p, mask_p, n_pts, pts_p, cov_p, status_p=None,
                                        f_scale=50.0, sigma_px=1.0, report=False, camera_model='fisheye'):
        """Device-pointer variant (every array resident in HBM, cov (n, 3, 3) and the optional int32
        status written there; only enqueues on the context stream unless `report`, which waits and
        returns the report dict)."""
        flags = ACS_DEVICE_PTRS | _model_flags(camera_model)
        rep = SbaCovReport() if report else None
        v = lambda p: C.c_void_p(p) if p else None  # noqa: E731
        self.check(self.lib.acs_sba_points_dense_covariance(self.h, v(cams_p), n_cams, v(uv_p), v(mask_p), n_pts,
                                                            v(pts_p), float(f_scale), float(sigma_px), v(cov_p),
                                                            v(status_p), C.byref(rep) if report else None, flags),
                   'acs_sba_points_dense_covariance')
        return rep.as_dict() if report else None

    # ---- a6 -------------------------------------------------------------------------
    def sba_ext_opts(self, **kw):
        o = SbaExtOpts()
        self.lib.acs_sba_ext_default_opts(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def sba_extrinsics(self, cams, uv, pt_idx, cam_idx, pts0, opts=None, residuals=True):
        """Points + camera extrinsics LM. Returns (cams (C,20), pts (n,3), res_before, res_after, report)."""
        cams = _c64(cams).copy()
        uv = _c64(uv).reshape(-1, 2)
        pi = np.ascontiguousarray(pt_idx, np.int32)
        ci = np.ascontiguousarray(cam_idx, np.int32)
        pts = _c64(pts0).reshape(-1, 3).copy()
        rb = np.empty(2 * len(uv)) if residuals else None
        ra = np.empty(2 * len(uv)) if residuals else None
        rep = SbaExtReport()
        opts = opts or self.sba_ext_opts()
        self.check(self.lib.acs_sba_extrinsics(self.h, _ptr(cams), len(cams), _ptr(uv), _ptr(pi), _ptr(ci), len(uv),
                                               _ptr(pts), len(pts), C.byref(opts), _ptr(rb), _ptr(ra),
                                               C.byref(rep), _std_flag(cams)), 'acs_sba_extrinsics')
        return cams, pts, rb, ra, rep.as_dict()

    def sba_boards(self, cams, obj_pts, uv, mask, board_r, board_t, opts=None, residuals=True):
        """acs_sba_boards: camera extrinsics and one rigid pose per board image. cams (C, 20) fisheye
        records, obj_pts (nc, 3) board coordinates, uv (B, C, nc, 2), mask (B, C), board_r (B, 3, 3) and
        board_t (B, 3) with X = R_b p + t_b. Returns (cams, board_r, board_t, res_before, res_after,
        report); the residuals hold the seen views in (board, camera, corner, row) order."""
        cams = _c64(cams).copy()
        obj = _c64(obj_pts).reshape(-1, 3)
        mask = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
        n_b, n_c = mask.shape
        uv = _c64(uv, (n_b, n_c, len(obj), 2))
        poses = np.concatenate([_c64(board_r, (n_b, 9)), _c64(board_t, (n_b, 3))], 1)
        n_res = 2 * len(obj) * int(mask.sum())
        rb = np.empty(n_res) if residuals else None
        ra = np.empty(n_res) if residuals else None
        rep = SbaExtReport()
        opts = opts or self.sba_ext_opts()
        self.check(self.lib.acs_sba_boards(self.h, _ptr(cams), len(cams), _ptr(obj), len(obj), _ptr(uv), _ptr(mask),
                                           n_b, _ptr(poses), C.byref(opts), _ptr(rb), _ptr(ra), C.byref(rep),
                                           _std_flag(cams)), 'acs_sba_boards')
        return cams, poses[:, :9].reshape(n_b, 3, 3).copy(), poses[:, 9:].copy(), rb, ra, rep.as_dict()

    def sba_boards_dev(self, cams_p, n_cams, obj_p, n_corners, uv_p, mask_p, n_boards, poses_p, opts=None,
                       resid_before_p=0, resid_after_p=0):
        """acs_sba_boards on raw device addresses (ACS_DEVICE_PTRS): cameras and board poses (B, 12) are
        refined in place; returns the report dict."""
        rep = SbaExtReport()
        opts = opts or self.sba_ext_opts()
        v = lambda p: C.c_void_p(p) if p else None  # noqa: E731
        self.check(self.lib.acs_sba_boards(self.h, v(cams_p), n_cams, v(obj_p), n_corners, v(uv_p), v(mask_p), n_boards,
                                           v(poses_p), C.byref(opts), v(resid_before_p), v(resid_after_p),
                                           C.byref(rep), ACS_DEVICE_PTRS), 'acs_sba_boards')
        return rep.as_dict()

    def sba_boards_points(self, cams, obj_pts, uv, mask, board_r, board_t, pt_uv, pt_mask, pts0, opts=None,
                          residuals=True):
        """acs_sba_boards_points: `sba_boards` with free (hand-labelled) points in the same solve. The
        board arrays as `sba_boards`; pt_uv (n, C, 2), pt_mask (n, C) the dense observations of the n free
        points (a camera sees a point at most once) and pts0 (n, 3) their start; n = 0 is the
        boards-only solve. Returns (cams, board_r, board_t, pts, res_before, res_after, report); the
        residuals hold the board part as `sba_boards` gives it, then the seen (point, camera) pairs in
        (point, camera, row) order."""
        cams = _c64(cams).copy()
        obj = _c64(obj_pts).reshape(-1, 3)
        mask = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
        n_b, n_c = mask.shape
        uv = _c64(uv, (n_b, n_c, len(obj), 2))
        poses = np.concatenate([_c64(board_r, (n_b, 9)), _c64(board_t, (n_b, 3))], 1)
        pts = _c64(pts0).reshape(-1, 3).copy()
        n = len(pts)
        pmask = np.ascontiguousarray(np.asarray(pt_mask).reshape(n, n_c) != 0, np.uint8)
        puv = _c64(pt_uv, (n, n_c, 2))
        n_res = 2 * (len(obj) * int(mask.sum()) + int(pmask.sum()))
        rb = np.empty(n_res) if residuals else None
        ra = np.empty(n_res) if residuals else None
        rep = SbaExtReport()
        opts = opts or self.sba_ext_opts()
        none = lambda a: _ptr(a) if n else None  # noqa: E731
        self.check(self.lib.acs_sba_boards_points(self.h, _ptr(cams), len(cams), _ptr(obj), len(obj), _ptr(uv),
                                                  _ptr(mask), n_b, _ptr(poses), none(puv), none(pmask), n, none(pts),
                                                  C.byref(opts), _ptr(rb), _ptr(ra), C.byref(rep), _std_flag(cams)),
                   'acs_sba_boards_points')
        return cams, poses[:, :9].reshape(n_b, 3, 3).copy(), poses[:, 9:].copy(), pts, rb, ra, rep.as_dict()

    def sba_boards_points_dev(self, cams_p, n_cams, obj_p, n_corners, uv_p, mask_p, n_boards, poses_p, pt_uv_p,
                              pt_mask_p, n_pts, pts_p, opts=None, resid_before_p=0, resid_after_p=0):
        """acs_sba_boards_points on raw device addresses (ACS_DEVICE_PTRS): cameras, board poses (B, 12)
        and points (n, 3) are refined in place; the residual arrays hold 2 (nc seen views + seen point
        observations) doubles; returns the report dict."""
        rep = SbaExtReport()
        opts = opts or self.sba_ext_opts()
        v = lambda p: C.c_void_p(p) if p else None  # noqa: E731
        self.check(self.lib.acs_sba_boards_points(self.h, v(cams_p), n_cams, v(obj_p), n_corners, v(uv_p), v(mask_p),
                                                  n_boards, v(poses_p), v(pt_uv_p), v(pt_mask_p), n_pts, v(pts_p),
                                                  C.byref(opts), v(resid_before_p), v(resid_after_p), C.byref(rep),
                                                  ACS_DEVICE_PTRS), 'acs_sba_boards_points')
        return rep.as_dict()

    def sba_boards_covariance(self, cams, obj_pts, uv, mask, board_r, board_t, f_scale=1.0, sigma_px=1.0,
                              gauge='anchor', anchor=0):
        """acs_sba_boards_covariance at (`cams`, `board_r`, `board_t`) (nothing is solved): the covariance
        of the camera poses in the chosen gauge and of every board pose. Arrays as `sba_boards`. Returns
        (cov_cams (6C, 6C), cov_boards (B, 6, 6), board_status (B,) int32, report dict). Rows 6c..6c+5
        of cov_cams are camera c's (dw, dt): R <- exp([dw]x) R (rad), t <- t + dt (m); a board's block
        is its (dw_b, dt_b). gauge 'free': inner constraints over the camera parameters
        (sigma^2 pinv(S)); 'anchor': camera `anchor`'s pose held (its rows and columns are exact
        zeros). A degenerate problem (report['status'] = 1) returns NaN everywhere; a board that is
        not OK has a NaN block. `f_scale` is the solve's."""
        if gauge not in GAUGES:
            raise ValueError(f"gauge must be 'free' or 'anchor', not {gauge!r}")
        cams = _c64(cams)
        obj = _c64(obj_pts).reshape(-1, 3)
        mask = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
        n_b, n_c = mask.shape
        uv = _c64(uv, (n_b, n_c, len(obj), 2))
        poses = np.concatenate([_c64(board_r, (n_b, 9)), _c64(board_t, (n_b, 3))], 1)
        o = SbaExtCovOpts(GAUGES[gauge], int(anchor), 0, 0, float(f_scale), float(sigma_px))
        cov_c = np.empty((6 * len(cams), 6 * len(cams)))
        cov_b = np.empty((n_b, 6, 6))
        status = np.empty(n_b, np.int32)
        rep = SbaBoardsCovReport()
        self.check(self.lib.acs_sba_boards_covariance(self.h, _ptr(cams), len(cams), _ptr(obj), len(obj), _ptr(uv),
                                                      _ptr(mask), n_b, _ptr(poses), C.byref(o), _ptr(cov_c),
                                                      _ptr(cov_b), _ptr(status), C.byref(rep), _std_flag(cams)),
                   'acs_sba_boards_covariance')
        return cov_c, cov_b, status, rep.as_dict()

    def sba_boards_covariance_dev(self, cams_p, n_cams, obj_p, n_corners, uv_p, mask_p, n_boards, poses_p, cov_cams_p,
                                  cov_boards_p=0, status_p=0, f_scale=1.0, sigma_px=1.0, gauge='anchor', anchor=0):
        """acs_sba_boards_covariance on raw device addresses (ACS_DEVICE_PTRS); returns the report dict."""
        o = SbaExtCovOpts(GAUGES[gauge], int(anchor), 0, 0, float(f_scale), float(sigma_px))
        rep = SbaBoardsCovReport()
        v = lambda p: C.c_void_p(p) if p else None  # noqa: E731
        self.check(self.lib.acs_sba_boards_covariance(self.h, v(cams_p), n_cams, v(obj_p), n_corners, v(uv_p),
                                                      v(mask_p), n_boards, v(poses_p), C.byref(o), v(cov_cams_p),
                                                      v(cov_boards_p), v(status_p), C.byref(rep), ACS_DEVICE_PTRS),
                   'acs_sba_boards_covariance')
        return rep.as_dict()

    def sba_extrinsics_covariance(self, cams, uv, pt_idx, cam_idx, pts, f_scale=1.0, sigma_px=1.0, gauge='anchor',
                                  anchor=(0, 1), points=True):
        """acs_sba_extrinsics_covariance at (`cams`, `pts`) (nothing is solved): the covariance of the
        camera poses in the chosen gauge and the joint covariance of every point. Returns
        (cov_cams (6C, 6C), cov_points (n, 3, 3) or None, status (n,) int32, report dict).
        cov_cams rows 6c..6c+5 are camera c's (dw, dt): R <- exp([dw]x) R (rad), t <- t + dt (m).
        gauge 'free': inner constraints over the camera parameters (sigma^2 pinv(S)); 'anchor':
        camera anchor[0]'s pose and the distance between the centres of anchor[0] and anchor[1]
        held (camera anchor[0]'s rows and columns are exact zeros). A degenerate problem
        (report['status'] = 1) returns NaN everywhere. `f_scale` is the solve's."""
        if gauge not in GAUGES:
            raise ValueError(f"gauge must be 'free' or 'anchor', not {gauge!r}")
        cams = _c64(cams)
        uv = _c64(uv).reshape(-1, 2)
        pi = np.ascontiguousarray(pt_idx, np.int32)
        ci = np.ascontiguousarray(cam_idx, np.int32)
        pts = _c64(pts).reshape(-1, 3)
        n, nc = len(pts), len(cams)
        o = SbaExtCovOpts(GAUGES[gauge], int(anchor[0]), int(anchor[1]), 0, float(f_scale), float(sigma_px))
        cov_c = np.empty((6 * nc, 6 * nc))
        cov_p = np.empty((n, 3, 3)) if points else None
        status = np.empty(n, np.int32)
        rep = SbaExtCovReport()
        self.check(self.lib.acs_sba_extrinsics_covariance(self.h, _ptr(cams), nc, _ptr(uv), _ptr(pi), _ptr(ci), len(uv),
                                                          _ptr(pts), n, C.byref(o), _ptr(cov_c), _ptr(cov_p),
                                                          _ptr(status), C.byref(rep), _std_flag(cams)),
                   'acs_sba_extrinsics_covariance')
        return cov_c, cov_p, status, rep.as_dict()

    # ---- f2: EKF + RTS smoother ----------------------------------------------------------
    def ekf_run(self, table, cams, meas, likelihood, fps, thresh, max_pixel_err, r_std_base, Q, P0, s0,
                ref_numerics=True, eps=1e-3, covariances=False, jacobian='fd'):
        """meas (S, N, C, L, 2) or (N, C, L, 2); returns dict of x_pred, x_est, x_smooth
        (S, N, n) [, P_est, P_smooth (S, N, n, n)], outliers (S,)."""
        cams = _c64(cams)
        meas = _c64(meas)
        single = meas.ndim == 4
        if single:
            meas = meas[None]
        S, N, Cn, L, _ = meas.shape
        assert L == table.L and Cn == len(cams), (meas.shape, table.L, len(cams))
        lik = _c64(likelihood).reshape(S, N, Cn, L)
        n = 3 * table.P
        s0 = _c64(s0).reshape(S, n)
        out = {k: np.empty((S, N, n)) for k in ('x_pred', 'x_est', 'x_smooth')}
        if covariances:
            out.update(P_est=np.empty((S, N, n, n)), P_smooth=np.empty((S, N, n, n)))
        outl = np.zeros(S, np.int64)
        ints = np.ascontiguousarray(table.ints, np.int32)
        reals = np.ascontiguousarray(table.reals, np.float64)
        self.check(self.lib.acs_ekf_run(self.h, _ptr(ints), len(ints), _ptr(reals), len(reals), _ptr(cams), Cn,
                                        _ptr(meas), _ptr(lik), S, N, float(fps), float(thresh), float(max_pixel_err),
                                        _ptr(_c64(r_std_base)), _ptr(_c64(Q)), _ptr(_c64(P0)), _ptr(s0),
                                        ekf_numerics_mode(ref_numerics, jacobian), float(eps), _ptr(out['x_pred']), _ptr(out['x_est']),
                                        _ptr(out['x_smooth']), _ptr(out.get('P_est')), _ptr(out.get('P_smooth')),
                                        _ptr(outl), _std_flag(cams)), 'acs_ekf_run')
        out['outliers'] = outl
        if single:
            out = {k: v[0] for k, v in out.items()}
        return out

    def ekf_run_dev(self, ints_p, n_ints, reals_p, n_reals, cams_p, n_cams, meas_p, lik_p, S, N, fps, thresh,
                    max_pixel_err, r_std_p, Q_p, P0_p, s0_p, x_est_p, x_smooth_p, x_pred_p=None, ref_numerics=True,
                    eps=1e-3, jacobian='fd'):
        """acs_ekf_run on device pointers (ACS_DEVICE_PTRS: inputs resident in HBM, outputs
        written there; asynchronous on the context stream, no outliers report): the layouts of
        ekf_run, every pointer an int (torch data_ptr()). Being asynchronous, the call does not
        check for singular solves itself: read them afterwards with ekf_singular_count()."""
        v = lambda p: C.c_void_p(p) if p else None  # noqa: E731
        self.check(self.lib.acs_ekf_run(self.h, v(ints_p), n_ints, v(reals_p), n_reals, v(cams_p), n_cams, v(meas_p),
                                        v(lik_p), S, N, float(fps), float(thresh), float(max_pixel_err), v(r_std_p),
                                        v(Q_p), v(P0_p), v(s0_p), ekf_numerics_mode(ref_numerics, jacobian),
                                        float(eps), v(x_pred_p), v(x_est_p), v(x_smooth_p), None, None, None,
                                        ACS_DEVICE_PTRS), 'acs_ekf_run')

    def ekf_singular_count(self):
        """Singular solves of the last EKF enqueue on this context (waits for its stream)."""
        n = C.c_int32(0)
        self.check(self.lib.acs_ekf_singular_count(self.h, C.byref(n)), 'acs_ekf_singular_count')
        return int(n.value)

    # ---- configs[4]: SBA + EKF fused ------------------------------------------------
    def sba_ekf_pipeline(self, table, cams, meas, likelihood, obs_markers, fps, thresh, max_pixel_err, r_std_base, Q,
                         P0, sba_opts=None, from_sba=False, ref_numerics=True, eps=1e-3, jacobian='fd'):
        """acs_sba_ekf_pipeline on host arrays: meas (S, N, C, Lobs, 2), likelihood (S, N, C,
        Lobs) with markers `obs_markers`; the EKF runs skeleton `table` (its markers a subset of
        obs_markers). Returns dict pts (S, N, Lobs, 3), x_est, x_smooth (S, N, 3P), outliers
        (S,), sba (report dict)."""
        cams = _c64(cams)
        meas = _c64(meas)
        S, N, Cn, Lo, _ = meas.shape
        assert Lo == len(obs_markers) and Cn == len(cams), (meas.shape, len(obs_markers), len(cams))
        lik = _c64(likelihood).reshape(S, N, Cn, Lo)
        obs = list(obs_markers)
        emap = np.array([obs.index(m) for m in table.markers], np.int32)
        n = 3 * table.P
        pts = np.empty((S, N, Lo, 3))
        xe = np.empty((S, N, n))
        xs = np.empty((S, N, n))
        outl = np.zeros(S, np.int64)
        rep = Report()
        opts = sba_opts or self.sba_opts()
        spec = ekf_init_spec(table, obs, from_sba)
        ints = np.ascontiguousarray(table.ints, np.int32)
        reals = np.ascontiguousarray(table.reals, np.float64)
        self.check(self.lib.acs_sba_ekf_pipeline(
            self.h, _ptr(ints), len(ints), _ptr(reals), len(reals), _ptr(cams), Cn, _ptr(meas), _ptr(lik), S, N, Lo,
            _ptr(emap), float(fps), float(thresh), float(max_pixel_err), _ptr(_c64(r_std_base)), _ptr(_c64(Q)),
            _ptr(_c64(P0)), C.byref(opts), C.byref(spec), ekf_numerics_mode(ref_numerics, jacobian), float(eps), _ptr(pts), _ptr(xe),
            _ptr(xs), _ptr(outl), C.byref(rep), _std_flag(cams)), 'acs_sba_ekf_pipeline')
        return dict(pts=pts, x_est=xe, x_smooth=xs, outliers=outl, sba=rep.as_dict())

    def sba_ekf_pipeline_dev(self, table, obs_markers, cams_p, n_cams, meas_p, lik_p, S, N, fps, thresh,
                             max_pixel_err, rstd_p, Q_p, P0_p, pts_p, xe_p, xs_p, sba_opts=None, from_sba=False,
                             ref_numerics=True, eps=1e-3, report=False, jacobian='fd'):
        """acs_sba_ekf_pipeline on HBM-resident arrays (device pointers, asynchronous unless
        `report`: then waits and returns (sba report dict, outliers (S,)))."""
        obs = list(obs_markers)
        emap = np.array([obs.index(m) for m in table.markers], np.int32)
        spec = ekf_init_spec(table, obs, from_sba)
        opts = sba_opts or self.sba_opts()
        ints = np.ascontiguousarray(table.ints, np.int32)
        reals = np.ascontiguousarray(table.reals, np.float64)
        rep = Report() if report else None
        outl = np.zeros(S, np.int64) if report else None
        P_ = C.c_void_p
        self.check(self.lib.acs_sba_ekf_pipeline(
            self.h, _ptr(ints), len(ints), _ptr(reals), len(reals), P_(cams_p), n_cams, P_(meas_p), P_(lik_p), S, N,
            len(obs), _ptr(emap), float(fps), float(thresh), float(max_pixel_err), P_(rstd_p), P_(Q_p), P_(P0_p),
            C.byref(opts), C.byref(spec), ekf_numerics_mode(ref_numerics, jacobian), float(eps), P_(pts_p), P_(xe_p), P_(xs_p),
            _ptr(outl), C.byref(rep) if report else None, ACS_DEVICE_PTRS), 'acs_sba_ekf_pipeline')
        return (rep.as_dict(), outl) if report else None

    # ---- a9 -------------------------------------------------------------------------
    def redescending_loss(self, err, a=3.0, b=10.0, c=20.0, deriv=False):
        e = _c64(err).ravel()
        out = np.empty_like(e)
        d = np.empty_like(e) if deriv else None
        self.check(self.lib.acs_redescending_loss(self.h, _ptr(e), len(e), a, b, c, _ptr(out), _ptr(d), 0),
                   'acs_redescending_loss')
        return (out, d) if deriv else out

    # ---- a7 -------------------------------------------------------------------------
    def fk(self, table, x, dx=None, ddx=None, tau=None, intermode=0, directions=False, jac=False):
        x = _c64(x).reshape(-1, table.P)
        n = len(x)
        dx = None if dx is None else _c64(dx).reshape(n, table.P)
        ddx = None if ddx is None else _c64(ddx).reshape(n, table.P)
        tau = None if tau is None else _c64(np.broadcast_to(tau, (n,)))
        Lo = table.L + (2 if directions else 0)
        out = np.empty((n, Lo, 3))
        J = np.empty((n, table.L, 3, table.P)) if jac else None
        ints = np.ascontiguousarray(table.ints, np.int32)
        reals = np.ascontiguousarray(table.reals, np.float64)
        self.check(self.lib.acs_fk(self.h, _ptr(ints), len(ints), _ptr(reals), len(reals), _ptr(x), _ptr(dx),
                                   _ptr(ddx), _ptr(tau), n, int(intermode), int(bool(directions)), _ptr(out),
                                   _ptr(J), 0), 'acs_fk')
        return (out, J) if jac else out

    # ---- a10-a13: FTE ------------------------------------------------------------------
    def fte_default_opts(self, **kw):
        o = FteOpts()
        self.lib.acs_fte_default_opts(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def _fte_args(self, table, cams, meas, w, Ts, qinv, shutter_delay, intermode):
        cams = _c64(cams)
        N, Cn, L, _ = np.shape(meas)
        assert L == table.L and Cn == len(cams), (np.shape(meas), table.L, len(cams))
        meas = _c64(np.nan_to_num(meas))
        w = _c64(w).reshape(N, Cn, L)
        qinv = _c64(qinv).reshape(table.P)
        ints = np.ascontiguousarray(table.ints, np.int32)
        reals = np.ascontiguousarray(table.reals, np.float64)
        return ints, reals, cams, meas, w, qinv, N, Cn

    @staticmethod
    def _tau_init(tau, N, Cn, sd_mode):
        """Shutter delays in the layout of sd_mode (0 const: (C,), 1 variable: (N, C)),
        camera 0 pinned at 0 (src/core/fte.py:304-308)."""
        shape = (N, Cn) if sd_mode == 1 else (Cn,)
        t = np.zeros(shape) if tau is None else np.array(np.broadcast_to(_c64(tau), shape), np.float64)
        t[..., 0] = 0.0
        return np.ascontiguousarray(t)

    def fte_solve(self, table, cams, meas, w, Ts, qinv, X0, tau0=None, shutter_delay=True, intermode=1,
                  opts=None, sd_mode=0):
        """sd_mode 0 = 'const' (tau (C,)), 1 = 'variable' (tau (N, C), src/core/fte.py:236-238)."""
        ints, reals, cams, meas, w, qinv, N, Cn = self._fte_args(table, cams, meas, w, Ts, qinv, shutter_delay,
                                                                 intermode)
        sd_mode = SD_MODES.get(sd_mode, sd_mode)
        X = _c64(X0).reshape(N + 2, table.P).copy()
        tau = self._tau_init(tau0, N, Cn, sd_mode)
        rep = FteReport()
        opts = opts or self.fte_default_opts()
        self.check(self.lib.acs_fte_solve(self.h, _ptr(ints), len(ints), _ptr(reals), len(reals), _ptr(cams), Cn,
                                          _ptr(meas), _ptr(w), N, int(bool(shutter_delay)), float(Ts), _ptr(qinv),
                                          int(sd_mode), int(intermode), _ptr(X), _ptr(tau), C.byref(opts),
                                          C.byref(rep), _std_flag(cams)), 'acs_fte_solve')
        return X, tau, rep.as_dict()

    def fte_solve_dev(self, table_ints_p, n_ints, table_reals_p, n_reals, cams_p, n_cams, meas_p, w_p, N,
                      shutter_delay, Ts, qinv_p, intermode, X_p, tau_p, opts=None, sd_mode=0):
        """Device-pointer variant (all arrays resident in HBM); returns the report."""
        sd_mode = SD_MODES.get(sd_mode, sd_mode)
        rep = FteReport()
        opts = opts or self.fte_default_opts()
        self.check(self.lib.acs_fte_solve(self.h, C.c_void_p(table_ints_p), n_ints, C.c_void_p(table_reals_p), n_reals,
                                          C.c_void_p(cams_p), n_cams, C.c_void_p(meas_p), C.c_void_p(w_p), N,
                                          int(bool(shutter_delay)), float(Ts), C.c_void_p(qinv_p), int(sd_mode),
                                          int(intermode),
                                          C.c_void_p(X_p), C.c_void_p(tau_p), C.byref(opts), C.byref(rep),
                                          ACS_DEVICE_PTRS), 'acs_fte_solve')
        return rep.as_dict()

    def fte_eval(self, table, cams, meas, w, Ts, qinv, X, tau=None, shutter_delay=True, intermode=1, hessian=True,
                 sd_mode=0):
        ints, reals, cams, meas, w, qinv, N, Cn = self._fte_args(table, cams, meas, w, Ts, qinv, shutter_delay,
                                                                 intermode)
        sd_mode = SD_MODES.get(sd_mode, sd_mode)
        X = _c64(X).reshape(N + 2, table.P)
        tau = np.zeros((N, Cn) if sd_mode == 1 else Cn) if tau is None else _c64(tau)
        nv = (N + 2) * table.P + ((N * Cn if sd_mode == 1 else Cn) if shutter_delay else 0)
        cost = np.empty(3)
        grad = np.empty(nv)
        H = np.empty((nv, nv)) if hessian else None
        self.check(self.lib.acs_fte_eval(self.h, _ptr(ints), len(ints), _ptr(reals), len(reals), _ptr(cams), Cn,
                                         _ptr(meas), _ptr(w), N, int(bool(shutter_delay)), float(Ts), _ptr(qinv),
                                         int(sd_mode), int(intermode), _ptr(X), _ptr(tau), _ptr(cost), _ptr(grad),
                                         _ptr(H), _std_flag(cams)),
                   'acs_fte_eval')
        return cost, grad, H

    def fte_covariance(self, table, cams, meas, w, Ts, qinv, X, tau=None, shutter_delay=True, intermode=1,
                       markers=False, sd_mode=0):
        """acs_fte_covariance: the blocks of the inverse of the undamped GN normal matrix at (X, tau)
        (held delays removed). Returns a dict: x_cov (N + 2, P, P), rows as X; tau_cov (C, C), held
        rows / columns zero; marker_cov (N, L, 3, 3) if `markers` else None; and the report fields
        n_bad_pivots, n_tau_free, var_min, var_max. Constant or no shutter delay only."""
        ints, reals, cams, meas, w, qinv, N, Cn = self._fte_args(table, cams, meas, w, Ts, qinv, shutter_delay,
                                                                 intermode)
        sd_mode = SD_MODES.get(sd_mode, sd_mode)
        X = _c64(X).reshape(N + 2, table.P)
        tau = self._tau_init(tau, N, Cn, sd_mode)
        x_cov = np.empty((N + 2, table.P, table.P))
        tau_cov = np.empty((Cn, Cn))
        marker_cov = np.empty((N, table.L, 3, 3)) if markers else None
        rep = FteCovReport()
        self.check(self.lib.acs_fte_covariance(self.h, _ptr(ints), len(ints), _ptr(reals), len(reals), _ptr(cams), Cn,
                                               _ptr(meas), _ptr(w), N, int(bool(shutter_delay)), float(Ts),
                                               _ptr(qinv), int(sd_mode), int(intermode), _ptr(X), _ptr(tau),
                                               _ptr(x_cov), _ptr(tau_cov), _ptr(marker_cov), C.byref(rep),
                                               _std_flag(cams)),
                   'acs_fte_covariance')
        return dict(x_cov=x_cov, tau_cov=tau_cov, marker_cov=marker_cov, n_bad_pivots=int(rep.n_bad_pivots),
                    n_tau_free=int(rep.n_tau_free), var_min=float(rep.var_min), var_max=float(rep.var_max))

    def fte_covariance_dev(self, table_ints_p, n_ints, table_reals_p, n_reals, cams_p, n_cams, meas_p, w_p, N,
                           shutter_delay, Ts, qinv_p, intermode, X_p, tau_p, x_cov_p, tau_cov_p=None,
                           marker_cov_p=None, report=False):
        """Device-pointer variant (every array resident in HBM, outputs written there; asynchronous
        on the context stream unless `report`, which waits and returns the report dict)."""
        v = lambda p: C.c_void_p(p) if p else None  # noqa: E731
        rep = FteCovReport() if report else None
        self.check(self.lib.acs_fte_covariance(self.h, v(table_ints_p), n_ints, v(table_reals_p), n_reals, v(cams_p),
                                               n_cams, v(meas_p), v(w_p), N, int(bool(shutter_delay)), float(Ts),
                                               v(qinv_p), 0, int(intermode), v(X_p), v(tau_p), v(x_cov_p),
                                               v(tau_cov_p), v(marker_cov_p), C.byref(rep) if report else None,
                                               ACS_DEVICE_PTRS), 'acs_fte_covariance')
        if not report:
            return None
        return dict(n_bad_pivots=int(rep.n_bad_pivots), n_tau_free=int(rep.n_tau_free), var_min=float(rep.var_min),
                    var_max=float(rep.var_max))

    def fte_debug_blocks(self, table, cams, meas, w, Ts, qinv, X, tau=None, lam=0.0, levels=0, shutter_delay=True,
                         intermode=1):
        """acs_fte_debug_blocks (test hook): the damped super-blocks D (n_blk, BP, BP) of the FTE's
        block-tridiagonal system at (X, tau), after `levels` cyclic-reduction levels with the
        pending Schur terms applied (blocks 2^levels m then hold the D the next level factors).
        Returns (D, levels run)."""
        ints, reals, cams, meas, w, qinv, N, Cn = self._fte_args(table, cams, meas, w, Ts, qinv, shutter_delay,
                                                                 intermode)
        X = _c64(X).reshape(N + 2, table.P)
        tau = self._tau_init(tau, N, Cn, 0)
        nblk = (N + 2 + 2) // 3
        BP = ((3 * table.P + 15) // 16) * 16
        D = np.empty((nblk, BP, BP))
        dims = (C.c_int64 * 3)()
        self.check(self.lib.acs_fte_debug_blocks(self.h, _ptr(ints), len(ints), _ptr(reals), len(reals), _ptr(cams), Cn,
                                                 _ptr(meas), _ptr(w), N, int(bool(shutter_delay)), float(Ts),
                                                 _ptr(qinv), 0, int(intermode), _ptr(X), _ptr(tau), float(lam),
                                                 int(levels), _ptr(D), dims, _std_flag(cams)), 'acs_fte_debug_blocks')
        assert dims[0] == nblk and dims[1] == BP, (list(dims), nblk, BP)
        return D, int(dims[2])

    # ---- triangulation -------------------------------------------------
    def triangulate_pairs(self, cams, uv_a, uv_b, cam_a, cam_b):
        cams, mf = _cams_flags(cams)
        uv_a = _c64(uv_a).reshape(-1, 2)
        uv_b = _c64(uv_b).reshape(-1, 2)
        n = len(uv_a)
        ca = np.ascontiguousarray(np.broadcast_to(cam_a, (n,)), np.int32)
        cb = np.ascontiguousarray(np.broadcast_to(cam_b, (n,)), np.int32)
        out = np.empty((n, 3))
        self.check(self.lib.acs_triangulate_pairs(self.h, _ptr(cams), len(cams), _ptr(uv_a), _ptr(uv_b), _ptr(ca),
                                                  _ptr(cb), n, _ptr(out), mf), 'acs_triangulate_pairs')
        return out

    def triangulate_dense(self, cams, uv, mask):
        cams, mf = _cams_flags(cams)
        C_ = len(cams)
        uv = _c64(np.nan_to_num(uv)).reshape(-1, C_, 2)
        mask = np.ascontiguousarray(mask, np.uint8).reshape(-1, C_)
        n = len(uv)
        out = np.empty((n, 3))
        cnt = np.empty(n, np.int32)
        self.check(self.lib.acs_triangulate_dense(self.h, _ptr(cams), C_, _ptr(uv), _ptr(mask), n, _ptr(out),
                                                  _ptr(cnt), mf), 'acs_triangulate_dense')
        return out, cnt


_default_ctx = None


def default_context() -> Context:
    """Process-wide context on the device selected by LOCAL_RANK (default 0)."""
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(int(os.environ.get('ACINOSET_DEVICE', os.environ.get('LOCAL_RANK', 0))))
    return _default_ctx
