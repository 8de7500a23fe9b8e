/*
 * acinoset_hip.h — C ABI of the MI355X-native AcinoSet SBA/FTE core
 * (libacinoset_hip.so, HIP kernels for gfx950).
 *
 * The reference has no FFI layer: its seams are Python call signatures. Every entry
 * point below replaces the numeric body of one of those seams (cited per function);
 * the Python drop-ins in acinoset_amd/lib and acinoset_amd/core bind them via ctypes
 * (INTEGRATION.md shows the binding a reference maintainer would add).
 *
 * Conventions
 *  - All functions return an int status: ACS_OK (0) or a negative ACS_E_* code; the
 *    message is in acs_last_error(ctx).
 *  - Array arguments are HOST pointers (copied into context-owned device buffers and
 *    back) unless ACS_DEVICE_PTRS is set in `flags`, in which case every array pointer
 *    of that call is a device pointer and the call is asynchronous on the context
 *    stream (results valid after acs_ctx_sync or a later synchronous call).
 *  - float64 everywhere (the reference is float64 throughout: src/lib/utils.py:68-71).
 *  - Camera block: ACS_CAM_STRIDE doubles per camera:
 *      [fx, fy, cx, cy, k1, k2, k3, k4, R00..R22 (row-major), t0, t1, t2]
 *    = K[0,0], K[1,1], K[0,2], K[1,2] of the scene JSON 'k', 'd' (4), 'r' (3x3), 't' (3)
 *    (src/lib/utils.py:55-74). Skew K[0,1] is ignored, as by cv::fisheye (alpha = 0).
 *  - One context = one HIP device + one stream; calls on a context are not thread-safe.
 */
#ifndef ACINOSET_HIP_H
#define ACINOSET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACS_ABI_VERSION 5
#define ACS_CAM_STRIDE 20
#define ACS_CAM_STRIDE_STD 24 /* standard (pinhole) camera records, see ACS_CAMS_STANDARD */

/* status codes */
#define ACS_OK 0
#define ACS_E_INVALID -1   /* bad argument / shape */
#define ACS_E_HIP -2       /* HIP runtime error */
#define ACS_E_NOMEM -3     /* device allocation failed */
#define ACS_E_NODEV -4     /* no usable gfx950 device */

/* flags */
#define ACS_DEVICE_PTRS 1u  /* array arguments are device pointers; call is async */
/* `cams` holds standard-model (cv::projectPoints) records of ACS_CAM_STRIDE_STD doubles:
 *   [fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6, R00..R22 (row-major), t0, t1, t2]
 * (a shorter OpenCV coefficient vector zero-padded; skew ignored). Accepted by acs_project_standard,
 * acs_sba_residuals, acs_sba_points, acs_sba_points_dense[_io], acs_sba_points_covariance,
 * acs_sba_points_dense_covariance, acs_triangulate_pairs and acs_triangulate_dense; every other
 * entry point that takes cameras returns ACS_E_INVALID when the bit is set.               */
#define ACS_CAMS_STANDARD 2u

/* per-problem convergence status (acs_report.status_counts index / oracle/sba.py) */
/* acs_ekf_run / acs_sba_ekf_pipeline measurement-model mode (their ref_numerics argument) */
#define ACS_EKF_ANALYTIC_H 2

#define ACS_STATUS_RUNNING 0
#define ACS_STATUS_GTOL 1
#define ACS_STATUS_FTOL 2
#define ACS_STATUS_XTOL 3
#define ACS_STATUS_STALLED 4
#define ACS_STATUS_MAXITER 5
#define ACS_STATUS_NOOBS 6
#define ACS_N_STATUS 7

/* LM steps whose model decrease -g.dx - dx.H.dx/2 is <= ACS_COST_RES * cost are below the
 * resolution of a float64 cost sum: the problem stops as converged (ACS_STATUS_FTOL)
 * instead of letting rounding accept or reject the step (points-only SBA).              */
#define ACS_COST_RES 1e-14

typedef struct acs_ctx acs_ctx;

typedef struct {
  int32_t max_iters;  /* LM iterations (accepted + rejected) per problem; default 100 */
  int32_t reserved;
  double f_scale;     /* Cauchy soft-threshold in px; reference default 50 (src/lib/sba.py:181) */
  double ftol;        /* relative cost decrease; reference passes 1e-15 (src/lib/sba.py:189) */
  double xtol;        /* relative step; default 1e-9 (scipy default 1e-8) */
  double gtol;        /* max |gradient|; default 1e-10 */
} acs_sba_opts;

typedef struct {
  int64_t n_problems;                   /* points (SBA) or 1 (FTE) */
  int64_t status_counts[ACS_N_STATUS];  /* problems ending in each ACS_STATUS_* */
  int64_t iters_max;                    /* max LM iterations over problems */
  int64_t iters_sum;                    /* total LM iterations */
  int64_t nfev_sum;                     /* total cost evaluations */
  double cost_before;                   /* sum of robust cost at x0 */
  double cost_after;                    /* sum of robust cost at the solution */
} acs_report;

/* ---- context -------------------------------------------------------------------- */
int acs_ctx_create(int device, acs_ctx** out);
int acs_ctx_destroy(acs_ctx* ctx);
const char* acs_last_error(const acs_ctx* ctx);
int acs_ctx_set_stream(acs_ctx* ctx, void* hip_stream);  /* NULL = context's own stream */
int acs_ctx_sync(acs_ctx* ctx);
int acs_abi_version(void);
int acs_device_count(int* n);
/* Device and pinned-host allocations + frees the library has made in this process (a
 * counter; no GPU needed): a timed region that reuses its buffers leaves it unchanged. */
int64_t acs_alloc_events(void);
void acs_sba_default_opts(acs_sba_opts* o);

/* ---- a1: fisheye projection (src/lib/calib.py:132-136, src/core/fte.py:80-96) -------
 * uv[i] = project(cams[cam_idx[i]], pts[i]); cam_idx may be NULL (all camera 0).
 * fte_form != 0 uses the FTE restatement r = sqrt(a^2 + b^2 + 1e-12) (fte.py:88)
 * instead of OpenCV's r > 1e-8 guard.                                                 */
int acs_project_fisheye(acs_ctx* ctx, const double* cams, int32_t n_cams, const double* pts,
                        const int32_t* cam_idx, int64_t n, int32_t fte_form, double* uv_out,
                        uint32_t flags);

/* ---- standard-model projection (project_points, src/lib/calib.py:65-67) --------------
 * As acs_project_fisheye for ACS_CAM_STRIDE_STD records (ACS_CAMS_STANDARD is implied and
 * may be set): a = Y0/Y2, b = Y1/Y2, r2 = a^2 + b^2,
 *   cd = (1 + k1 r2 + k2 r2^2 + k3 r2^3) / (1 + k4 r2 + k5 r2^2 + k6 r2^3)
 *   u = fx (a cd + 2 p1 a b + p2 (r2 + 2 a^2)) + cx,  v = fy (b cd + p1 (r2 + 2 b^2) + 2 p2 a b) + cy
 * with no guard on Y2 (a point behind the camera projects by the same formula, as OpenCV's). */
int acs_project_standard(acs_ctx* ctx, const double* cams, int32_t n_cams, const double* pts,
                         const int32_t* cam_idx, int64_t n, double* uv_out, uint32_t flags);

/* ---- a2: SBA residual vector (cost_func_points_only, src/lib/sba.py:149-153) -------
 * resid[2i+d] = project(cams[cam_idx[i]], pts[pt_idx[i]])[d] - uv[2i+d]              */
int acs_sba_residuals(acs_ctx* ctx, const double* cams, int32_t n_cams, const double* uv,
                      const int32_t* pt_idx, const int32_t* cam_idx, int64_t n_obs,
                      const double* pts, int64_t n_pts, double* resid_out, uint32_t flags);

/* ---- a3/a4: points-only SBA (bundle_adjust_points_only, src/lib/sba.py:181-195) -----
 * Observation list as the reference passes it (points_2d, point_3d_indices,
 * camera_indices; any order, duplicates allowed). pts (n_pts x 3) is the initial
 * estimate on input and the solution on output. resid_before / resid_after (2*n_obs,
 * may be NULL) are the reference's residuals['before'/'after']. report may be NULL.  */
int acs_sba_points(acs_ctx* ctx, const double* cams, int32_t n_cams, const double* uv,
                   const int32_t* pt_idx, const int32_t* cam_idx, int64_t n_obs, double* pts,
                   int64_t n_pts, const acs_sba_opts* opts, double* resid_before,
                   double* resid_after, acs_report* report, uint32_t flags);

/* ---- dense observation-tensor SBA (the core.sba layout, src/core/sba.py:41-43) ------
 * Point p = one (frame, marker); uv is (n_pts, n_cams, 2), mask (n_pts, n_cams) u8
 * (1 = valid observation). Same solver as acs_sba_points.                             */
int acs_sba_points_dense(acs_ctx* ctx, const double* cams, int32_t n_cams, const double* uv,
                         const uint8_t* mask, int64_t n_pts, double* pts,
                         const acs_sba_opts* opts, acs_report* report, uint32_t flags);
/* Same solve with separate initial (pts_in) and solution (pts_out) buffers, so a repeated
 * solve from one initialisation needs no reset copy (pts_in == pts_out is allowed).    */
int acs_sba_points_dense_io(acs_ctx* ctx, const double* cams, int32_t n_cams, const double* uv,
                            const uint8_t* mask, int64_t n_pts, const double* pts_in, double* pts_out,
                            const acs_sba_opts* opts, acs_report* report, uint32_t flags);

/* ---- per-point position covariance of the points-only SBA -----------------------------
 * For point i with observations o, residuals r_od (pixels) at `pts`, z = r^2 / f_scale^2 and
 * w = 1 / (1 + z):
 *   H_i = sum_o sum_d wh_od J_od^T J_od,  wh = max((1 - z) w^2, 0.1 w)
 * (the solver's own Triggs-weighted Gauss-Newton matrix, undamped, evaluated at the points
 * passed in: nothing is solved here), and
 *   cov_i = sigma_px^2 H_i^-1   (m^2; sigma_px = the pixel noise the caller assumes, e.g. 1).
 * The inverse is an LDL^T without pivoting with pivots d0, d1, d2; the point is DEGENERATE when
 * any pivot fails d > 1e-9 max(H00, H11, H22) (a NaN fails it): a point seen by one camera, or
 * by cameras on one line with it. status (int32 per point, may be NULL) is ACS_COV_*; for a
 * status other than ACS_COV_OK all nine entries of the point's cov are NaN. cov (n_pts, 3, 3)
 * is exactly symmetric. The report (may be NULL; waits for the stream) counts the statuses
 * and gives the extreme marginal variances over the OK points and the a-posteriori pixel scale
 *   sigma_hat_px^2 = sum w r^2 / (m - 3 n_ok)
 * over the observations of the OK points, m their number of scalar residuals (NaN when
 * m <= 3 n_ok): reported, never applied to cov. Observation layouts, ACS_CAMS_STANDARD and
 * ACS_DEVICE_PTRS as acs_sba_points / acs_sba_points_dense; with device pointers and no report
 * the call only enqueues on the context stream.                                          */
#define ACS_COV_OK 0
#define ACS_COV_NOOBS 1
#define ACS_COV_DEGENERATE 2
typedef struct {
  int64_t n_points, n_ok, n_noobs, n_degenerate;
  double var_min, var_max;  /* extreme diagonal entries of cov over the OK points (NaN: none) */
  double sigma_hat_px;
} acs_sba_cov_report;
int acs_sba_points_covariance(acs_ctx* ctx, const double* cams, int32_t n_cams, const double* uv,
                              const int32_t* pt_idx, const int32_t* cam_idx, int64_t n_obs,
                              const double* pts, int64_t n_pts, double f_scale, double sigma_px,
                              double* cov, int32_t* status, acs_sba_cov_report* report, uint32_t flags);
int acs_sba_points_dense_covariance(acs_ctx* ctx, const double* cams, int32_t n_cams, const double* uv,
                                    const uint8_t* mask, int64_t n_pts, const double* pts, double f_scale,
                                    double sigma_px, double* cov, int32_t* status,
                                    acs_sba_cov_report* report, uint32_t flags);

/* Test hook: which instance of the LM kernel a points-only solve of this context launches.
 * AUTO (the default) takes the row instance (one point per 16-lane row, row-broadcast sums) for
 * 3..8 observation slots without camera ids when the grid is at most one wave per SIMD, else
 * the butterfly instances; BUTTERFLY and ROW force either wherever both are legal (3..8 slots,
 * no camera ids). The instances give bit-identical results.                               */
#define ACS_SBA_LM_AUTO 0
#define ACS_SBA_LM_BUTTERFLY 1
#define ACS_SBA_LM_ROW 2
int acs_sba_set_lm_layout(acs_ctx* ctx, int32_t layout);
/* -> ACS_SBA_LM_BUTTERFLY or ACS_SBA_LM_ROW: what a solve of n_pts points with n_slots
 * observation slots per point would launch under the context's setting (-1: bad arguments).
 * n_cu (may be NULL) receives the CU count the selection works with.                        */
int acs_sba_lm_layout(const acs_ctx* ctx, int32_t n_slots, int64_t n_pts, int32_t with_cam_ids,
                      int32_t* n_cu);
/* The same for a solve whose call carries `flags`: with ACS_CAMS_STANDARD always
 * ACS_SBA_LM_BUTTERFLY (the standard model has the LDS-staged butterfly instances only). */
int acs_sba_lm_layout_flags(const acs_ctx* ctx, int32_t n_slots, int64_t n_pts, int32_t with_cam_ids,
                            int32_t* n_cu, uint32_t flags);

/* ---- a9: redescending loss (src/lib/misc.py:329-343), elementwise ------------------ */
int acs_redescending_loss(acs_ctx* ctx, const double* err, int64_t n, double a, double b, double c,
                          double* out, double* dout /* d loss/d err, may be NULL */, uint32_t flags);

/* ---- a7: forward kinematics (get_3d_marker_coords, src/lib/misc.py:144-326) ----------
 * Skeleton tables come from acinoset_amd.kinematics.build_table (int/real blobs).
 * x, dx, ddx: (n, P); tau: (n,) or NULL; intermode 0 pos / 1 vel / 2 acc;
 * out: (n, L + 2*directions, 3); jac (n, L, 3, P) may be NULL.                        */
int acs_fk(acs_ctx* ctx, const int32_t* skel_ints, int64_t n_ints, const double* skel_reals,
           int64_t n_reals, const double* x, const double* dx, const double* ddx, const double* tau,
           int64_t n, int32_t intermode, int32_t directions, double* out, double* jac,
           uint32_t flags);

/* ---- a10-a13: FTE trajectory solve (src/core/fte.py:176-555) ------------------------
 * Unknowns: X ((n_frames + 2) x P, row f = frame f - 2; rows 0, 1 are the virtual frames
 * carrying the reference's free dx[1], ddx[1]) and tau, only when shutter_delay:
 * sd_mode 0 = 'const' (fte.py:236): tau (n_cams), tau[0] pinned to 0; sd_mode 1 =
 * 'variable' (fte.py:238): tau (n_frames x n_cams, frame major), tau[n][0] pinned to 0;
 * |tau| <= Ts (fte.py:304-318; a delay on the bound whose descent direction points out is
 * held for that step). meas (n_frames, n_cams, L, 2) pixels,
 * w (n_frames, n_cams, L) = 1/R where likelihood > thresh else 0 (fte.py:210-215),
 * qinv (P) = 1/Q_p = 1/_Q[p]^2 (fte.py:113-144, 217-218). intermode 0 pos / 1 vel / 2 acc
 * (shutter_delay requires vel/acc, fte.py:44-48). X and tau are in/out.                 */
typedef struct {
  int32_t max_iters;  /* LM iterations; default 200 */
  int32_t window;     /* reserved (0) */
  double ftol;        /* relative cost decrease (|F|); default 1e-12 */
  double xtol;        /* relative step; default 1e-12 */
  double gtol;        /* max |gradient|; default 1e-8 */
  double lambda0;     /* initial LM damping; default 1e-3 */
  double redesc_a, redesc_b, redesc_c;  /* redescending loss knots; 3, 10, 20 (fte.py:53-55) */
} acs_fte_opts;

typedef struct {
  int32_t status;      /* ACS_STATUS_* */
  int32_t iters;       /* LM iterations (accepted + rejected) */
  int32_t n_accepted;
  int32_t n_bad_pivots;
  double cost_before, cost_after, cost_meas, cost_model;
  double grad_max, lambda_final;
} acs_fte_report;

void acs_fte_default_opts(acs_fte_opts* o);
int acs_fte_solve(acs_ctx* ctx, const int32_t* skel_ints, int64_t n_ints, const double* skel_reals,
                  int64_t n_reals, const double* cams, int32_t n_cams, const double* meas,
                  const double* w, int32_t n_frames, int32_t shutter_delay, double Ts,
                  const double* qinv, int32_t sd_mode, int32_t intermode, double* X, double* tau,
                  const acs_fte_opts* opts, acs_fte_report* report, uint32_t flags);
/* objective (cost3 = [total, measurement, model]), gradient (nv = (n_frames+2)*P + the
 * number of delays: C const / n_frames*C variable, if shutter_delay) and the dense undamped GN normal matrix (nv x nv, may be NULL) at
 * (X, tau): the linearisation acs_fte_solve uses, exported for parity tests. Host ptrs. */
int acs_fte_eval(acs_ctx* ctx, const int32_t* skel_ints, int64_t n_ints, const double* skel_reals,
                 int64_t n_reals, const double* cams, int32_t n_cams, const double* meas,
                 const double* w, int32_t n_frames, int32_t shutter_delay, double Ts,
                 const double* qinv, int32_t sd_mode, int32_t intermode, const double* X,
                 const double* tau, double* cost3, double* grad, double* H, uint32_t flags);
/* Covariance of the FTE estimate at (X, tau): cov = the matching blocks of the inverse of the
 * undamped GN normal matrix H that acs_fte_eval returns at (X, tau), with the held delays
 * removed (camera 0, and a delay on a bound of [-Ts, Ts] whose descent direction points out:
 * constants, as in an LM step). The blocks are read off the solve's block cyclic reduction
 * tree (selected inversion); the dense inverse is never formed.
 * cov_x (n_frames + 2, P, P): per-row pose covariance, rows as X; cov_tau (C, C), may be NULL:
 * the delays' covariance, held rows and columns zero, all zeros without shutter_delay;
 * cov_marker (n_frames, L, 3, 3), may be NULL: J cov_x[k + 2] J^T per frame k and marker, J the
 * Jacobian of the marker position (acs_fk's jac) at X row k + 2 alone (no delay shift, no
 * direction markers). Arguments up to intermode exactly as acs_fte_eval; host pointers, or
 * ACS_DEVICE_PTRS for every array (then asynchronous unless `report` is given).
 * Non-positive pivots (H not positive definite) are counted in the report, never clamped away.
 * sd_mode 1 ('variable') returns ACS_E_INVALID: the per-frame delays are eliminated inside the
 * block build and their covariances need a back-substitution of their own (not built yet).
 * The factors and covariance blocks (about 4 BP^2 + 2 BP GR doubles per super-block) are
 * allocated on first use and kept in the context. Single GPU only.                          */
typedef struct {
  int32_t n_bad_pivots;  /* non-positive pivots met (0 for a positive definite H) */
  int32_t n_tau_free;    /* delays treated as unknowns */
  double var_min, var_max;  /* extreme diagonal entries of cov_x over rows 2.. */
} acs_fte_cov_report;
int acs_fte_covariance(acs_ctx* ctx, const int32_t* skel_ints, int64_t n_ints, const double* skel_reals,
                       int64_t n_reals, const double* cams, int32_t n_cams, const double* meas,
                       const double* w, int32_t n_frames, int32_t shutter_delay, double Ts,
                       const double* qinv, int32_t sd_mode, int32_t intermode, const double* X,
                       const double* tau, double* cov_x, double* cov_tau, double* cov_marker,
                       acs_fte_cov_report* report, uint32_t flags);
/* Test hook: the damped 3-frame super-blocks D_i (n_blk x BP x BP, BP = 3P padded to 16) of
 * acs_fte_solve's block-tridiagonal system at (X, tau) with damping lam, after `levels`
 * cyclic-reduction levels with every pending Schur term applied (0: as assembled; L > 0:
 * blocks 2^L m hold the D the next level factors). dims = {n_blk, BP, levels run}. Constant
 * or no shutter delay; host pointers, or ACS_DEVICE_PTRS for every array. */
int acs_fte_debug_blocks(acs_ctx* ctx, const int32_t* skel_ints, int64_t n_ints, const double* skel_reals,
                         int64_t n_reals, const double* cams, int32_t n_cams, const double* meas,
                         const double* w, int32_t n_frames, int32_t shutter_delay, double Ts,
                         const double* qinv, int32_t sd_mode, int32_t intermode, const double* X,
                         const double* tau, double lam, int32_t levels, double* D_out, int64_t* dims,
                         uint32_t flags);
/* Test hook, host only (no device memory, no launch): the kernels and grids acs_fte_solve
 * picks for n_frames frames of a P-parameter skeleton seen by n_cams cameras, computed by the
 * functions the solve itself dispatches with. n_cu > 0: the CU count to plan for (ctx may be
 * NULL); n_cu <= 0: the context's device.
 * head[8] = {n_blk, n_lev, BP, GR, Cg, assembly (512 / 1024: k_cr_assemble_build's threads; 0:
 * k_fte_assemble + k_cr_build, the variable-delay mode), k_fte_linearize instance (4 / 5), D
 * stored as upper tiles (0 / 1)}; levels[4 l ..] = {blocks eliminated, survivor workgroups,
 * nsplit, deep path (0 / 1)} of reduction level l < min(n_lev, max_levels). */
int acs_fte_debug_plan(acs_ctx* ctx, int32_t n_cu, int32_t n_frames, int32_t P, int32_t n_cams,
                       int32_t shutter_delay, int32_t sd_mode, int32_t* head, int32_t* levels,
                       int32_t max_levels);

/* ---- §8(e): frame-window distributed FTE (configs[3]) --------------------------------
 * One handle per rank (rank of world); every rank gets the full-size inputs of
 * acs_fte_solve. The super-blocks of 3 frames are split into `world` chains that share their
 * end blocks; a term belongs to the chain holding its lowest row. X is kept only on the
 * rank's own chain (its rows and both shared end blocks).
 * ONE all-reduce (sum) per LM step, of one DEVICE payload of payload_sizes[0] doubles: the
 * chain ends' reduced system (~ (world+1) (2 BP^2 + BP GR) doubles) followed by the pending
 * step's trial cost and step / state norms (4 doubles):
 *   init(P0) -> all-reduce(P0) -> round(P0, P1) -> all-reduce(P1) -> round(P1, P0) -> ...
 * round(in, out), on the summed `in`: every rank takes the same accept / reject decision on
 * the pending step (its cost is in `in`), solves the reduced system of `in`, back-substitutes
 * and steps its own chain, and writes into `out` the new step's trial cost and the reduced
 * system at the trial state, formed speculatively with the damping an acceptance gives
 * (linearised there already for the trial cost). After a rejection the round writes the
 * reduced system at the unchanged state with the new damping instead, and no step: a
 * rejection costs one extra round. Decisions are taken on the device; a round never waits
 * for the host. poll(h, r, &status) waits for round r (0-based) only and returns the LM
 * status after it (0 = running), so a host can queue round r + 1 first (a round after the
 * stop changes nothing). Then gather(p2) -> all-reduce(p2) -> scatter(p2) (the solution
 * rows, n_blocks x BP doubles = payload_sizes[1], once per solve) before result(). Every
 * rank runs the same reduced solve and takes the same decisions; the result equals
 * acs_fte_solve up to summation order.
 * shutter_delay with sd_mode 1 ('variable'): each frame's delays are interior unknowns of
 * the rank that owns the frame, eliminated in its rows and stepped by that rank; they are
 * gathered with the solution rows by p2, and result() returns tau as (n_frames, n_cams).  */
typedef struct acs_fte_dist acs_fte_dist;
int acs_fte_dist_create(acs_ctx* ctx, const int32_t* skel_ints, int64_t n_ints, const double* skel_reals,
                        int64_t n_reals, const double* cams, int32_t n_cams, const double* meas,
                        const double* w, int32_t n_frames, int32_t shutter_delay, double Ts,
                        const double* qinv, int32_t sd_mode, int32_t intermode, const double* X,
                        const double* tau, const acs_fte_opts* opts, int32_t rank, int32_t world,
                        acs_fte_dist** out, int64_t* payload_sizes, uint32_t flags);
int acs_fte_dist_init(acs_fte_dist* h, double* payload);
int acs_fte_dist_round(acs_fte_dist* h, const double* in, double* out);
int acs_fte_dist_poll(acs_fte_dist* h, int64_t round, int32_t* status);
int acs_fte_dist_gather(acs_fte_dist* h, double* p2);
int acs_fte_dist_scatter(acs_fte_dist* h, const double* p2);
int acs_fte_dist_result(acs_fte_dist* h, double* X, double* tau, acs_fte_report* report, uint32_t flags);
int acs_fte_dist_destroy(acs_fte_dist* h);
/* A new solve on the same handle from X ((n_frames + 2) x P) and tau (NULL = zeros), host
 * pointers or ACS_DEVICE_PTRS: the LM restarts as after acs_fte_dist_create (then
 * acs_fte_dist_init), with no allocation (the arena, payload sizes and captured round graphs
 * are kept), so a timed multi-GPU solve reuses one handle per rank. */
int acs_fte_dist_reset(acs_fte_dist* h, const double* X, const double* tau, uint32_t flags);

/* ---- next: triangulation ---------------------------------------------
 * With ACS_CAMS_STANDARD the views are undistorted as triangulate_points does
 * (src/lib/calib.py:53-62): cv::undistortPoints with its default criteria, exactly 5
 * fixed-point iterations and no convergence test; the DLT is the same.
 * acs_triangulate_pairs: triangulate_points_fisheye (src/lib/calib.py:120-129) for n
 * (view a, view b) pairs; uv_a/uv_b (n, 2) pixels, cam_a/cam_b (n) camera ids, out (n, 3).
 * acs_triangulate_dense: get_pairwise_3d_points_from_df (src/lib/utils.py:319-349) on the
 * dense (n_pts, n_cams) observation tensor: mean over adjacent pairs (c, c+1 mod C) seen
 * by both cameras; n_pairs_out (may be NULL) = number of pairs (0 -> NaN point).      */
int acs_triangulate_pairs(acs_ctx* ctx, const double* cams, int32_t n_cams, const double* uv_a,
                          const double* uv_b, const int32_t* cam_a, const int32_t* cam_b, int64_t n,
                          double* xyz_out, uint32_t flags);
int acs_triangulate_dense(acs_ctx* ctx, const double* cams, int32_t n_cams, const double* uv,
                          const uint8_t* mask, int64_t n_pts, double* xyz_out, int32_t* n_pairs_out,
                          uint32_t flags);

/* ---- §8(a) a6: bundle adjustment of points AND extrinsics ---------------------------
 * bundle_adjust_points_and_extrinsics (src/lib/sba.py:158-178): least_squares(trf,
 * loss='cauchy', f_scale=1) over cost_func_points_extrinsics (:142-146), x = [rvecs, tvecs,
 * points]. Schur-complement LM on the GPU; cams (n_cams <= 16 records) and pts are in/out
 * (rotation and translation of every camera refined, intrinsics kept). Observation list
 * form as acs_sba_points; a point may have at most 64 observations.                   */
typedef struct {
  int32_t max_iters;  /* LM iterations; default 500 */
  int32_t reserved;
  double f_scale;     /* Cauchy scale; default 1 (scipy default used at sba.py:168) */
  double ftol, xtol, gtol;  /* defaults 1e-12, 1e-12, 1e-8 */
  double lambda0;     /* default 1e-3 */
} acs_sba_ext_opts;

typedef struct {
  int32_t status, iters, n_accepted, n_bad_pivots;
  double cost_before, cost_after, grad_max, lambda_final;
} acs_sba_ext_report;

void acs_sba_ext_default_opts(acs_sba_ext_opts* o);
int acs_sba_extrinsics(acs_ctx* ctx, double* cams, int32_t n_cams, const double* uv,
                       const int32_t* pt_idx, const int32_t* cam_idx, int64_t n_obs, double* pts,
                       int64_t n_pts, const acs_sba_ext_opts* opts, double* resid_before,
                       double* resid_after, acs_sba_ext_report* report, uint32_t flags);
/* acs_sba_ext_plan (test hook, host only, no device): what acs_sba_extrinsics selects for n_pts
 * points whose largest observation count is K: the lane group G of a point (2..64), the points
 * per Schur block and the number of Schur blocks. ACS_E_INVALID for n_pts < 1 or K outside 1..64. */
int acs_sba_ext_plan(int64_t n_pts, int32_t K, int32_t* G, int32_t* chunk, int32_t* nchunk);

/* ---- bundle adjustment of extrinsics AND rigid calibration-board poses ------------------
 * One rigid pose per board image instead of one free 3-D point per corner: the known board
 * geometry fixes the metric scale, and the gauge is the 6-DoF rigid motion only.
 *   cameras c = 0..n_cams-1: fisheye records (ACS_CAM_STRIDE), intrinsics kept, 1..16
 *   boards b = 0..n_boards-1: pose (R_b, t_b) from board to world coordinates, as 12 doubles
 *     (R row-major, then t); in/out
 *   obj_pts (n_corners, 3): the target's points p_j in board coordinates (any rigid target,
 *     e.g. create_board_object_pts), 3 <= n_corners <= 256
 *   world point X_bj = R_b p_j + t_b
 *   uv (n_boards, n_cams, n_corners, 2) pixels and mask (n_boards, n_cams) uint8: a camera sees
 *     a board image with all its corners or not at all
 *   residual r = project(R_c X_bj + t_c) - uv; cost F = 1/2 f^2 sum log1p(r^2 / f^2); weights
 *     w = 1 / (1 + z), wh = max((1 - z) w^2, 0.1 w), z = r^2 / f^2 (those of acs_sba_extrinsics)
 *   left perturbations R <- exp([dw]x) R, t <- t + dt for cameras and boards;
 *     J_cam = J_Y [-[R_c X]x | I], J_pt = J_Y R_c, J_brd = J_pt [-[R_b p_j]x | I]
 *   per seen view: U_bc = sum wh J_cam^T J_cam, W_bc = sum wh J_cam^T J_brd (6 x 6), g_c;
 *     per board: V_b = sum wh J_brd^T J_brd (6 x 6), g_b
 *   LM of acs_sba_extrinsics with the boards eliminated: M_b = (V_b + lam diag V_b + 1e-300 I)^-1,
 *     S = sum U + lam D - sum W M W^T, b = -g_c + sum W M g_b, db = -M_b (g_b + sum W^T dc);
 *     accept iff the cost falls (lam /= 10, floor 1e-7), else lam *= 10; stops, options and
 *     report as acs_sba_extrinsics (|d|^2 = sum dc^2 + sum db^2, |x|^2 = sum |t_c|^2 + sum |t_b|^2)
 *   a board whose damped V_b is not positive definite (no view, a NaN, a pivot not > 0) takes
 *     no step in that iteration; a board with one view is legal. The rigid gauge is left free.
 * resid_before / resid_after (either may be NULL): the seen views in (board, camera, corner, row)
 * order, 2 n_corners doubles per seen view. Host pointers, or ACS_DEVICE_PTRS for every array.
 * ACS_E_INVALID before anything is staged: f_scale <= 0, n_cams outside 1..16, n_corners outside
 * 3..256, n_boards < 1, ACS_CAMS_STANDARD.
 * acs_sba_boards_chunk: boards per block of the Schur complement for n_cams cameras (test hook). */
int acs_sba_boards(acs_ctx* ctx, double* cams, int32_t n_cams, const double* obj_pts,
                   int32_t n_corners, const double* uv, const uint8_t* mask, int32_t n_boards,
                   double* board_poses, const acs_sba_ext_opts* opts, double* resid_before,
                   double* resid_after, acs_sba_ext_report* report, uint32_t flags);
int32_t acs_sba_boards_chunk(int32_t n_cams);

/* ---- rigid boards with free (hand-labelled) points in the same solve --------------------
 * Everything of acs_sba_boards stays as it is: fisheye cameras c < C <= 16 with fixed intrinsics,
 * boards b < B with pose (R_b, t_b), object points p_j, uv (B, C, nc, 2), mask (B, C). Added:
 *   free points X_p, p = 0..n_pts-1, stored densely like the boards and the manual-points file:
 *     pt_uv (n_pts, n_cams, 2) pixels, pt_mask (n_pts, n_cams) uint8; a camera sees a point at
 *     most once (in acs_sba_extrinsics' terms slot = camera, K = C). pts (n_pts, 3) is in/out.
 *   the same robust cost and weights for every residual (Cauchy with f_scale; Triggs
 *     wh = max((1 - z) w^2, 0.1 w)): F = F_boards + F_points; U and g_c of a camera sum over its
 *     board views and its point observations
 *   one LM, those of acs_sba_boards and acs_sba_extrinsics joined: Marquardt damping on every
 *     diagonal, M_b as in acs_sba_boards, M_p = (V_p + lam diag V_p + 1e-300 I)^-1 as in
 *     acs_sba_extrinsics,
 *       S = sum U + lam D - sum_b W M_b W^T - sum_p W M_p W^T,
 *       b = -g_c + sum_b W M_b g_b + sum_p W M_p g_p,
 *     db and dX by back-substitution, gmax = max(|g_c|, |g_b|, |g_p|),
 *     |d|^2 = sum dc^2 + sum db^2 + sum dX^2, |x|^2 = sum |t_c|^2 + sum |t_b|^2 + sum |X_p|^2;
 *     accept / reject, the lambda schedule and its floor 1e-7, stops, options, status codes and
 *     report unchanged
 *   a point without an observation takes no step and contributes nothing; a board without a view
 *     behaves as in acs_sba_boards. The 6-DoF rigid gauge stays free (resolved by the damping floor).
 * resid_before / resid_after (either may be NULL): the board part exactly as acs_sba_boards writes
 * it, then the seen (point, camera) pairs in (point, camera, row) order, 2 doubles each. Host
 * pointers, or ACS_DEVICE_PTRS for every array. n_pts = 0 is allowed (the point arrays may be NULL)
 * and runs the board kernels alone: the bits of acs_sba_boards. A second call of the same size
 * allocates nothing.
 * ACS_E_INVALID before anything is staged or allocated: the refusals of acs_sba_boards, n_pts < 0
 * (or n_pts n_cams >= 2^31), a null point array with n_pts > 0, ACS_CAMS_STANDARD.
 * Not here: covariances of the mixed problem (acs_sba_boards_covariance describes the boards-only
 * problem), separate noise scales for clicks and corners, the standard camera model, a
 * distributed form. */
int acs_sba_boards_points(acs_ctx* ctx, double* cams, int32_t n_cams, const double* obj_pts,
                          int32_t n_corners, const double* uv, const uint8_t* mask, int32_t n_boards,
                          double* board_poses, const double* pt_uv, const uint8_t* pt_mask,
                          int32_t n_pts, double* pts, const acs_sba_ext_opts* opts,
                          double* resid_before, double* resid_after, acs_sba_ext_report* report,
                          uint32_t flags);

/* ---- camera-pose and joint point covariances of the points + extrinsics SBA -----------
 * Evaluated at the cameras (fisheye records, n_cams <= 16) and points passed in; nothing is
 * solved. Observation list as acs_sba_extrinsics.
 * Linearisation: the solver's own. Per camera (dw, dt) with R <- exp([dw]x) R, t <- t + dt, so
 * J_cam = J_Y [-[R X]x | I], J_pt = J_Y R; Triggs weights wh = max((1 - z) w^2, 0.1 w),
 * w = 1 / (1 + z), z = r^2 / f_scale^2.
 * Points: status by the rule of acs_sba_points_covariance on the point's own V = sum wh J_pt^T
 * J_pt (ACS_COV_NOOBS without a usable observation, ACS_COV_DEGENERATE when an LDL^T pivot fails
 * d > 1e-9 max(V00, V11, V22), else ACS_COV_OK). A point that is not OK is left out entirely
 * (its U, W and V terms): a single-view point carries no information about the cameras.
 * Reduced system: S = sum U - sum_OK W V^-1 W^T (6C x 6C, undamped, symmetrised).
 * Gauge generators G (6C x 7), per camera c: rotation theta: dw = -R_c theta, dt = 0;
 * translation tau: dw = 0, dt = -R_c tau; scale: dw = 0, dt = t_c. S G = 0.
 * ACS_GAUGE_FREE (inner constraints over the camera parameters, minimum trace): with Q an
 * orthonormal basis of span G and mu = max diag S,
 *   cov = sigma_px^2 [(S + mu Q Q^T)^-1 - Q Q^T / mu]   (= sigma_px^2 pinv(S)).
 * ACS_GAUGE_ANCHOR: the pose of camera anchor_cam (a) and the distance between the centres of
 * a and scale_cam (b) are held. Cm (7 x 6C) = six identity rows on camera a and the row
 * e^T dc_b/d(dw_b, dt_b), c = -R^T t, dc/d(dw, dt) = [-R^T [t]x | -R^T], e the unit baseline;
 *   cov = P cov_free P^T,  P = I - G (Cm G)^-1 Cm,
 * camera a's rows and columns exact zeros.
 * Degenerate problem: with Ah = S + mu Q Q^T scaled to unit diagonal, status is
 * ACS_EXT_COV_DEGENERATE when a diagonal entry is not > 0, a pivot of the unpivoted LDL^T of Ah
 * in natural order fails d > 1e-9 (a NaN fails), or G has rank < 7 (one camera, or all centres
 * in one place). Then every covariance is NaN. min_pivot = the smallest pivot up to and
 * including the first that fails.
 * Points (OK, B_i the 6C x 3 stack of the point's W blocks):
 *   cov_i = sigma_px^2 V_i^-1 + V_i^-1 B_i^T cov_cc B_i V_i^-1,  NaN for the others.
 * sigma_hat_px^2 = sum w r^2 / dof, dof = m - 3 n_ok - (6C - 7) over the residuals of the OK
 * points (NaN when dof <= 0): reported, never applied.
 * cov_cams (6C, 6C) with camera c's (dw, dt) at rows 6c..6c+5 (rad, m); cov_pts (n_pts, 3, 3)
 * and pt_status (n_pts, int32) may be NULL; every matrix is exactly symmetric. The call waits
 * for the stream. Invalid arguments (f_scale or sigma_px <= 0, n_cams outside 1..16, for the
 * anchor gauge with n_cams >= 2: anchor_cam == scale_cam, either out of range, or coincident
 * centres; ACS_CAMS_STANDARD) return ACS_E_INVALID before anything is staged.             */
#define ACS_GAUGE_FREE 0
#define ACS_GAUGE_ANCHOR 1
#define ACS_EXT_COV_OK 0
#define ACS_EXT_COV_DEGENERATE 1
typedef struct {
  int32_t gauge;       /* ACS_GAUGE_*; default ACS_GAUGE_ANCHOR */
  int32_t anchor_cam;  /* default 0 */
  int32_t scale_cam;   /* default 1 */
  int32_t reserved;
  double f_scale;      /* the solve's Cauchy scale; default 1 (acs_sba_ext_default_opts) */
  double sigma_px;     /* assumed pixel noise; default 1 */
} acs_sba_ext_cov_opts;
typedef struct {
  int32_t status;      /* ACS_EXT_COV_* */
  int32_t reserved;
  int64_t n_points, n_ok, n_noobs, n_degenerate;
  int64_t dof;
  double min_pivot;
  double sigma_hat_px;
  double rot_sd_max;    /* largest rotation sd over the cameras (rad) */
  double trans_sd_max;  /* largest translation sd over the cameras (m) */
} acs_sba_ext_cov_report;
void acs_sba_ext_cov_default_opts(acs_sba_ext_cov_opts* o);
int acs_sba_extrinsics_covariance(acs_ctx* ctx, const double* cams, int32_t n_cams, const double* uv,
                                  const int32_t* pt_idx, const int32_t* cam_idx, int64_t n_obs,
                                  const double* pts, int64_t n_pts, const acs_sba_ext_cov_opts* opts,
                                  double* cov_cams, double* cov_pts, int32_t* pt_status,
                                  acs_sba_ext_cov_report* report, uint32_t flags);

/* ---- camera and board pose covariances of the rigid-board SBA --------------------------
 * Evaluated at the cameras and board poses passed in; nothing is solved.
 * Problem and linearisation: those of acs_sba_boards. Fisheye records, 1 <= n_cams (C) <= 16,
 * 3 <= n_corners (nc) <= 256, n_boards (B) >= 1, uv (B, C, nc, 2), mask (B, C), board_poses
 * (B, 12). Left perturbations R <- exp([dw]x) R, t <- t + dt for cameras and boards;
 * J_cam = J_Y [-[R_c X]x | I], J_pt = J_Y R_c, J_brd = J_pt [-[R_b p_j]x | I]; Triggs weights
 * wh = max((1 - z) w^2, 0.1 w), w = 1 / (1 + z), z = r^2 / f_scale^2. Per seen view U_bc and
 * W_bc (6 x 6); per board V_b = sum_views sum wh J_brd^T J_brd. All undamped.
 * Board status (int32 per board, ACS_COV_*): ACS_COV_NOOBS without a view; ACS_COV_DEGENERATE
 * when an entry of diag V_b is not > 0, or a pivot of the unpivoted LDL^T of V_b scaled to unit
 * diagonal fails d > 1e-9 (a NaN fails; a collinear target is an example; the scaling matters
 * because V_b mixes rad^-2 and m^-2); ACS_COV_OK otherwise (a board with one view of a planar
 * target is OK). A board that is not OK is left out entirely (its U, W and V terms), so S G = 0
 * stays exact.
 * Reduced system: S = sum_OK U_bc - sum_OK W_b V_b^-1 W_b^T (6C x 6C, symmetrised), W_b the
 * 6C x 6 stack of the board's view blocks.
 * Gauge generators G (6C x 6), per camera c: rotation theta: dw_c = -R_c theta, dt_c = 0;
 * translation tau: dw_c = 0, dt_c = -R_c tau (the boards move with dw_b = theta,
 * dt_b = -[t_b]x theta + tau). S G = 0.
 * ACS_GAUGE_FREE: with Q = orth(G) and mu = max diag S,
 *   cov_cc = sigma_px^2 [(S + mu Q Q^T)^-1 - Q Q^T / mu]   (= sigma_px^2 pinv(S)).
 * ACS_GAUGE_ANCHOR (the default): the pose of camera anchor_cam (a) is held. Cm (6 x 6C) is the
 * identity on camera a,
 *   cov_cc = P cov_free P^T,  P = I - G (Cm G)^-1 Cm,
 * camera a's rows and columns exact zeros. scale_cam is ignored: the board fixes the scale.
 * Problem status: ACS_EXT_COV_DEGENERATE when, with Ah = S + mu Q Q^T scaled to unit diagonal, a
 * diagonal entry is not > 0 (a camera seen by no OK board ends here or at the next test), a
 * pivot of the unpivoted LDL^T of Ah in natural order fails d > 1e-9, or G has rank < 6. Then
 * every covariance is NaN. min_pivot as in acs_sba_extrinsics_covariance.
 * n_cams = 1 is decided before S is formed: the camera is pure gauge, so cov_cams is exact
 * zeros in both gauges, the status is OK, min_pivot is NaN (nothing is factored) and the boards
 * get sigma_px^2 V_b^-1.
 * Boards (OK boards; NaN for the others):
 *   cov_b = sigma_px^2 V_b^-1 + V_b^-1 W_b^T cov_cc W_b V_b^-1   (6 x 6, (dw_b, dt_b), rad and m).
 * sigma_hat_px^2 = sum w r^2 / dof over the residuals of the OK boards' views,
 * dof = m - 6 n_ok - (6C - 6) (NaN when dof <= 0): reported, never applied.
 * cov_cams (6C, 6C); cov_boards (B, 6, 6) and board_status (B) may be NULL; every matrix is
 * exactly symmetric. Host pointers, or ACS_DEVICE_PTRS for every array. The call waits for the
 * stream. ACS_E_INVALID before anything is staged: f_scale or sigma_px <= 0, n_cams outside
 * 1..16, n_corners outside 3..256, n_boards < 1, anchor_cam out of range in the anchor gauge, an
 * unknown gauge, ACS_CAMS_STANDARD.                                                          */
typedef struct {
  int32_t status, reserved;                 /* ACS_EXT_COV_* */
  int64_t n_boards, n_ok, n_noobs, n_degenerate, dof;
  double min_pivot, sigma_hat_px;
  double rot_sd_max, trans_sd_max;              /* cameras (rad, m) */
  double board_rot_sd_max, board_trans_sd_max;  /* OK boards (rad, m) */
} acs_sba_boards_cov_report;
int acs_sba_boards_covariance(acs_ctx* ctx, const double* cams, int32_t n_cams, const double* obj_pts,
                              int32_t n_corners, const double* uv, const uint8_t* mask,
                              int32_t n_boards, const double* board_poses,
                              const acs_sba_ext_cov_opts* opts /* scale_cam ignored */,
                              double* cov_cams /* 6C x 6C */, double* cov_boards /* B x 6 x 6, may be NULL */,
                              int32_t* board_status /* may be NULL */, acs_sba_boards_cov_report* report,
                              uint32_t flags);

/* ---- §8(e): points + extrinsics SBA over ranks -------------------------------------
 * Each rank passes its own points and their observations (point indices local to the
 * rank); cameras are replicated. ONE all-reduce per LM step:
 *   init(P) -> all-reduce(P, sum); then for k = 0, 1, ...:
 *     round(P, P') -> all-reduce(P', sum); poll(k - 1, &status) until status != 0
 * P = [p1 | p3] (payload_sizes[0] doubles): p1 = the reduced camera system
 * [S (6C x 6C) | b | diag U | g_c] + one |g| slot per rank, p3 = (cost, |dX|^2, |X|^2) of the
 * rank's points at the pending trial. A round decides on the pending trial from p3 (the
 * rule of acs_sba_extrinsics), steps from p1, and forms the next p1 at the new trial state
 * with the damping an acceptance sets (a rejected trial costs one extra round that
 * re-forms the system). poll() waits only for that round (pinned status ring of 4).
 * Device buffers. result() returns the (replicated) cameras and this rank's points.    */
typedef struct acs_sba_ext_dist acs_sba_ext_dist;
int acs_sba_ext_dist_create(acs_ctx* ctx, const double* cams, int32_t n_cams, const double* uv,
                            const int32_t* pt_idx, const int32_t* cam_idx, int64_t n_obs,
                            const double* pts, int64_t n_pts, const acs_sba_ext_opts* opts,
                            int32_t rank, int32_t world, acs_sba_ext_dist** out,
                            int64_t* payload_sizes, uint32_t flags);
int acs_sba_ext_dist_init(acs_sba_ext_dist* h, double* payload);
int acs_sba_ext_dist_round(acs_sba_ext_dist* h, const double* in, double* out);
int acs_sba_ext_dist_poll(acs_sba_ext_dist* h, int64_t round, int32_t* status);
int acs_sba_ext_dist_result(acs_sba_ext_dist* h, double* cams, double* pts, acs_sba_ext_report* report,
                            uint32_t flags);
int acs_sba_ext_dist_destroy(acs_sba_ext_dist* h);

/* ---- §8(f)-2: EKF + RTS smoother (core.ekf, src/core/ekf.py:26-347) -----------------
 * n_seq independent sequences of n_frames frames (one workgroup each). State n = 3P:
 * [x, dx, ddx]. meas (n_seq, n_frames, n_cams, L, 2) pixels (NaN = missing), likelihood
 * (n_seq, n_frames, n_cams, L); R = diag(s^2) with s = r_std_base[cam] (the reference's
 * 2 cov_c / min cov, :244-248) or max_pixel_err below `thresh`. Q, P0: n x n; s0: (n_seq, n).
 * ref_numerics (the measurement-model mode): 1 reproduces the reference's float32
 * prediction cast and float32 Jacobian perturbation (:79, :81-96; eps = the forward-
 * difference step, 1e-3); 0 is the same forward-difference H in float64;
 * ACS_EKF_ANALYTIC_H (2) replaces the P+1 forward-difference poses by the analytic H
 * (SURVEY §8(f)2): one FK with its Jacobian d pos / d x, times the projection's 2 x 3
 * Jacobian, in float64 (eps unused).
 * Outputs (n_seq, n_frames, n) x_pred (may be NULL), x_est, x_smooth; (.., n, n) P_est,
 * P_smooth (may be NULL); outliers (n_seq) = the reference's 3-sigma count (may be NULL). */
int acs_ekf_run(acs_ctx* ctx, const int32_t* skel_ints, int64_t n_ints, const double* skel_reals,
                int64_t n_reals, const double* cams, int32_t n_cams, const double* meas,
                const double* likelihood, int32_t n_seq, int32_t n_frames, double fps, double thresh,
                double max_pixel_err, const double* r_std_base, const double* Q, const double* P0,
                const double* s0, int32_t ref_numerics, double eps, double* x_pred, double* x_est,
                double* x_smooth, double* P_est, double* P_smooth, int64_t* outliers, uint32_t flags);
/* Singular solves (I + A P_xx in an update, P_pred in a gain) of the last EKF enqueue on this
 * context (acs_ekf_run or acs_sba_ekf_pipeline); waits for the context stream. A call that
 * synchronises anyway (host arrays, or an outlier report) already fails on them; a
 * device-pointer call without outliers does not check, and this reads the count afterwards. */
int acs_ekf_singular_count(acs_ctx* ctx, int32_t* count);
/* Test hook, host only (no context, no device memory, no launch): the kernels acs_ekf_run
 * picks for a skeleton table of P parameters, n_joints joints, n_nodes nodes and L markers
 * seen by n_cams cameras over n_frames frames, with or without P_smooth, from the function the
 * run itself dispatches with (the table's joint and node counts size its place in the filter's
 * LDS). plan[6] = {filter (0: k_ekf_filter, 1: k_ekf_filter_w1), waves of the filter,
 * gains (0: none, 1: k_ekf_gain_w, 2: k_ekf_gain, 3..6: k_ekf_gain_t<NB> + k_ekf_gain_piv),
 * smoother (0: k_ekf_smooth, 1: k_ekf_smooth_xs<18,8>, 2: k_ekf_smooth_xs<87,2>,
 * 3: k_ekf_smooth_x), npad (3P padded to 16), filter LDS bytes}. ACS_E_INVALID where the run
 * refuses the shape: P outside 3..32, n_cams outside 1..64, a table out of range, or a filter
 * that needs more than 160 KB of LDS. */
int acs_ekf_debug_plan(int32_t P, int32_t n_joints, int32_t n_nodes, int32_t n_cams, int32_t L,
                       int32_t n_frames, int32_t with_p_smooth, int32_t* plan);

/* ---- configs[4]: SBA + EKF fused on one observation tensor ------------------------------
 * core.sba (src/core/sba.py:27-70) and core.ekf (src/core/ekf.py:26-298) of the same
 * DLC observations as one device-resident enqueue: pairwise triangulation and points-only
 * SBA of every (sequence, frame, marker) with likelihood > thresh (src/core/sba.py:41;
 * points no adjacent camera pair saw are left out, as the reference's inner merge does,
 * src/lib/sba.py:299), then per sequence the initial state of src/core/ekf.py:121-157 (nose /
 * lure line fits; init->from_sba = 1: on the SBA points, 0: on the triangulated points as
 * core.ekf does) and the EKF + RTS smoother of acs_ekf_run on the EKF model's markers.
 * meas (n_seq, n_frames, n_cams, n_markers, 2), likelihood (n_seq, n_frames, n_cams,
 * n_markers); ekf_markers (L of the skeleton table): observation marker index of every EKF
 * model marker. skel_ints / skel_reals / ekf_markers / sba_opts / init are HOST descriptors
 * whatever `flags` says; the arrays follow `flags`.
 * Outputs: pts_out (n_seq, n_frames, n_markers, 3) SBA points (NaN where not triangulated),
 * x_est, x_smooth (n_seq, n_frames, 3P); outliers (n_seq, may be NULL); sba_report (may be
 * NULL; waits for the SBA). Without ACS_DEVICE_PTRS (or with outliers) the call waits and
 * fails if a sequence's nose was seen in fewer than two frames.                        */
typedef struct {
  int32_t nose;      /* observation marker index of the nose */
  int32_t lure;      /* ... of the lure, -1 if the model has none */
  int32_t x0, y0, psi0;  /* pose parameter indices of x_0, y_0, psi_0 */
  int32_t xl, yl;    /* ... of x_l, y_l (-1: no lure states) */
  int32_t from_sba;  /* 1: line fits on the SBA points, 0: on the triangulated points */
} acs_ekf_init_spec;
int acs_sba_ekf_pipeline(acs_ctx* ctx, const int32_t* skel_ints, int64_t n_ints, const double* skel_reals,
                         int64_t n_reals, const double* cams, int32_t n_cams, const double* meas,
                         const double* likelihood, int32_t n_seq, int32_t n_frames, int32_t n_markers,
                         const int32_t* ekf_markers, double fps, double thresh, double max_pixel_err,
                         const double* r_std_base, const double* Q, const double* P0, const acs_sba_opts* sba_opts,
                         const acs_ekf_init_spec* init, int32_t ref_numerics, double eps, double* pts_out,
                         double* x_est, double* x_smooth, int64_t* outliers, acs_report* sba_report,
                         uint32_t flags);

#ifdef __cplusplus
}
#endif
#endif /* ACINOSET_HIP_H */
