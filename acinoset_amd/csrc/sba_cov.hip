// sba_cov.hip — per-point position covariance of the points-only SBA on gfx950.
//
// Definition (include/acinoset_hip.h): for point i with observations o, residuals
// r_od in pixels at the points passed in, z = r^2 / f_scale^2 and w = 1 / (1 + z),
//   H_i = sum_o sum_d wh_od J_od^T J_od,  wh = max((1 - z) w^2, 0.1 w)
// is the Triggs-weighted Gauss-Newton matrix k_sba_lm (sba.hip) factorises on every pass, here
// undamped; cov_i = sigma_px^2 H_i^-1. The inverse, the pivot rule that makes a point degenerate
// and the status are ldl3_inverse and cov_point_status (common.hpp), shared with the extrinsics
// covariance. Nothing is solved: one evaluation and one 3x3 inverse per point.
//
// Mapping: one point = one aligned group of G = clamp(nextpow2(K), 2, 64) lanes over the
// (n_pts, K) slot tensor of k_sba_lm, slots strided over the lanes (slot = lane, lane + G, ...),
// so one family covers K = 1..256. The camera records are staged in LDS. Each lane projects its
// slots with the general model_project<MODEL, true> (one pass, no iteration chain to shorten)
// and accumulates the 6 entries of H, sum w r^2 and its residual count; group_sum<G> of the 8
// values sums in a fixed order whatever the group's place in the wave. Empty and out-of-range
// slots are skipped by a branch: the grid is throughput-bound, and a null record would be
// projected in full. Lane 0 of the group alone inverts and writes the 72-byte record, upper
// triangle mirrored.
#include "common.hpp"

template <int G, bool CAMID, int MODEL>
__global__ __launch_bounds__(256) void k_sba_cov(const double2* __restrict__ uv, const uint8_t* __restrict__ mask,
                                                 int64_t n_pts, const double* __restrict__ pts,
                                                 const double* __restrict__ cams, int K, int C,
                                                 const uint8_t* __restrict__ camid, double if2, double s2,
                                                 double* __restrict__ cov, int32_t* __restrict__ status,
                                                 double* __restrict__ wr2, int32_t* __restrict__ nres) {
  constexpr int CS = CamRec<MODEL>::stride;
  extern __shared__ double s_cam[];
  for (int i = threadIdx.x; i < C * CS; i += blockDim.x) s_cam[i] = cams[i];
  __syncthreads();
  const int lane = threadIdx.x & (G - 1);
  const int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
  if (p >= n_pts) return;  // whole group leaves together
  const double x0 = pts[3 * p], x1 = pts[3 * p + 1], x2 = pts[3 * p + 2];
  // H (packed upper: 00 01 02 11 12 22), sum w r^2, number of scalar residuals
  double v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = 0.0;
  for (int slot = lane; slot < K; slot += G) {
    const int64_t o = p * K + slot;
    if (!mask[o]) continue;
    const int cam = CAMID ? camid[o] : slot;
    if (cam >= C) continue;
    const double2 q = uv[o];
    ProjOut po;
    model_project<MODEL, true>(s_cam + cam * CS, x0, x1, x2, po);
    const double r[2] = {po.u - q.x, po.v - q.y};
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const double rr = r[d] * r[d];
      const double z = rr * if2;
      const double w = rcp_nr(1.0 + z);
      const double wh = fmax((1.0 - z) * w * w, 0.1 * w);
      const double j0 = po.J[3 * d], j1 = po.J[3 * d + 1], j2 = po.J[3 * d + 2];
      const double hj0 = wh * j0, hj1 = wh * j1, hj2 = wh * j2;
      v[0] += hj0 * j0;
      v[1] += hj0 * j1;
      v[2] += hj0 * j2;
      v[3] += hj1 * j1;
      v[4] += hj1 * j2;
      v[5] += hj2 * j2;
      v[6] += w * rr;
    }
    v[7] += 2.0;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = group_sum<G>(v[i]);
  if (lane != 0) return;  // the inverse and the record are lane 0's alone
  double ci[6];
  const bool ok = ldl3_inverse(v, [](double d) { return rcp_nr(d); }, ci);
  const int st = cov_point_status(v[7], ok);
  const double nan = __builtin_nan("");
  const bool good = st == ACS_COV_OK;
  double* c = cov + 9 * p;
  const double e00 = good ? s2 * ci[0] : nan, e01 = good ? s2 * ci[1] : nan, e02 = good ? s2 * ci[2] : nan;
  const double e11 = good ? s2 * ci[3] : nan, e12 = good ? s2 * ci[4] : nan, e22 = good ? s2 * ci[5] : nan;
  c[0] = e00;
  c[1] = e01;
  c[2] = e02;
  c[3] = e01;
  c[4] = e11;
  c[5] = e12;
  c[6] = e02;
  c[7] = e12;
  c[8] = e22;
  if (status) status[p] = st;
  // the a-posteriori scale's per-point terms feed k_sba_cov_report only
  if (wr2) {
    wr2[p] = v[6];
    nres[p] = (int32_t)v[7];
  }
}

// Deterministic single-block reduction (fixed-order tree, no atomics) of the per-point outputs
// into an acs_sba_cov_report.
__global__ __launch_bounds__(256) void k_sba_cov_report(const double* __restrict__ cov,
                                                        const int32_t* __restrict__ status,
                                                        const double* __restrict__ wr2,
                                                        const int32_t* __restrict__ nres, int64_t n,
                                                        acs_sba_cov_report* __restrict__ rep) {
  __shared__ double s_d[256][3];     // var_min, var_max, sum w r^2
  __shared__ long long s_i[256][4];  // n_ok, n_noobs, n_degenerate, m
  const int t = threadIdx.x;
  double vmin = __builtin_inf(), vmax = -__builtin_inf(), sw = 0.0;
  long long cnt[3] = {0, 0, 0}, m = 0;
  for (int64_t i = t; i < n; i += 256) {
    const int s = status[i];
    if (s >= 0 && s < 3) cnt[s]++;
    if (s != ACS_COV_OK) continue;
    for (int k = 0; k < 9; k += 4) {
      vmin = fmin(vmin, cov[9 * i + k]);
      vmax = fmax(vmax, cov[9 * i + k]);
    }
    sw += wr2[i];
    m += nres[i];
  }
  s_d[t][0] = vmin;
  s_d[t][1] = vmax;
  s_d[t][2] = sw;
  for (int k = 0; k < 3; ++k) s_i[t][k] = cnt[k];
  s_i[t][3] = m;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) {
      s_d[t][0] = fmin(s_d[t][0], s_d[t + h][0]);
      s_d[t][1] = fmax(s_d[t][1], s_d[t + h][1]);
      s_d[t][2] += s_d[t + h][2];
      for (int k = 0; k < 4; ++k) s_i[t][k] += s_i[t + h][k];
    }
    __syncthreads();
  }
  if (t == 0) {
    const double nan = __builtin_nan("");
    const long long n_ok = s_i[0][0], dof = s_i[0][3] - 3 * n_ok;
    rep->n_points = n;
    rep->n_ok = n_ok;
    rep->n_noobs = s_i[0][1];
    rep->n_degenerate = s_i[0][2];
    rep->var_min = n_ok > 0 ? s_d[0][0] : nan;
    rep->var_max = n_ok > 0 ? s_d[0][1] : nan;
    rep->sigma_hat_px = dof > 0 ? sqrt(s_d[0][2] / (double)dof) : nan;
  }
}

template <bool CAMID, int MODEL>
static void launch_cov_g(acs_ctx* ctx, int G, int blocks, int block, const double2* uv, const uint8_t* mask,
                         int64_t n_pts, const double* pts, const double* cams, int K, int C, const uint8_t* camid,
                         double if2, double s2, double* cov, int32_t* status, double* wr2, int32_t* nres) {
  const size_t lds = sizeof(double) * CamRec<MODEL>::stride * C;
#define COV_G(g)                                                                                                 \
  hipLaunchKernelGGL((k_sba_cov<g, CAMID, MODEL>), dim3(blocks), dim3(block), lds, ctx->stream, uv, mask, n_pts, \
                     pts, cams, K, C, camid, if2, s2, cov, status, wr2, nres)
  ACS_G_SWITCH(G, COV_G)
#undef COV_G
}

// The covariance kernel (and, with a report, its reduction) over an (n_pts, K) slot tensor
// already on the device. dstatus may be null without a report.
static int run_cov(acs_ctx* ctx, int model, const double* dcams, int C, int K, const double2* duv,
                   const uint8_t* dmask, const uint8_t* dcamid, int64_t n_pts, const double* dpts, double f_scale,
                   double sigma_px, double* dcov, int32_t* dstatus, acs_sba_cov_report* report) {
  double* wr2 = nullptr;
  int32_t* nres = nullptr;
  acs_sba_cov_report* drep = nullptr;
  if (report) {
    wr2 = (double*)acs_ws(ctx, WS_PERPT_F0, sizeof(double) * n_pts);
    nres = (int32_t*)acs_ws(ctx, WS_PERPT_I, sizeof(int32_t) * n_pts);
    drep = (acs_sba_cov_report*)acs_ws(ctx, WS_REPORT, sizeof(acs_sba_cov_report));
    if (!dstatus) dstatus = (int32_t*)acs_ws(ctx, WS_TMP5, sizeof(int32_t) * n_pts);
    if (!wr2 || !nres || !drep || !dstatus) return ACS_E_NOMEM;
  }
  int G = 2;
  while (G < K && G < 64) G <<= 1;
  const int64_t threads = n_pts * G;
  ACS_CHECK(ctx, threads / 64 < (int64_t)INT32_MAX, "n_pts=%lld is too large for one launch (%d lanes per point)",
            (long long)n_pts, G);
  int block = 256;
  if (threads < (int64_t)256 * 2 * ctx->n_cu) block = 64;  // small problem: spread over more CUs
  const int blocks = acs_grid(threads, block);
  const double if2 = 1.0 / (f_scale * f_scale), s2 = sigma_px * sigma_px;
#define ACS_COV_ARGS ctx, G, blocks, block, duv, dmask, n_pts, dpts, dcams, K, C, dcamid, if2, s2, dcov, dstatus, wr2, nres
  if (model == ACS_MODEL_STANDARD)
    dcamid ? launch_cov_g<true, ACS_MODEL_STANDARD>(ACS_COV_ARGS) : launch_cov_g<false, ACS_MODEL_STANDARD>(ACS_COV_ARGS);
  else
    dcamid ? launch_cov_g<true, ACS_MODEL_FISHEYE>(ACS_COV_ARGS) : launch_cov_g<false, ACS_MODEL_FISHEYE>(ACS_COV_ARGS);
#undef ACS_COV_ARGS
  ACS_HIP(ctx, hipGetLastError());
  if (report) {
    hipLaunchKernelGGL(k_sba_cov_report, dim3(1), dim3(256), 0, ctx->stream, (const double*)dcov,
                       (const int32_t*)dstatus, (const double*)wr2, (const int32_t*)nres, n_pts, drep);
    ACS_HIP(ctx, hipGetLastError());
    ACS_HIP(ctx, hipMemcpyAsync(report, drep, sizeof(*report), hipMemcpyDeviceToHost, ctx->stream));
  }
  return ACS_OK;
}

// the tail both entry points share: results to the host, then wait where the call is synchronous
static int finish_cov(acs_ctx* ctx, int64_t n_pts, double* cov, const double* dcov, int32_t* status,
                      const int32_t* dstatus, bool report, uint32_t flags) {
  int rc;
  if ((rc = acs_stage_out(ctx, cov, dcov, sizeof(double) * 9 * n_pts, flags))) return rc;
  if (status && (rc = acs_stage_out(ctx, status, dstatus, sizeof(int32_t) * n_pts, flags))) return rc;
  if (report || !(flags & ACS_DEVICE_PTRS)) ACS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ACS_OK;
}

extern "C" {

int acs_sba_points_dense_covariance(acs_ctx* ctx, const double* cams, int32_t n_cams, const double* uv,
                                    const uint8_t* mask, int64_t n_pts, const double* pts, double f_scale,
                                    double sigma_px, double* cov, int32_t* status, acs_sba_cov_report* report,
                                    uint32_t flags) {
  ACS_DEVICE_GUARD(ctx);
  ACS_CHECK(ctx, n_pts >= 0 && n_cams >= 1 && n_cams <= 255,
            "acs_sba_points_dense_covariance: n_pts=%lld n_cams=%d (1..255)", (long long)n_pts, n_cams);
  ACS_CHECK(ctx, f_scale > 0 && sigma_px > 0, "acs_sba_points_dense_covariance: f_scale=%g sigma_px=%g (both > 0)",
            f_scale, sigma_px);
  if (n_pts == 0) {
    if (report) std::memset(report, 0, sizeof(*report));
    return ACS_OK;
  }
  void *dc, *duv, *dm, *dp;
  int rc;
  const int model = acs_flags_model(flags);
  if ((rc = acs_stage_in(ctx, WS_CAMS, cams, sizeof(double) * acs_cam_stride(model) * n_cams, flags, &dc))) return rc;
  if ((rc = acs_stage_in(ctx, WS_UV, uv, sizeof(double) * 2 * n_pts * n_cams, flags, &duv))) return rc;
  if ((rc = acs_stage_in(ctx, WS_MASK, mask, (size_t)n_pts * n_cams, flags, &dm))) return rc;
  if ((rc = acs_stage_in(ctx, WS_PTS, pts, sizeof(double) * 3 * n_pts, flags, &dp))) return rc;
  double* dcov = (double*)acs_out_buf(ctx, WS_OUT0, cov, sizeof(double) * 9 * n_pts, flags);
  int32_t* dst = status ? (int32_t*)acs_out_buf(ctx, WS_OUT1, status, sizeof(int32_t) * n_pts, flags) : nullptr;
  if (!dcov || (status && !dst)) return ACS_E_NOMEM;
  if ((rc = run_cov(ctx, model, (const double*)dc, n_cams, n_cams, (const double2*)duv, (const uint8_t*)dm, nullptr,
                    n_pts, (const double*)dp, f_scale, sigma_px, dcov, dst, report)))
    return rc;
  return finish_cov(ctx, n_pts, cov, dcov, status, dst, report != nullptr, flags);
}

int acs_sba_points_covariance(acs_ctx* ctx, const double* cams, int32_t n_cams, const double* uv,
                              const int32_t* pt_idx, const int32_t* cam_idx, int64_t n_obs, const double* pts,
                              int64_t n_pts, double f_scale, double sigma_px, double* cov, int32_t* status,
                              acs_sba_cov_report* report, uint32_t flags) {
  ACS_DEVICE_GUARD(ctx);
  ACS_CHECK(ctx, n_obs >= 0 && n_pts >= 0 && n_cams >= 1 && n_cams <= 255, "acs_sba_points_covariance: bad sizes");
  ACS_CHECK(ctx, n_obs < (int64_t)INT32_MAX, "acs_sba_points_covariance: n_obs too large");
  ACS_CHECK(ctx, f_scale > 0 && sigma_px > 0, "acs_sba_points_covariance: f_scale=%g sigma_px=%g (both > 0)", f_scale,
            sigma_px);
  if (n_pts == 0) {
    if (report) std::memset(report, 0, sizeof(*report));
    return ACS_OK;
  }
  int rc;
  const int model = acs_flags_model(flags);
  ObsSlots o;  // without observations every point is ACS_COV_NOOBS
  if ((rc = acs_stage_obs(ctx, "acs_sba_points_covariance", 256, acs_cam_stride(model), cams, n_cams, uv, pt_idx,
                          cam_idx, n_obs, pts, n_pts, flags, &o)))
    return rc;
  double* dcov = (double*)acs_out_buf(ctx, WS_OUT0, cov, sizeof(double) * 9 * n_pts, flags);
  int32_t* dst = status ? (int32_t*)acs_out_buf(ctx, WS_OUT1, status, sizeof(int32_t) * n_pts, flags) : nullptr;
  if (!dcov || (status && !dst)) return ACS_E_NOMEM;
  if ((rc = run_cov(ctx, model, o.cams, n_cams, o.K, o.uvp, o.mask, o.camid, n_pts, o.pts, f_scale, sigma_px, dcov, dst,
                    report)))
    return rc;
  return finish_cov(ctx, n_pts, cov, dcov, status, dst, report != nullptr, flags);
}

}  // extern "C"
