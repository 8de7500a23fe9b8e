// sba_ext_cov.hip — camera-pose and joint point covariances of the points + extrinsics SBA
// (sba_ext.hip) on gfx950.
//
// Definition (include/acinoset_hip.h), everything at the state passed in:
//   per camera (dw, dt): R <- exp([dw]x) R, t <- t + dt; J_cam = J_Y [-[R X]x | I], J_pt = J_Y R;
//   wh = max((1 - z) w^2, 0.1 w), w = 1 / (1 + z), z = r^2 / f_scale^2 (ext_obs_blocks, sba_ext.hpp).
//   Point status on its own V = sum wh J_pt^T J_pt (cov_point_status); a point that is not OK is
//   left out entirely. S = sum U - sum_OK W V^-1 W^T, undamped, symmetrised.
//   Gauge generators G (6C x 7): rotation dw = -R_c theta; translation dt = -R_c tau; scale
//   dt = t_c. Q = orth(G), mu = max diag S, Ah = S + mu Q Q^T scaled to unit diagonal.
//   FREE:   cov = sigma^2 [(S + mu Q Q^T)^-1 - Q Q^T / mu]
//   ANCHOR: cov = P cov_free P^T, P = I - Q (Cm Q)^-1 Cm, Cm = [I_6 on camera a; h on camera b],
//           h = e^T [-R_b^T [t_b]x | -R_b^T], e the unit baseline of the centres c = -R^T t.
//   Degenerate: G of rank < 7, or a pivot of the unpivoted LDL^T of Ah fails d > 1e-9.
//   Point i: cov_i = sigma^2 V_i^-1 + V_i^-1 B_i^T cov_cc B_i V_i^-1.
//
// Kernels:
//   k_extcov_linearize<G> [point groups] one point per aligned lane group (ACS_G_SWITCH): per
//                   slot U (21 packed) and W (18) by ext_obs_blocks; per point V summed over the
//                   group, V^-1 and its status (ldl3_inverse, cov_point_status; common.hpp) and
//                   the sigma_hat terms
//   k_extcov_schur  [point chunks] fixed-order chunk partials of S over the OK points
//                   (ext_schur_stage, ext_schur_entry with M = V^-1; no atomics)
//   k_extcov_cams   [1 block] the core of sba_cov_cams.hpp with seven generators (chunk sums in
//                   order, symmetrise, Gram-Schmidt of G, mu, Jacobi scaling, scalar LDL^T pivot
//                   test, SPD inverse on the f64 MFMA tiles (wg_spd_inverse) with one refinement
//                   step, unscale, - Q Q^T / mu, the report's sums; shared with k_brdcov_cams of
//                   sba_boards_cov.hip); here G, the anchor transform with the baseline row, the
//                   mirror, sigma^2 and the report
//   k_extcov_points<G> [point groups] cov_cc staged in LDS; lane l owns slot l: T = sum_o'
//                   cov_cc[c_o, c_o'] W_o', then W_o^T T, group_sum, lane 0 writes the record
#include "sba_cov_cams.hpp"
#include "sba_ext.hpp"

template <int G>
__global__ __launch_bounds__(256) void k_extcov_linearize(ExtDims d, const double* __restrict__ cams,
                                                          const double* __restrict__ pts,
                                                          const double2* __restrict__ uv,
                                                          const uint8_t* __restrict__ mask,
                                                          const uint8_t* __restrict__ camid, double* __restrict__ Q,
                                                          double* __restrict__ Vi, int32_t* __restrict__ status,
                                                          double* __restrict__ wr2, int32_t* __restrict__ nres) {
  __shared__ double s_cam[EXT_MAXC * ACS_CAM_STRIDE];
  for (int i = threadIdx.x; i < d.C * ACS_CAM_STRIDE; i += blockDim.x) s_cam[i] = cams[i];
  __syncthreads();
  const int lane = threadIdx.x & (G - 1);
  const int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
  if (p >= d.n) return;  // whole group leaves together
  const double X0 = pts[3 * p], X1 = pts[3 * p + 1], X2 = pts[3 * p + 2];
  // V (packed upper: 00 01 02 11 12 22), sum w r^2, number of scalar residuals
  double v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = 0.0;
  for (int slot = lane; slot < d.K; slot += G) {
    const int64_t o = p * d.K + slot;
    double* q = Q + (size_t)o * EXT_Q<false>;
    if (!mask[o] || camid[o] >= d.C) {
      for (int e = 0; e < EXT_Q<false>; ++e) q[e] = 0.0;
      continue;
    }
    ExtObs ob;
    ext_obs_blocks(s_cam + camid[o] * ACS_CAM_STRIDE, X0, X1, X2, uv[o], d.f2, ob, q);
    for (int dd = 0; dd < 2; ++dd) {
      const double* jp = ob.jp[dd];
      const double wh = ob.wh[dd];
      v[0] += wh * jp[0] * jp[0];
      v[1] += wh * jp[0] * jp[1];
      v[2] += wh * jp[0] * jp[2];
      v[3] += wh * jp[1] * jp[1];
      v[4] += wh * jp[1] * jp[2];
      v[5] += wh * jp[2] * jp[2];
      v[6] += ob.w[dd] * (ob.r[dd] * ob.r[dd]);
    }
    v[7] += 2.0;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = group_sum<G>(v[i]);
  if (lane != 0) return;
  double ci[6];
  const bool ok = ldl3_inverse(v, [](double x) { return 1.0 / x; }, ci);
  const int st = cov_point_status(v[7], ok);
  const bool good = st == ACS_COV_OK;
  double* vi = Vi + (size_t)p * 6;  // V^-1, packed upper; zeros for a point that is left out
  for (int e = 0; e < 6; ++e) vi[e] = good ? ci[e] : 0.0;
  status[p] = st;
  wr2[p] = good ? v[6] : 0.0;
  nres[p] = good ? (int32_t)v[7] : 0;
}

// chunk partial of S (6C x 6C) over the OK points of the chunk, every entry summed in point and
// slot order by one thread
__global__ __launch_bounds__(256) void k_extcov_schur(ExtDims d, const double* __restrict__ Q,
                                                      const double* __restrict__ Vi,
                                                      const int32_t* __restrict__ status,
                                                      const uint8_t* __restrict__ mask,
                                                      const uint8_t* __restrict__ camid, double* __restrict__ part) {
  const int ch = blockIdx.x;
  const int p0 = ch * d.chunk, p1 = min(d.n, p0 + d.chunk), np = p1 - p0;
  const int NC = 6 * d.C, nE = NC * NC;
  extern __shared__ double lds[];
  double* sZ = lds;                                     // np x K x 18  (W V^-1)
  int* scam = (int*)(sZ + (size_t)d.chunk * d.K * 18);  // np x K camera id (-1 = none / left out)
  ext_schur_stage<false>(d, p0, np, Q, mask, camid, sZ, scam, [&](int p, int, double* M) {
    const double* vi = Vi + (size_t)p * 6;
    const double m[9] = {vi[0], vi[1], vi[2], vi[1], vi[3], vi[4], vi[2], vi[4], vi[5]};
    for (int k = 0; k < 9; ++k) M[k] = m[k];
    return status[p] == ACS_COV_OK;
  });
  for (int e = threadIdx.x; e < nE; e += blockDim.x)
    part[(size_t)ch * nE + e] = ext_schur_entry<false>(d, p0, np, Q, sZ, scam, e / NC, e % NC);
}

struct XcCamArgs {
  int nchunk, gauge, a, b;
  double s2;
};

__global__ __launch_bounds__(256) void k_extcov_cams(ExtDims d, XcCamArgs ar, const double* __restrict__ part,
                                                     const double* __restrict__ cams,
                                                     const int32_t* __restrict__ status,
                                                     const double* __restrict__ wr2, const int32_t* __restrict__ nres,
                                                     double* __restrict__ Ag, double* __restrict__ T1,
                                                     double* __restrict__ T2, double* __restrict__ cov,
                                                     acs_sba_ext_cov_report* __restrict__ rep, int* __restrict__ bad) {
  const int NC = 6 * d.C, NP = ((NC + 15) / 16) * 16, LD = NP + 1, nE = NC * NC;
  const int tid = threadIdx.x;
  extern __shared__ double lds[];
  const CovCamsLds L = cov_cams_carve(lds, NP);
  // sQ: seven columns; s_sm: from 8 h, from 16 (Cm Q)^-1
  double *sS = L.sS, *sQ = L.sQ, *sK = L.sK, *sMC = L.sMC, *sCM = L.sCM, *s_sm = L.s_sm;
  cov_cams_sum_chunks(L, NC, NP, ar.nchunk, part, T1);  // 1.
  // 2. gauge generators
  for (int e = tid; e < NP * 8; e += blockDim.x) {
    const int r = e >> 3, k = e & 7;
    double v = 0.0;
    if (r < NC && k < 7) {
      const double* cm = cams + (r / 6) * ACS_CAM_STRIDE;
      const int i = r % 6;
      if (i < 3)
        v = k < 3 ? -cm[8 + 3 * i + k] : 0.0;
      else
        v = k < 3 ? 0.0 : (k < 6 ? -cm[8 + 3 * (i - 3) + (k - 3)] : cm[17 + (i - 3)]);
    }
    sQ[e] = v;
  }
  __syncthreads();
  double mu, minp = __builtin_inf();
  bool gbad;
  bool degenerate = cov_cams_factor<7>(L, NC, NP, Ag, mu, minp, gbad);  // 3. - 5., uniform
  if (!degenerate) {
    cov_cams_invert<7>(L, NC, NP, mu, Ag, T1, T2, bad);  // 6. - 8.
    if (ar.gauge == ACS_GAUGE_ANCHOR) {
      // 9. M <- P M P^T, P = I - K Cm, K = Q (Cm Q)^-1
      if (tid == 0) {
        const double* ca = cams + ar.a * ACS_CAM_STRIDE;
        const double* cb = cams + ar.b * ACS_CAM_STRIDE;
        double e3[3], n2 = 0.0;
        for (int j = 0; j < 3; ++j) {  // c = -R^T t
          const double a_ = -(ca[8 + j] * ca[17] + ca[11 + j] * ca[18] + ca[14 + j] * ca[19]);
          const double b_ = -(cb[8 + j] * cb[17] + cb[11 + j] * cb[18] + cb[14 + j] * cb[19]);
          e3[j] = b_ - a_;
          n2 += e3[j] * e3[j];
        }
        const double in = 1.0 / sqrt(n2);
        for (int j = 0; j < 3; ++j) e3[j] *= in;
        // y = R_b e; h = [t_b x y, -y]  (e^T (-R^T [t]x) = -y^T [t]x = (t x y)^T)
        double y[3];
        for (int i = 0; i < 3; ++i) y[i] = cb[8 + 3 * i] * e3[0] + cb[8 + 3 * i + 1] * e3[1] + cb[8 + 3 * i + 2] * e3[2];
        const double* tb = cb + 17;
        double* h = s_sm + 8;
        h[0] = tb[1] * y[2] - tb[2] * y[1];
        h[1] = tb[2] * y[0] - tb[0] * y[2];
        h[2] = tb[0] * y[1] - tb[1] * y[0];
        h[3] = -y[0];
        h[4] = -y[1];
        h[5] = -y[2];
        // Cm Q (7 x 7) and its inverse by Gauss-Jordan with partial pivoting
        double A[7][14];
        for (int k = 0; k < 7; ++k) {
          for (int i = 0; i < 6; ++i) A[i][k] = sQ[(6 * ar.a + i) * 8 + k];
          double v = 0.0;
          for (int j = 0; j < 6; ++j) v += h[j] * sQ[(6 * ar.b + j) * 8 + k];
          A[6][k] = v;
          for (int i = 0; i < 7; ++i) A[i][7 + k] = i == k ? 1.0 : 0.0;
        }
        bool abad = false;
        for (int k = 0; k < 7; ++k) {
          int pv = k;
          for (int i = k + 1; i < 7; ++i)
            if (fabs(A[i][k]) > fabs(A[pv][k])) pv = i;
          if (!(fabs(A[pv][k]) > 1e-12)) {
            abad = true;
            break;
          }
          for (int j = 0; j < 14; ++j) {
            const double x = A[k][j];
            A[k][j] = A[pv][j];
            A[pv][j] = x;
          }
          const double ip = 1.0 / A[k][k];
          for (int j = 0; j < 14; ++j) A[k][j] *= ip;
          for (int i = 0; i < 7; ++i) {
            if (i == k) continue;
            const double f = A[i][k];
            for (int j = 0; j < 14; ++j) A[i][j] -= f * A[k][j];
          }
        }
        for (int i = 0; i < 7; ++i)
          for (int k = 0; k < 7; ++k) s_sm[16 + i * 7 + k] = A[i][7 + k];
        s_sm[2] = abad ? 1.0 : 0.0;
      }
      __syncthreads();
      const double* h = s_sm + 8;
      for (int e = tid; e < NC * 8; e += blockDim.x) {
        const int r = e >> 3, k = e & 7;
        double v = 0.0;
        if (k < 7)
          for (int j = 0; j < 7; ++j) v += sQ[r * 8 + j] * s_sm[16 + j * 7 + k];
        sK[e] = v;
      }
      for (int e = tid; e < 7 * NC; e += blockDim.x) {
        const int k = e / NC, c = e % NC;
        double v;
        if (k < 6) {
          v = sS[(6 * ar.a + k) * LD + c];
        } else {
          v = 0.0;
          for (int j = 0; j < 6; ++j) v += h[j] * sS[(6 * ar.b + j) * LD + c];
        }
        sCM[k * NP + c] = v;
      }
      __syncthreads();
      for (int e = tid; e < nE; e += blockDim.x) {
        const int r = e / NC, c = e % NC;
        double v = 0.0;
        for (int k = 0; k < 7; ++k) v += sK[r * 8 + k] * sCM[k * NP + c];
        sS[r * LD + c] -= v;
      }
      __syncthreads();
      for (int e = tid; e < NC * 8; e += blockDim.x) {
        const int r = e >> 3, k = e & 7;
        double v = 0.0;
        if (k < 6) {
          v = sS[r * LD + 6 * ar.a + k];
        } else if (k == 6) {
          for (int j = 0; j < 6; ++j) v += h[j] * sS[r * LD + 6 * ar.b + j];
        }
        sMC[e] = v;
      }
      __syncthreads();
      for (int e = tid; e < nE; e += blockDim.x) {
        const int r = e / NC, c = e % NC;
        double v = 0.0;
        for (int k = 0; k < 7; ++k) v += sMC[r * 8 + k] * sK[c * 8 + k];
        sS[r * LD + c] -= v;
      }
      __syncthreads();
      degenerate = s_sm[2] != 0.0;
    }
  }
  // 10. mirror the upper triangle, sigma^2, exact zeros on the anchor camera, NaN when degenerate
  const double nan = __builtin_nan("");
  const bool anchored = ar.gauge == ACS_GAUGE_ANCHOR;
  for (int e = tid; e < nE; e += blockDim.x) {
    const int r = e / NC, c = e % NC, lo = min(r, c), hi = max(r, c);
    double v = ar.s2 * sS[lo * LD + hi];
    if (anchored && (r / 6 == ar.a || c / 6 == ar.a)) v = 0.0;
    cov[e] = degenerate ? nan : v;
  }
  const CovCamsTotals tot = cov_cams_totals(L, NC, NP, ar.s2, anchored ? ar.a : -1, false, d.n, status, wr2, nres);
  if (tid == 0) {
    const long long n_ok = tot.n_ok, dof = tot.n_res - 3 * n_ok - (6 * d.C - 7);
    rep->status = degenerate ? ACS_EXT_COV_DEGENERATE : ACS_EXT_COV_OK;
    rep->reserved = 0;
    rep->n_points = d.n;
    rep->n_ok = n_ok;
    rep->n_noobs = tot.n_noobs;
    rep->n_degenerate = tot.n_degenerate;
    rep->dof = dof;
    rep->min_pivot = gbad ? 0.0 : minp;
    rep->sigma_hat_px = dof > 0 ? sqrt(tot.wr2 / (double)dof) : nan;
    rep->rot_sd_max = degenerate ? nan : tot.rot_sd_max;
    rep->trans_sd_max = degenerate ? nan : tot.trans_sd_max;
  }
}

// The throughput path: one point per aligned lane group, lane l owns slot l. cov_cc (6C x 6C,
// sigma^2 applied) is staged in LDS.
template <int G>
__global__ __launch_bounds__(256) void k_extcov_points(ExtDims d, const double* __restrict__ covc,
                                                       const double* __restrict__ Q, const double* __restrict__ Vi,
                                                       const int32_t* __restrict__ status,
                                                       const uint8_t* __restrict__ mask,
                                                       const uint8_t* __restrict__ camid, double s2,
                                                       const acs_sba_ext_cov_report* __restrict__ rep,
                                                       double* __restrict__ covp) {
  const int NC = 6 * d.C;
  extern __shared__ double s_cc[];
  for (int i = threadIdx.x; i < NC * NC; i += blockDim.x) s_cc[i] = covc[i];
  __syncthreads();
  const int lane = threadIdx.x & (G - 1);
  const int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
  if (p >= d.n) return;  // whole group leaves together
  const bool pok = status[p] == ACS_COV_OK;
  double acc[6] = {0, 0, 0, 0, 0, 0};  // B^T cov_cc B, packed upper
  if (pok) {
    for (int slot = lane; slot < d.K; slot += G) {
      const int64_t o = p * d.K + slot;
      if (!mask[o] || camid[o] >= d.C) continue;
      const int co = camid[o];
      const double* Wo = Q + (size_t)o * EXT_Q<false> + EXT_Q_W;
      double T[18];
      for (int e = 0; e < 18; ++e) T[e] = 0.0;
      for (int s = 0; s < d.K; ++s) {
        const int64_t o2 = p * d.K + s;
        if (!mask[o2] || camid[o2] >= d.C) continue;
        const double* W2 = Q + (size_t)o2 * EXT_Q<false> + EXT_Q_W;
        const double* blk = s_cc + (size_t)(6 * co) * NC + 6 * camid[o2];
        for (int k = 0; k < 6; ++k) {
          const double w0 = W2[k * 3], w1 = W2[k * 3 + 1], w2 = W2[k * 3 + 2];
          for (int i = 0; i < 6; ++i) {
            const double c = blk[i * NC + k];
            T[i * 3] += c * w0;
            T[i * 3 + 1] += c * w1;
            T[i * 3 + 2] += c * w2;
          }
        }
      }
      for (int i = 0; i < 6; ++i) {
        const double w0 = Wo[i * 3], w1 = Wo[i * 3 + 1], w2 = Wo[i * 3 + 2];
        acc[0] += w0 * T[i * 3];
        acc[1] += w0 * T[i * 3 + 1];
        acc[2] += w0 * T[i * 3 + 2];
        acc[3] += w1 * T[i * 3 + 1];
        acc[4] += w1 * T[i * 3 + 2];
        acc[5] += w2 * T[i * 3 + 2];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) acc[i] = group_sum<G>(acc[i]);
  if (lane != 0) return;
  const double* vi = Vi + (size_t)p * 6;
  const double A[9] = {vi[0], vi[1], vi[2], vi[1], vi[3], vi[4], vi[2], vi[4], vi[5]};
  const double Mm[9] = {acc[0], acc[1], acc[2], acc[1], acc[3], acc[4], acc[2], acc[4], acc[5]};
  double AM[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) AM[i * 3 + j] = A[i * 3] * Mm[j] + A[i * 3 + 1] * Mm[3 + j] + A[i * 3 + 2] * Mm[6 + j];
  const bool good = pok && rep->status == ACS_EXT_COV_OK;
  const double nan = __builtin_nan("");
  double out[9];
  for (int i = 0; i < 3; ++i)
    for (int j = i; j < 3; ++j) {
      const double v = s2 * A[i * 3 + j] + AM[i * 3] * A[j] + AM[i * 3 + 1] * A[3 + j] + AM[i * 3 + 2] * A[6 + j];
      out[i * 3 + j] = out[j * 3 + i] = good ? v : nan;  // the upper triangle mirrored
    }
  double* c = covp + 9 * p;
  for (int e = 0; e < 9; ++e) c[e] = out[e];
}

extern "C" {

void acs_sba_ext_cov_default_opts(acs_sba_ext_cov_opts* o) {
  o->gauge = ACS_GAUGE_ANCHOR;
  o->anchor_cam = 0;
  o->scale_cam = 1;
  o->reserved = 0;
  o->f_scale = 1.0;
  o->sigma_px = 1.0;
}

int acs_sba_extrinsics_covariance(acs_ctx* ctx, const double* cams, int32_t n_cams, const double* uv,
                                  const int32_t* pt_idx, const int32_t* cam_idx, int64_t n_obs, const double* pts,
                                  int64_t n_pts, const acs_sba_ext_cov_opts* opts, double* cov_cams, double* cov_pts,
                                  int32_t* pt_status, acs_sba_ext_cov_report* report, uint32_t flags) {
  ACS_DEVICE_GUARD(ctx);
  ACS_FISHEYE_ONLY(ctx, flags, "acs_sba_extrinsics_covariance");
  acs_sba_ext_cov_opts op;
  acs_sba_ext_cov_default_opts(&op);
  if (opts) op = *opts;
  ACS_CHECK(ctx, n_cams >= 1 && n_cams <= EXT_MAXC, "acs_sba_extrinsics_covariance: n_cams=%d (1..%d)", n_cams,
            EXT_MAXC);
  ACS_CHECK(ctx, n_obs >= 1 && n_pts >= 1 && n_obs < (int64_t)INT32_MAX && n_pts < (int64_t)INT32_MAX / 64,
            "acs_sba_extrinsics_covariance: bad sizes");
  ACS_CHECK(ctx, op.f_scale > 0 && op.sigma_px > 0, "acs_sba_extrinsics_covariance: f_scale=%g sigma_px=%g (both > 0)",
            op.f_scale, op.sigma_px);
  ACS_CHECK(ctx, op.gauge == ACS_GAUGE_FREE || op.gauge == ACS_GAUGE_ANCHOR, "acs_sba_extrinsics_covariance: gauge %d",
            op.gauge);
  ACS_CHECK(ctx, cams && uv && pt_idx && cam_idx && pts && cov_cams, "acs_sba_extrinsics_covariance: null argument");
  hipStream_t s = ctx->stream;
  // one camera has no anchor pair: the problem is reported DEGENERATE, not refused
  const bool anchored = op.gauge == ACS_GAUGE_ANCHOR && n_cams >= 2;
  if (anchored) {
    ACS_CHECK(ctx, op.anchor_cam >= 0 && op.anchor_cam < n_cams && op.scale_cam >= 0 && op.scale_cam < n_cams,
              "acs_sba_extrinsics_covariance: anchor_cam=%d scale_cam=%d (0..%d)", op.anchor_cam, op.scale_cam,
              n_cams - 1);
    ACS_CHECK(ctx, op.anchor_cam != op.scale_cam, "acs_sba_extrinsics_covariance: anchor_cam == scale_cam (%d)",
              op.anchor_cam);
    double rec[2][ACS_CAM_STRIDE];
    const int id[2] = {op.anchor_cam, op.scale_cam};
    for (int k = 0; k < 2; ++k) {
      const double* src = cams + (size_t)id[k] * ACS_CAM_STRIDE;
      if (flags & ACS_DEVICE_PTRS) {
        ACS_HIP(ctx, hipMemcpyAsync(rec[k], src, sizeof(rec[k]), hipMemcpyDeviceToHost, s));
        ACS_HIP(ctx, hipStreamSynchronize(s));
      } else {
        std::memcpy(rec[k], src, sizeof(rec[k]));
      }
    }
    double d2 = 0.0, sc2 = 0.0;
    for (int j = 0; j < 3; ++j) {
      double c[2];
      for (int k = 0; k < 2; ++k)
        c[k] = -(rec[k][8 + j] * rec[k][17] + rec[k][11 + j] * rec[k][18] + rec[k][14 + j] * rec[k][19]);
      d2 += (c[1] - c[0]) * (c[1] - c[0]);
      sc2 += c[0] * c[0] + c[1] * c[1];
    }
    ACS_CHECK(ctx, d2 > 1e-24 * (sc2 > 1.0 ? sc2 : 1.0),
              "acs_sba_extrinsics_covariance: the centres of cameras %d and %d coincide", op.anchor_cam, op.scale_cam);
  }
  int rc;
  ObsSlots in;
  if ((rc = acs_stage_obs(ctx, "acs_sba_extrinsics_covariance", EXT_MAXK, ACS_CAM_STRIDE, cams, n_cams, uv, pt_idx,
                          cam_idx, n_obs, pts, n_pts, flags, &in)))
    return rc;
  const ExtDims d = ext_dims(n_pts, in.K, n_cams, op.f_scale);
  const int nchunk = ext_nchunk(d);
  const int NC = 6 * n_cams, NP = ((NC + 15) / 16) * 16, nE = NC * NC;
  double *Q, *Vi, *wr2, *part, *Ag, *T1, *T2;
  int32_t* nres;
  int* bad;
  auto layout = [&](double* base) {
    Arena a{base};
    Q = a.take((size_t)n_pts * d.K * EXT_Q<false>);
    Vi = a.take((size_t)n_pts * 6);
    wr2 = a.take(n_pts);
    nres = a.take<int32_t>(((size_t)n_pts + 1) / 2);
    part = a.take((size_t)nchunk * nE);
    Ag = a.take((size_t)NP * NP);
    T1 = a.take((size_t)NP * NP);
    T2 = a.take((size_t)NP * NP);
    bad = a.take<int>(2);
    return a.bytes();
  };
  double* arena = (double*)acs_ws(ctx, WS_FTE7, layout(nullptr));
  double* dcc = (double*)acs_out_buf(ctx, WS_OUT0, cov_cams, sizeof(double) * nE, flags);
  // without cov_pts the point kernel is not run; the status is needed by the camera kernel anyway
  double* dcp = cov_pts ? (double*)acs_out_buf(ctx, WS_OUT1, cov_pts, sizeof(double) * 9 * n_pts, flags) : nullptr;
  int32_t* dst = (int32_t*)acs_out_buf(ctx, WS_PERPT_I, pt_status, sizeof(int32_t) * n_pts,
                                       pt_status ? flags : (flags & ~ACS_DEVICE_PTRS));
  acs_sba_ext_cov_report* drep = (acs_sba_ext_cov_report*)acs_ws(ctx, WS_REPORT, sizeof(acs_sba_ext_cov_report));
  if (!arena || !dcc || (cov_pts && !dcp) || !dst || !drep) return ACS_E_NOMEM;
  layout(arena);
  ACS_HIP(ctx, hipMemsetAsync(bad, 0, sizeof(int), s));
  const int blocks = acs_grid((int64_t)n_pts * d.G, 256);
#define XC_LIN(g)                                                                                                  \
  hipLaunchKernelGGL((k_extcov_linearize<g>), dim3(blocks), dim3(256), 0, s, d, in.cams, in.pts, in.uvp, in.mask, \
                     in.camid, Q, Vi, dst, wr2, nres)
  ACS_G_SWITCH(d.G, XC_LIN)
#undef XC_LIN
  hipLaunchKernelGGL(k_extcov_schur, dim3(nchunk), dim3(256), ext_schur_lds(d, 0), s, d, Q, Vi, dst, in.mask, in.camid,
                     part);
  XcCamArgs ar{nchunk, anchored ? ACS_GAUGE_ANCHOR : ACS_GAUGE_FREE, anchored ? op.anchor_cam : 0,
               anchored ? op.scale_cam : 0, op.sigma_px * op.sigma_px};
  hipLaunchKernelGGL(k_extcov_cams, dim3(1), dim3(256), cov_cams_lds(NP), s, d, ar, part, in.cams, dst, wr2, nres, Ag,
                     T1, T2, dcc, drep, bad);
  if (dcp) {
#define XC_PTS(g)                                                                                                   \
  hipLaunchKernelGGL((k_extcov_points<g>), dim3(blocks), dim3(256), sizeof(double) * nE, s, d, dcc, Q, Vi, dst, in.mask, \
                     in.camid, ar.s2, drep, dcp)
    ACS_G_SWITCH(d.G, XC_PTS)
#undef XC_PTS
  }
  ACS_HIP(ctx, hipGetLastError());
  if ((rc = acs_stage_out(ctx, cov_cams, dcc, sizeof(double) * nE, flags))) return rc;
  if (cov_pts && (rc = acs_stage_out(ctx, cov_pts, dcp, sizeof(double) * 9 * n_pts, flags))) return rc;
  if (pt_status && (rc = acs_stage_out(ctx, pt_status, dst, sizeof(int32_t) * n_pts, flags))) return rc;
  if (report) ACS_HIP(ctx, hipMemcpyAsync(report, drep, sizeof(*report), hipMemcpyDeviceToHost, s));
  ACS_HIP(ctx, hipStreamSynchronize(s));
  return ACS_OK;
}

}  // extern "C"
