// sba_boards_cov.hip — camera and board pose covariances of the rigid-board bundle adjustment
// (sba_boards.hip) on gfx950 (acs_sba_boards_covariance).
//
// Definition (include/acinoset_hip.h, tests/sba_boards_cov_ref.py), everything at the
// cameras and board poses passed in; nothing is solved:
//   the problem and the linearisation of acs_sba_boards: fisheye records, 1 <= C <= 16,
//   3 <= nc <= 256, B >= 1, uv (B, C, nc, 2), mask (B, C); left perturbations
//   R <- exp([dw]x) R, t <- t + dt for cameras and boards; J_cam = J_Y [-[R_c X]x | I],
//   J_pt = J_Y R_c, J_brd = J_pt [-[R_b p_j]x | I]; wh = max((1 - z) w^2, 0.1 w), w = 1 / (1 + z),
//   z = r^2 / f_scale^2; per seen view U_bc, W_bc (6 x 6), per board V_b = sum wh J_brd^T J_brd,
//   all undamped.
//   Board status: NOOBS without a view; DEGENERATE when an entry of diag V_b is not > 0 or a
//   pivot of the unpivoted LDL^T of V_b scaled to unit diagonal fails d > 1e-9 (a NaN fails);
//   else OK. A board that is not OK is left out entirely (its U, W and V terms).
//   S = sum_OK U_bc - sum_OK W_b V_b^-1 W_b^T (6C x 6C, symmetrised), W_b the 6C x 6 stack.
//   Gauge generators G (6C x 6), per camera c: rotation theta: dw = -R_c theta; translation tau:
//   dt = -R_c tau. Q = orth(G), mu = max diag S, Ah = S + mu Q Q^T scaled to unit diagonal.
//   FREE:   cov_cc = sigma^2 [(S + mu Q Q^T)^-1 - Q Q^T / mu]
//   ANCHOR: cov_cc = P cov_free P^T, P = I - G (Cm G)^-1 Cm, Cm (6 x 6C) the identity on camera
//           a; camera a's rows and columns exact zeros; scale_cam is ignored.
//   Degenerate problem: a diagonal entry of Ah's unscaled form is not > 0, a pivot of the unpivoted
//   LDL^T of Ah in natural order fails d > 1e-9, or G has rank < 6. Then every covariance is NaN.
//   One camera: decided before S is formed; cov_cams exact zeros, status OK, min_pivot NaN.
//   Board b (OK): cov_b = sigma^2 V_b^-1 + V_b^-1 W_b^T cov_cc W_b V_b^-1; NaN for the others.
//   sigma_hat^2 = sum w r^2 / dof over the OK boards' views, dof = m - 6 n_ok - (6C - 6).
//
// Kernels:
//   k_brdcov_linearize [1 block of 4 waves per board] k_brd_linearize's mapping and code (brd_stage,
//                   brd_view_sums; sba_boards.hpp: waves over the cameras, lanes over the corners,
//                   group_sum<64> per entry kept by the owning lane) without state, gradient and
//                   cost: the view record U (21), W (36) and, over the views in camera order, V (21)
//                   and sum w r^2; then the board's unit-diagonal LDL^T status and V^-1
//   k_brdcov_schur  [board chunks x entry slices] undamped S over the OK boards: W V^-1 tiles in
//                   LDS, each entry summed by one thread in board order (brd_schur_stage,
//                   brd_schur_entry with M = V^-1: k_brd_schur's code and layout)
//   k_brdcov_cams   [1 block] the core of sba_cov_cams.hpp with six generators (chunk sums in order,
//                   symmetrise, Gram-Schmidt of G, mu, Jacobi scaling, scalar pivot test,
//                   wg_spd_inverse with one refinement step, unscale, - Q Q^T / mu, the report's
//                   sums); here G, the six-row anchor transform, the symmetric part, sigma^2, the
//                   one-camera shortcut and the report
//   k_brdcov_boards [4 boards per block, one wave each] cov_cc staged in LDS; lane e < 36 owns
//                   entry e of T = sum_{c, c'} W_bc^T cov_cc[c, c'] W_bc' (seen cameras in camera
//                   order), then V^-1 T V^-1 + sigma^2 V^-1, the upper triangle mirrored
//   k_brdcov_board_sd [1 block] the largest board sds of the report
// No floating-point atomics; every sum has a fixed order.
#include "sba_boards.hpp"
#include "sba_cov_cams.hpp"

#define BC_PIVOT_TOL 1e-9  // pivots of the unit-diagonal V_b

// a view's part of the board record; the view record is BRD_Q<false> (sba_boards.hpp)
enum : int { BC_P_V = 0, BC_P_WR2 = 21, BC_P = 22 };

// V (packed upper, upk) -> V^-1 (row-major) through the unpivoted LDL^T of V scaled to unit
// diagonal; false when a diagonal entry is not > 0 or a pivot fails d > BC_PIVOT_TOL (a NaN fails)
__device__ __forceinline__ bool bc_vinv(const double* V, double Vi[36]) {
  double sc[6], L[6][6], Li[6][6], dg[6];
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double v = V[upk(i, i)];
    const bool pos = v > 0.0;
    ok = ok && pos;
    sc[i] = pos ? 1.0 / sqrt(v) : 0.0;
  }
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double a = V[upk(j, j)] * sc[j] * sc[j];
#pragma unroll
    for (int k = 0; k < j; ++k) a -= L[j][k] * L[j][k] * dg[k];
    dg[j] = a;
    ok = ok && (a > BC_PIVOT_TOL);
    const double inv = 1.0 / a;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double s = V[upk(j, i)] * sc[i] * sc[j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k] * dg[k];
      L[i][j] = s * inv;
    }
  }
  // Li = L^-1 (unit lower), V^-1 = Li^T D^-1 Li, unscaled
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    Li[j][j] = 1.0;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double a = 0.0;
#pragma unroll
      for (int k = j; k < i; ++k) a -= L[i][k] * Li[k][j];
      Li[i][j] = a;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i; j < 6; ++j) {
      double a = 0.0;
#pragma unroll
      for (int k = j; k < 6; ++k) a += Li[k][i] * Li[k][j] / dg[k];
      a *= sc[i] * sc[j];
      Vi[i * 6 + j] = a;
      Vi[j * 6 + i] = a;
    }
  return ok;
}

__global__ __launch_bounds__(256) void k_brdcov_linearize(BrdDims d, const double* __restrict__ cams,
                                                          const double* __restrict__ poses,
                                                          const double* __restrict__ obj,
                                                          const double2* __restrict__ uv,
                                                          const uint8_t* __restrict__ mask, double* __restrict__ Qv,
                                                          double* __restrict__ Vi,
                                                          int32_t* __restrict__ status, double* __restrict__ wr2,
                                                          int32_t* __restrict__ nres) {
  const int b = blockIdx.x;
  __shared__ double s_cam[EXT_MAXC * ACS_CAM_STRIDE];
  __shared__ double s_rp[BRD_MAXNC * 3], s_X[BRD_MAXNC * 3];
  __shared__ double s_part[EXT_MAXC][BC_P];
  __shared__ double s_v[BC_P];
  brd_stage(d, cams, poses + (size_t)b * 12, obj, s_cam, s_rp, s_X);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
  for (int c = wave; c < d.C; c += nwave) {
    const size_t view = (size_t)b * d.C + c;
    double* q = Qv + view * BRD_Q<false>;
    if (!mask[view]) {
      if (lane < BRD_Q<false>) q[lane] = 0.0;
      if (lane < BC_P) s_part[c][lane] = 0.0;
      continue;
    }
    // the 79 sums: nothing between W and V, then sum w r^2
    BrdLaneSums sums{lane};
    brd_view_sums(
        d, s_cam + c * ACS_CAM_STRIDE, s_rp, s_X, uv + view * d.nc, sums, [](const ExtObs&, BrdLaneSums&) {},
        [](const ExtObs& ob, const double[2][6], BrdLaneSums& add) {
          add(ob.w[0] * (ob.r[0] * ob.r[0]) + ob.w[1] * (ob.r[1] * ob.r[1]));
        });
    if (lane < BRD_Q<false>)
      q[lane] = sums.acc0;
    else
      s_part[c][lane - BRD_Q<false>] = sums.acc0;                                    // entries 57..63
    if (lane < BC_P - (64 - BRD_Q<false>)) s_part[c][64 - BRD_Q<false> + lane] = sums.acc1;  // entries 64..78
  }
  __syncthreads();
  if (threadIdx.x < BC_P) {
    double v = 0.0;
    for (int c = 0; c < d.C; ++c) v += s_part[c][threadIdx.x];
    s_v[threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int n_views = 0;
    for (int c = 0; c < d.C; ++c) n_views += mask[(size_t)b * d.C + c] ? 1 : 0;
    double inv[36];
    const bool ok = bc_vinv(s_v + BC_P_V, inv);
    const int st = n_views == 0 ? ACS_COV_NOOBS : (ok ? ACS_COV_OK : ACS_COV_DEGENERATE);
    const bool good = st == ACS_COV_OK;
    double* vi = Vi + (size_t)b * 36;  // zeros for a board that is left out
    for (int k = 0; k < 36; ++k) vi[k] = good ? inv[k] : 0.0;
    status[b] = st;
    wr2[b] = good ? s_v[BC_P_WR2] : 0.0;
    nres[b] = good ? 2 * d.nc * n_views : 0;
  }
}

// chunk partial of S (6C x 6C) over the OK boards of the chunk. Grid (chunks, entry slices): every
// block stages its chunk's V^-1 and W V^-1 tiles and sums its slice of the entries, each entry by
// one thread over the chunk's boards in order.
__global__ __launch_bounds__(256) void k_brdcov_schur(BrdDims d, const double* __restrict__ Qv,
                                                      const double* __restrict__ Vi,
                                                      const int32_t* __restrict__ status,
                                                      const uint8_t* __restrict__ mask, double* __restrict__ part) {
  const int ch = blockIdx.x;
  const int b0 = ch * d.chunk, b1 = min(d.B, b0 + d.chunk), nb = b1 - b0;
  const int NC = 6 * d.C, nE = NC * NC;
  extern __shared__ double lds[];
  double* sZ = lds;                               // nb x C x 36  (W V^-1)
  double* sM = sZ + (size_t)d.chunk * d.C * 36;   // nb x 36
  int* sseen = (int*)(sM + (size_t)d.chunk * 36);  // nb x C: seen by an OK board
  for (int i = threadIdx.x; i < nb * 36; i += blockDim.x) sM[i] = Vi[(size_t)b0 * 36 + i];
  for (int i = threadIdx.x; i < nb * d.C; i += blockDim.x)
    sseen[i] = (mask[(size_t)b0 * d.C + i] && status[b0 + i / d.C] == ACS_COV_OK) ? 1 : 0;
  __syncthreads();
  brd_schur_stage<false>(d, b0, nb, Qv, sseen, sZ, [&](int t) -> const double* { return sM + t * 36; });
  for (int e = blockIdx.y * blockDim.x + threadIdx.x; e < nE; e += gridDim.y * blockDim.x) {
    part[(size_t)ch * nE + e] = brd_schur_entry<false>(d, b0, nb, Qv, sZ, sseen, e / NC, e % NC);
  }
}

struct BcCamArgs {
  int nchunk, gauge, a, pad;
  double s2;
};

__global__ __launch_bounds__(256) void k_brdcov_cams(BrdDims d, BcCamArgs ar, const double* __restrict__ part,
                                                     const double* __restrict__ cams,
                                                     const int32_t* __restrict__ status,
                                                     const double* __restrict__ wr2, const int32_t* __restrict__ nres,
                                                     double* __restrict__ Ag, double* __restrict__ T1,
                                                     double* __restrict__ T2, double* __restrict__ cov,
                                                     acs_sba_boards_cov_report* __restrict__ rep,
                                                     int* __restrict__ bad) {
  const int NC = 6 * d.C, NP = ((NC + 15) / 16) * 16, LD = NP + 1, nE = NC * NC;
  const int tid = threadIdx.x;
  extern __shared__ double lds[];
  const CovCamsLds L = cov_cams_carve(lds, NP);
  // sQ: six columns; s_sm: from 16 (Cm Q)^-1, from 56 its Gauss-Jordan tableau
  double *sS = L.sS, *sQ = L.sQ, *sK = L.sK, *sMC = L.sMC, *sCM = L.sCM, *s_sm = L.s_sm;
  const bool single = d.C == 1;   // one camera is pure gauge: nothing is formed or factored
  const bool anchored = ar.gauge == ACS_GAUGE_ANCHOR;
  const double nan = __builtin_nan("");
  double minp = single ? nan : __builtin_inf();
  bool degenerate = false, gbad = false;  // uniform
  if (!single) {
    cov_cams_sum_chunks(L, NC, NP, ar.nchunk, part, T1);  // 1.
    // 2. gauge generators
    for (int e = tid; e < NP * 8; e += blockDim.x) {
      const int r = e >> 3, k = e & 7;
      double v = 0.0;
      if (r < NC && k < 6) {
        const double* cm = cams + (r / 6) * ACS_CAM_STRIDE;
        const int i = r % 6;
        if (i < 3)
          v = k < 3 ? -cm[8 + 3 * i + k] : 0.0;
        else
          v = k < 3 ? 0.0 : -cm[8 + 3 * (i - 3) + (k - 3)];
      }
      sQ[e] = v;
    }
    __syncthreads();
    double mu;
    degenerate = cov_cams_factor<6>(L, NC, NP, Ag, mu, minp, gbad);  // 3. - 5.
    if (!degenerate) {
      cov_cams_invert<6>(L, NC, NP, mu, Ag, T1, T2, bad);  // 6. - 8.
      if (anchored) {
        // 9. M <- P M P^T, P = I - K Cm, K = Q (Cm Q)^-1, Cm the identity on camera a
        if (tid == 0) {
          // Cm Q (6 x 6) and its inverse by Gauss-Jordan with partial pivoting, [Cm Q | I] (6 x 12) in LDS
          double* A = s_sm + 56;
          for (int k = 0; k < 6; ++k)
            for (int i = 0; i < 6; ++i) {
              A[i * 12 + k] = sQ[(6 * ar.a + i) * 8 + k];
              A[i * 12 + 6 + k] = i == k ? 1.0 : 0.0;
            }
          bool abad = false;
          for (int k = 0; k < 6; ++k) {
            int pv = k;
            for (int i = k + 1; i < 6; ++i)
              if (fabs(A[i * 12 + k]) > fabs(A[pv * 12 + k])) pv = i;
            if (!(fabs(A[pv * 12 + k]) > 1e-12)) {
              abad = true;
              break;
            }
            for (int j = 0; j < 12; ++j) {
              const double x = A[k * 12 + j];
              A[k * 12 + j] = A[pv * 12 + j];
              A[pv * 12 + j] = x;
            }
            const double ip = 1.0 / A[k * 12 + k];
            for (int j = 0; j < 12; ++j) A[k * 12 + j] *= ip;
            for (int i = 0; i < 6; ++i) {
              if (i == k) continue;
              const double f = A[i * 12 + k];
              for (int j = 0; j < 12; ++j) A[i * 12 + j] -= f * A[k * 12 + j];
            }
          }
          for (int i = 0; i < 6; ++i)
            for (int k = 0; k < 6; ++k) s_sm[16 + i * 6 + k] = A[i * 12 + 6 + k];
          s_sm[2] = abad ? 1.0 : 0.0;
        }
        __syncthreads();
        for (int e = tid; e < NC * 8; e += blockDim.x) {
          const int r = e >> 3, k = e & 7;
          double v = 0.0;
          if (k < 6)
            for (int j = 0; j < 6; ++j) v += sQ[r * 8 + j] * s_sm[16 + j * 6 + k];
          sK[e] = v;
        }
        for (int e = tid; e < 6 * NC; e += blockDim.x) {
          const int k = e / NC, c = e % NC;
          sCM[k * NP + c] = sS[(6 * ar.a + k) * LD + c];
        }
        __syncthreads();
        for (int e = tid; e < nE; e += blockDim.x) {
          const int r = e / NC, c = e % NC;
          double v = 0.0;
          for (int k = 0; k < 6; ++k) v += sK[r * 8 + k] * sCM[k * NP + c];
          sS[r * LD + c] -= v;
        }
        __syncthreads();
        for (int e = tid; e < NC * 8; e += blockDim.x) {
          const int r = e >> 3, k = e & 7;
          sMC[e] = k < 6 ? sS[r * LD + 6 * ar.a + k] : 0.0;
        }
        __syncthreads();
        for (int e = tid; e < nE; e += blockDim.x) {
          const int r = e / NC, c = e % NC;
          double v = 0.0;
          for (int k = 0; k < 6; ++k) v += sMC[r * 8 + k] * sK[c * 8 + k];
          sS[r * LD + c] -= v;
        }
        __syncthreads();
        degenerate = s_sm[2] != 0.0;
      }
    }
  } else {
    for (int e = tid; e < NP * LD; e += blockDim.x) sS[e] = 0.0;
    __syncthreads();
  }
  // 10. the symmetric part (the mean of an entry and its transpose: the same bits on both sides),
  //     sigma^2, exact zeros on the anchor camera, NaN when degenerate. The mean, not one triangle:
  //     the refinement step leaves the inverse unsymmetric by ~cond eps, and what one triangle keeps
  //     of that is no perturbation of S; the boards' V^-1 W^T cov_cc W V^-1, a difference of large
  //     terms, multiplies it (measured: 1.4e-9 on a board sd from one triangle)
  for (int e = tid; e < nE; e += blockDim.x) {
    const int r = e / NC, c = e % NC;
    double v = ar.s2 * (0.5 * (sS[r * LD + c] + sS[c * LD + r]));
    if (single || (anchored && (r / 6 == ar.a || c / 6 == ar.a))) v = 0.0;
    cov[e] = degenerate ? nan : v;
  }
  const CovCamsTotals tot = cov_cams_totals(L, NC, NP, ar.s2, anchored ? ar.a : -1, single, d.B, status, wr2, nres);
  if (tid == 0) {
    const long long n_ok = tot.n_ok, dof = tot.n_res - 6 * n_ok - (6 * d.C - 6);
    rep->status = degenerate ? ACS_EXT_COV_DEGENERATE : ACS_EXT_COV_OK;
    rep->reserved = 0;
    rep->n_boards = d.B;
    rep->n_ok = n_ok;
    rep->n_noobs = tot.n_noobs;
    rep->n_degenerate = tot.n_degenerate;
    rep->dof = dof;
    rep->min_pivot = gbad ? 0.0 : minp;
    rep->sigma_hat_px = dof > 0 ? sqrt(tot.wr2 / (double)dof) : nan;
    rep->rot_sd_max = degenerate ? nan : tot.rot_sd_max;
    rep->trans_sd_max = degenerate ? nan : tot.trans_sd_max;
    rep->board_rot_sd_max = nan;  // k_brdcov_board_sd
    rep->board_trans_sd_max = nan;
  }
}

// One wave per board, four boards per block. cov_cc (6C x 6C, sigma^2 applied) is staged in LDS
// (dynamic, behind four 36-double T tiles); lane e < 36 owns entry (e / 6, e % 6).
__global__ __launch_bounds__(256) void k_brdcov_boards(BrdDims d, const double* __restrict__ covc,
                                                       const double* __restrict__ Qv, const double* __restrict__ Vi,
                                                       const int32_t* __restrict__ status,
                                                       const uint8_t* __restrict__ mask, double s2,
                                                       const acs_sba_boards_cov_report* __restrict__ rep,
                                                       double* __restrict__ covb) {
  const int NC = 6 * d.C;
  extern __shared__ double lds[];
  double* s_T = lds;         // 4 x 36
  double* s_cc = lds + 144;  // NC x NC
  for (int i = threadIdx.x; i < NC * NC; i += blockDim.x) s_cc[i] = covc[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * 4 + wave;
  const bool live = b < d.B && lane < 36;
  const bool bok = live && status[b] == ACS_COV_OK;
  const int i = lane / 6, j = lane % 6;
  double acc = 0.0;
  if (bok) {
    const uint8_t* mk = mask + (size_t)b * d.C;
    const double* Wb = Qv + (size_t)b * d.C * BRD_Q<false> + BRD_Q_W;
    for (int c1 = 0; c1 < d.C; ++c1) {
      if (!mk[c1]) continue;
      const double* W1 = Wb + (size_t)c1 * BRD_Q<false>;
      for (int c2 = 0; c2 < d.C; ++c2) {
        if (!mk[c2]) continue;
        const double* W2 = Wb + (size_t)c2 * BRD_Q<false>;
        const double* blk = s_cc + (size_t)(6 * c1) * NC + 6 * c2;
        for (int k = 0; k < 6; ++k) {
          double s = 0.0;
          for (int l = 0; l < 6; ++l) s += blk[k * NC + l] * W2[l * 6 + j];
          acc += W1[k * 6 + i] * s;
        }
      }
    }
  }
  if (lane < 36) s_T[wave * 36 + lane] = acc;
  __syncthreads();
  if (!live || i > j) return;
  const double* vi = Vi + (size_t)b * 36;
  const double* T = s_T + wave * 36;
  double v = 0.0;
  for (int k = 0; k < 6; ++k) {
    double s = 0.0;
    for (int l = 0; l < 6; ++l) s += T[k * 6 + l] * vi[l * 6 + j];
    v += vi[i * 6 + k] * s;
  }
  v += s2 * vi[i * 6 + j];
  if (!(bok && rep->status == ACS_EXT_COV_OK)) v = __builtin_nan("");
  double* o = covb + (size_t)b * 36;
  o[i * 6 + j] = v;  // the upper triangle mirrored
  o[j * 6 + i] = v;
}

// the largest rotation and translation sd over the OK boards (a maximum: any order gives the same bits)
__global__ __launch_bounds__(256) void k_brdcov_board_sd(BrdDims d, const double* __restrict__ covb,
                                                         const int32_t* __restrict__ status,
                                                         acs_sba_boards_cov_report* __restrict__ rep) {
  __shared__ double s_r[256], s_t[256];
  const int tid = threadIdx.x;
  double rs = 0.0, ts = 0.0;
  for (int b = tid; b < d.B; b += blockDim.x) {
    if (status[b] != ACS_COV_OK) continue;
    const double* c = covb + (size_t)b * 36;
    for (int k = 0; k < 3; ++k) {
      rs = fmax(rs, sqrt(c[k * 7]));
      ts = fmax(ts, sqrt(c[(k + 3) * 7]));
    }
  }
  s_r[tid] = rs;
  s_t[tid] = ts;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) {
      s_r[tid] = fmax(s_r[tid], s_r[tid + h]);
      s_t[tid] = fmax(s_t[tid], s_t[tid + h]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    const bool good = rep->status == ACS_EXT_COV_OK && rep->n_ok > 0;
    rep->board_rot_sd_max = good ? s_r[0] : __builtin_nan("");
    rep->board_trans_sd_max = good ? s_t[0] : __builtin_nan("");
  }
}

extern "C" {

int acs_sba_boards_covariance(acs_ctx* ctx, const double* cams, int32_t n_cams, const double* obj_pts,
                              int32_t n_corners, const double* uv, const uint8_t* mask, int32_t n_boards,
                              const double* board_poses, const acs_sba_ext_cov_opts* opts, double* cov_cams,
                              double* cov_boards, int32_t* board_status, acs_sba_boards_cov_report* report,
                              uint32_t flags) {
  ACS_DEVICE_GUARD(ctx);
  ACS_FISHEYE_ONLY(ctx, flags, "acs_sba_boards_covariance");
  acs_sba_ext_cov_opts op;
  acs_sba_ext_cov_default_opts(&op);
  if (opts) op = *opts;
  ACS_CHECK(ctx, n_cams >= 1 && n_cams <= EXT_MAXC, "acs_sba_boards_covariance: n_cams=%d (1..%d)", n_cams, EXT_MAXC);
  ACS_CHECK(ctx, n_corners >= 3 && n_corners <= BRD_MAXNC, "acs_sba_boards_covariance: n_corners=%d (3..%d)",
            n_corners, BRD_MAXNC);
  ACS_CHECK(ctx, n_boards >= 1, "acs_sba_boards_covariance: n_boards=%d (>= 1)", n_boards);
  ACS_CHECK(ctx, op.f_scale > 0 && op.sigma_px > 0, "acs_sba_boards_covariance: f_scale=%g sigma_px=%g (both > 0)",
            op.f_scale, op.sigma_px);
  ACS_CHECK(ctx, op.gauge == ACS_GAUGE_FREE || op.gauge == ACS_GAUGE_ANCHOR, "acs_sba_boards_covariance: gauge %d",
            op.gauge);
  const bool anchored = op.gauge == ACS_GAUGE_ANCHOR;
  if (anchored)
    ACS_CHECK(ctx, op.anchor_cam >= 0 && op.anchor_cam < n_cams, "acs_sba_boards_covariance: anchor_cam=%d (0..%d)",
              op.anchor_cam, n_cams - 1);
  ACS_CHECK(ctx, cams && obj_pts && uv && mask && board_poses && cov_cams, "acs_sba_boards_covariance: null argument");
  hipStream_t s = ctx->stream;
  const BrdDims d = brd_dims(n_boards, n_cams, n_corners, op.f_scale);
  const size_t views = (size_t)n_boards * n_cams;
  int rc;
  void *dcams, *dobj, *duv, *dmask, *dposes;
  if ((rc = acs_stage_in(ctx, WS_CAMS, cams, sizeof(double) * ACS_CAM_STRIDE * n_cams, flags, &dcams))) return rc;
  if ((rc = acs_stage_in(ctx, WS_PTS, obj_pts, sizeof(double) * 3 * n_corners, flags, &dobj))) return rc;
  if ((rc = acs_stage_in(ctx, WS_UV, uv, sizeof(double) * 2 * views * n_corners, flags, &duv))) return rc;
  if ((rc = acs_stage_in(ctx, WS_MASK, mask, views, flags, &dmask))) return rc;
  if ((rc = acs_stage_in(ctx, WS_TMP0, board_poses, sizeof(double) * 12 * n_boards, flags, &dposes))) return rc;
  const uint8_t* mk = (const uint8_t*)dmask;
  const int nchunk = brd_nchunk(d);
  const int NC = 6 * n_cams, NP = ((NC + 15) / 16) * 16, nE = NC * NC;
  double *Qv, *Vi, *wr2, *part, *Ag, *T1, *T2;
  int32_t* nres;
  int* bad;
  auto layout = [&](double* base) {
    Arena a{base};
    Qv = a.take(views * BRD_Q<false>);
    Vi = a.take((size_t)n_boards * 36);
    wr2 = a.take(n_boards);
    nres = a.take<int32_t>(((size_t)n_boards + 1) / 2);
    part = a.take((size_t)nchunk * nE);
    Ag = a.take((size_t)NP * NP);
    T1 = a.take((size_t)NP * NP);
    T2 = a.take((size_t)NP * NP);
    bad = a.take<int>(2);
    return a.bytes();
  };
  const uint32_t ws_flags = flags & ~(uint32_t)ACS_DEVICE_PTRS;  // an output that is not asked for lives in the workspace
  const size_t cb_bytes = sizeof(double) * 36 * (size_t)n_boards, st_bytes = sizeof(int32_t) * (size_t)n_boards;
  double* arena = (double*)acs_ws(ctx, WS_FTE7, layout(nullptr));
  double* dcc = (double*)acs_out_buf(ctx, WS_OUT0, cov_cams, sizeof(double) * nE, flags);
  // the board covariances and statuses are always formed: the report needs them
  double* dcb = (double*)acs_out_buf(ctx, WS_OUT1, cov_boards, cb_bytes, cov_boards ? flags : ws_flags);
  int32_t* dst = (int32_t*)acs_out_buf(ctx, WS_PERPT_I, board_status, st_bytes, board_status ? flags : ws_flags);
  acs_sba_boards_cov_report* drep =
      (acs_sba_boards_cov_report*)acs_ws(ctx, WS_REPORT, sizeof(acs_sba_boards_cov_report));
  if (!arena || !dcc || !dcb || !dst || !drep) return ACS_E_NOMEM;
  layout(arena);
  ACS_HIP(ctx, hipMemsetAsync(bad, 0, sizeof(int), s));
  hipLaunchKernelGGL(k_brdcov_linearize, dim3(n_boards), dim3(256), 0, s, d, (const double*)dcams,
                     (const double*)dposes, (const double*)dobj, (const double2*)duv, mk, Qv, Vi, dst, wr2, nres);
  if (n_cams > 1) {
    const int nslice = acs_grid(nE, 256);  // one entry per thread
    hipLaunchKernelGGL(k_brdcov_schur, dim3(nchunk, nslice), dim3(256), brd_schur_lds(d, 36), s, d, Qv, Vi, dst, mk, part);
  }
  BcCamArgs ar{nchunk, op.gauge, anchored ? op.anchor_cam : 0, 0, op.sigma_px * op.sigma_px};
  hipLaunchKernelGGL(k_brdcov_cams, dim3(1), dim3(256), cov_cams_lds(NP), s, d, ar, part, (const double*)dcams, dst, wr2,
                     nres, Ag, T1, T2, dcc, drep, bad);
  hipLaunchKernelGGL(k_brdcov_boards, dim3(acs_grid(n_boards, 4)), dim3(256), sizeof(double) * (144 + nE), s, d, dcc, Qv,
                     Vi, dst, mk, ar.s2, drep, dcb);
  hipLaunchKernelGGL(k_brdcov_board_sd, dim3(1), dim3(256), 0, s, d, dcb, dst, drep);
  ACS_HIP(ctx, hipGetLastError());
  if ((rc = acs_stage_out(ctx, cov_cams, dcc, sizeof(double) * nE, flags))) return rc;
  if (cov_boards && (rc = acs_stage_out(ctx, cov_boards, dcb, cb_bytes, flags))) return rc;
  if (board_status && (rc = acs_stage_out(ctx, board_status, dst, st_bytes, flags))) return rc;
  if (report) ACS_HIP(ctx, hipMemcpyAsync(report, drep, sizeof(*report), hipMemcpyDeviceToHost, s));
  ACS_HIP(ctx, hipStreamSynchronize(s));
  return ACS_OK;
}

}  // extern "C"
