// sba_boards.hip — bundle adjustment of camera extrinsics AND rigid calibration-board poses
// on gfx950 (acs_sba_boards), with free hand-labelled points in the same solve
// (acs_sba_boards_points, further down). Both entry points are one function, brd_solve: the
// boards-only solve is the mixed one without points. What the linearisation and the Schur partials
// share with the covariance (sba_boards_cov.hip) is in sba_boards.hpp; the LM driver loop is
// ext_lm_loop (sba_ext.hip).
//
// The problem (the one definition; also in include/acinoset_hip.h and tests/sba_boards_ref.py):
//   cameras c = 0..C-1: fisheye records, intrinsics fixed, 1 <= C <= EXT_MAXC
//   boards b = 0..B-1: a pose (R_b, t_b) from board to world coordinates
//   object points p_j, j = 0..nc-1 (3 <= nc <= BRD_MAXNC): any rigid target
//   world point X_bj = R_b p_j + t_b
//   observations uv (B, C, nc, 2), mask (B, C): a view holds all corners of a board or none
//   residual r = project(R_c X_bj + t_c) - uv, cost F = 1/2 f^2 sum log1p(r^2 / f^2),
//   w = 1 / (1 + z), Triggs wh = max((1 - z) w^2, 0.1 w), z = r^2 / f^2
//   left perturbations: R_c <- exp([dw_c]x) R_c, t_c <- t_c + dt_c and the same for (R_b, t_b)
//   J_cam = J_Y [-[R_c X]x | I], J_pt = J_Y R_c (ext_obs_blocks), J_brd = J_pt [-[R_b p_j]x | I]
//   per seen view (b, c), over the nc corners and both image rows:
//     U_bc = sum wh J_cam^T J_cam, W_bc = sum wh J_cam^T J_brd (6 x 6), g_c += sum w r J_cam
//   per board: V_b = sum_views sum wh J_brd^T J_brd, g_b = sum w r J_brd, its cost
// LM: the spec of oracle/sba_ext.py with "point" read as "board". Marquardt damping on every
// diagonal, M_b = (V_b + lam diag V_b + 1e-300 I)^-1 (6 x 6 Cholesky),
//   S = sum U + lam D - sum_b sum_{c1,c2} W_bc1 M_b W_bc2^T,  b = -g_c + sum W M g_b,
//   db = -M_b (g_b + sum_c W_bc^T dc); accept iff F_new < F (lam /= 10, floor EXT_LAM_MIN), else
//   lam *= 10; stop on gtol, ftol, xtol, lam > 1e16, max_iters; |d|^2 = sum dc^2 + sum db^2,
//   |x|^2 = sum |t_c|^2 + sum |t_b|^2.
// A board whose damped V_b is not positive definite (no view, a NaN, a pivot not > 0) takes no
// step in that iteration (M_b = 0); its views still count in U and g_c. The 6-DoF rigid gauge
// is left free and resolved by the damping floor.
//
//   k_brd_linearize [1 block of 4 waves per board] waves strided over the cameras, lanes over the
//                   corners (brd_stage, brd_view_sums; sba_boards.hpp); ext_obs_blocks per corner;
//                   every sum is a group_sum over the wave (rounds of 64 corners in order) kept by
//                   the lane that owns the entry; the view record U (21), W (36), g_c (6) and,
//                   summed over the views in camera order, the board record V (21), g_b (6), F. No
//                   floating-point atomics.
//   k_brd_schur     [board chunks x entry slices] M_b, the W M tiles (36 doubles per view) in LDS
//                   (brd_schur_stage), fixed-order chunk partials [S | b | diag U | g_c] in
//                   k_ext_solve's layout (S by brd_schur_entry); per board max |g_b| for
//                   k_ext_solve's slots argument
//   k_ext_solve     (sba_ext.hip, unchanged) camera step
//   k_brd_back      [boards] board steps db and the norm partials
//   k_brd_pose      [boards] trial board poses on SO(3) (EXT_EXP_SO3, as k_ext_cam)
//   k_ext_cam       (sba_ext.hip, unchanged) trial cameras
//   k_brd_cost      [1 block per board] robust cost at the trial state, views in camera order
//   k_ext_lm        (sba_ext.hip, unchanged) accept / reject, lambda, stop tests
#include <algorithm>

#include "sba_boards.hpp"

// the board record; the view record is BRD_Q<true> (sba_boards.hpp)
enum : int { BRD_V_V = 0, BRD_V_G = 21, BRD_V_F = 27, BRD_V = 28 };
// M_b (36, row-major) and whether the board steps (1.0 / 0.0)
enum : int { BRD_M_OK = 36, BRD_M = 37 };

__global__ __launch_bounds__(256) void k_brd_linearize(BrdDims d, const ExtState* __restrict__ st,
                                                       const double* __restrict__ camsbuf,
                                                       const double* __restrict__ posebuf,
                                                       const double* __restrict__ obj,
                                                       const double2* __restrict__ uv,
                                                       const uint8_t* __restrict__ mask, double* __restrict__ Qv,
                                                       double* __restrict__ Vb) {
  if (st->status != 0 || !st->relin) return;
  const int cur = st->cur, b = blockIdx.x;
  __shared__ double s_cam[EXT_MAXC * ACS_CAM_STRIDE];
  __shared__ double s_rp[BRD_MAXNC * 3], s_X[BRD_MAXNC * 3];
  __shared__ double s_part[EXT_MAXC][BRD_V];
  brd_stage(d, camsbuf + cur * d.C * ACS_CAM_STRIDE, posebuf + ((size_t)cur * d.B + b) * 12, obj, s_cam, s_rp, s_X);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
  for (int c = wave; c < d.C; c += nwave) {
    const size_t view = (size_t)b * d.C + c;
    double* q = Qv + view * BRD_Q<true>;
    if (!mask[view]) {
      if (lane < BRD_Q<true>) q[lane] = 0.0;
      if (lane < BRD_V) s_part[c][lane] = 0.0;
      continue;
    }
    // the 91 sums: g_c (6) between W and V, then g_b (6) and the cost
    BrdLaneSums sums{lane};
    brd_view_sums(
        d, s_cam + c * ACS_CAM_STRIDE, s_rp, s_X, uv + view * d.nc, sums,
        [](const ExtObs& ob, BrdLaneSums& add) {
          const double wr0 = ob.w[0] * ob.r[0], wr1 = ob.w[1] * ob.r[1];
#pragma unroll
          for (int i = 0; i < 6; ++i) add(wr0 * ob.jc[0][i] + wr1 * ob.jc[1][i]);
        },
        [&](const ExtObs& ob, const double jb[2][6], BrdLaneSums& add) {
          const double wr0 = ob.w[0] * ob.r[0], wr1 = ob.w[1] * ob.r[1];
#pragma unroll
          for (int i = 0; i < 6; ++i) add(wr0 * jb[0][i] + wr1 * jb[1][i]);
          add(0.5 * d.f2 * (log1p(ob.z[0]) + log1p(ob.z[1])));
        });
    if (lane < BRD_Q<true>) q[lane] = sums.acc0;
    if (lane == 63) s_part[c][0] = sums.acc0;
    if (lane < BRD_V - 1) s_part[c][1 + lane] = sums.acc1;
  }
  __syncthreads();
  if (threadIdx.x < BRD_V) {
    double v = 0.0;
    for (int c = 0; c < d.C; ++c) v += s_part[c][threadIdx.x];
    Vb[(size_t)b * BRD_V + threadIdx.x] = v;
  }
}

// damped board block inverse M = (V + lam diag V + 1e-300 I)^-1 by Cholesky, V packed upper
// (upk), M row-major; false (M = 0) when a pivot is not > 0 (no view, a NaN)
__device__ __forceinline__ bool board_minv(const double* V, double lam, double M[36]) {
  double L[6][6], Li[6][6];
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double a = V[upk(j, i)];
      if (i == j) a = a * (1.0 + lam) + 1e-300;
#pragma unroll
      for (int k = 0; k < j; ++k) a -= L[i][k] * L[j][k];
      if (i == j) {
        ok = ok && (a > 0.0);
        L[i][i] = sqrt(a);
      } else {
        L[i][j] = a / L[j][j];
      }
    }
  }
  if (!ok) {
    for (int k = 0; k < 36; ++k) M[k] = 0.0;
    return false;
  }
  // Li = L^-1 (lower), M = Li^T Li
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    Li[j][j] = 1.0 / L[j][j];
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double a = 0.0;
#pragma unroll
      for (int k = j; k < i; ++k) a -= L[i][k] * Li[k][j];
      Li[i][j] = a / L[i][i];
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i; j < 6; ++j) {
      double a = 0.0;
#pragma unroll
      for (int k = j; k < 6; ++k) a += Li[k][i] * Li[k][j];
      M[i * 6 + j] = a;
      M[j * 6 + i] = a;
    }
  return true;
}

// entries of a chunk partial, k_ext_solve's layout: S (6C x 6C), b (6C), U diagonal (6C), g_c (6C).
// Grid (chunks, entry slices): every block stages its chunk's M_b and W M tiles and sums its slice
// of the entries, each entry by one thread over the chunk's boards in order.
__global__ __launch_bounds__(256) void k_brd_schur(BrdDims d, const ExtState* __restrict__ st,
                                                   const double* __restrict__ Qv, const double* __restrict__ Vb,
                                                   const uint8_t* __restrict__ mask, double* __restrict__ Mb,
                                                   double* __restrict__ gslot, double* __restrict__ part) {
  if (st->status != 0) return;
  const int ch = blockIdx.x;
  const int b0 = ch * d.chunk, b1 = min(d.B, b0 + d.chunk), nb = b1 - b0;
  const int NC = 6 * d.C, nE = NC * NC + 3 * NC;
  const double lam = st->lam;
  extern __shared__ double lds[];
  double* sZ = lds;                               // nb x C x 36  (W M)
  double* sM = sZ + (size_t)d.chunk * d.C * 36;   // nb x BRD_M
  double* sg = sM + (size_t)d.chunk * BRD_M;      // nb x 6 (g_b)
  int* sseen = (int*)(sg + d.chunk * 6);          // nb x C
  for (int t = threadIdx.x; t < nb; t += blockDim.x) {
    const double* vb = Vb + (size_t)(b0 + t) * BRD_V;
    double M[36];
    int n_views = 0;
    for (int c = 0; c < d.C; ++c) n_views += mask[(size_t)(b0 + t) * d.C + c] ? 1 : 0;
    bool ok = board_minv(vb + BRD_V_V, lam, M);
    if (n_views == 0) {  // a board without a view: no step (its V is zero, the pivots 1e-300)
      ok = false;
      for (int k = 0; k < 36; ++k) M[k] = 0.0;
    }
    for (int k = 0; k < 36; ++k) sM[t * BRD_M + k] = M[k];
    sM[t * BRD_M + BRD_M_OK] = ok ? 1.0 : 0.0;
    double gm = 0.0;
    for (int k = 0; k < 6; ++k) {
      sg[t * 6 + k] = vb[BRD_V_G + k];
      gm = fmax(gm, fabs(vb[BRD_V_G + k]));
    }
    if (blockIdx.y == 0) {  // every block of the chunk stages the same M_b: the first one keeps it
      double* mb = Mb + (size_t)(b0 + t) * BRD_M;
      for (int k = 0; k < BRD_M; ++k) mb[k] = sM[t * BRD_M + k];
      gslot[b0 + t] = gm;
    }
  }
  for (int i = threadIdx.x; i < nb * d.C; i += blockDim.x) sseen[i] = mask[(size_t)b0 * d.C + i];
  __syncthreads();
  brd_schur_stage<true>(d, b0, nb, Qv, sseen, sZ, [&](int t) -> const double* {
    return sM[t * BRD_M + BRD_M_OK] != 0.0 ? sM + t * BRD_M : nullptr;
  });
  for (int e = blockIdx.y * blockDim.x + threadIdx.x; e < nE; e += gridDim.y * blockDim.x) {
    double acc = 0.0;
    if (e < NC * NC) {
      acc = brd_schur_entry<true>(d, b0, nb, Qv, sZ, sseen, e / NC, e % NC);
    } else {
      const int r = e - NC * NC, kind = r / NC, a = r % NC, c1 = a / 6, k1 = a % 6;
      for (int t = 0; t < nb; ++t) {
        if (!sseen[t * d.C + c1]) continue;
        const double* q = Qv + ((size_t)(b0 + t) * d.C + c1) * BRD_Q<true>;
        if (kind == 0) {  // b = -g_c + Z g_b
          const double* z = sZ + ((size_t)t * d.C + c1) * 36 + k1 * 6;
          double s = 0.0;
          for (int k = 0; k < 6; ++k) s += z[k] * sg[t * 6 + k];
          acc += -q[BRD_Q_GC + k1] + s;
        } else if (kind == 1) {  // U diagonal
          acc += q[BRD_Q_U + upk(k1, k1)];
        } else {  // g_c
          acc += q[BRD_Q_GC + k1];
        }
      }
    }
    part[(size_t)ch * nE + e] = acc;
  }
}

// db = -M_b (g_b + sum_c W_bc^T dc), zero for a board that takes no step; |db|^2 and |t_b|^2
__global__ __launch_bounds__(256) void k_brd_back(BrdDims d, const ExtState* __restrict__ st,
                                                  const double* __restrict__ Qv, const double* __restrict__ Vb,
                                                  const double* __restrict__ Mb, const uint8_t* __restrict__ mask,
                                                  const double* __restrict__ dc, const double* __restrict__ posebuf,
                                                  double* __restrict__ db, double* __restrict__ normp) {
  if (st->status != 0) return;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= d.B) return;
  const double* M = Mb + (size_t)b * BRD_M;
  const double* t = posebuf + ((size_t)st->cur * d.B + b) * 12 + 9;
  double acc[6];
  for (int k = 0; k < 6; ++k) acc[k] = Vb[(size_t)b * BRD_V + BRD_V_G + k];
  for (int c = 0; c < d.C; ++c) {
    if (!mask[(size_t)b * d.C + c]) continue;
    const double* W = Qv + ((size_t)b * d.C + c) * BRD_Q<true> + BRD_Q_W;
    for (int k = 0; k < 6; ++k)
      for (int i = 0; i < 6; ++i) acc[k] += W[i * 6 + k] * dc[6 * c + i];
  }
  const bool ok = M[BRD_M_OK] != 0.0;
  double dn = 0.0;
  for (int k = 0; k < 6; ++k) {
    double v = 0.0;
    for (int i = 0; i < 6; ++i) v -= M[k * 6 + i] * acc[i];
    if (!ok) v = 0.0;
    db[(size_t)b * 6 + k] = v;
    dn += v * v;
  }
  normp[2 * b] = dn;
  normp[2 * b + 1] = t[0] * t[0] + t[1] * t[1] + t[2] * t[2];
}

// trial board poses R <- exp([dw]x) R, t <- t + dt
__global__ __launch_bounds__(256) void k_brd_pose(BrdDims d, const ExtState* __restrict__ st,
                                                  const double* __restrict__ db, double* __restrict__ posebuf) {
  if (st->status != 0) return;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= d.B) return;
  const int cur = st->cur;
  const double* pm = posebuf + ((size_t)cur * d.B + b) * 12;
  double* pn = posebuf + ((size_t)(cur ^ 1) * d.B + b) * 12;
  const double* s = db + (size_t)b * 6;
  const double w0 = s[0], w1 = s[1], w2 = s[2];
  EXT_EXP_SO3(E, w0, w1, w2)
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) pn[i * 3 + j] = E[i * 3] * pm[j] + E[i * 3 + 1] * pm[3 + j] + E[i * 3 + 2] * pm[6 + j];
    pn[9 + i] = pm[9 + i] + s[3 + i];
  }
}

// robust cost per board: which = 0 at the current state, 1 at the trial
__global__ __launch_bounds__(256) void k_brd_cost(BrdDims d, const ExtState* __restrict__ st, int which,
                                                  const double* __restrict__ camsbuf,
                                                  const double* __restrict__ posebuf,
                                                  const double* __restrict__ obj, const double2* __restrict__ uv,
                                                  const uint8_t* __restrict__ mask, double* __restrict__ Fp) {
  if (which == 1 && st->status != 0) return;
  const int buf = which == 1 ? (st->cur ^ 1) : st->cur, b = blockIdx.x;
  __shared__ double s_cam[EXT_MAXC * ACS_CAM_STRIDE];
  __shared__ double s_rp[BRD_MAXNC * 3], s_X[BRD_MAXNC * 3];
  __shared__ double s_f[EXT_MAXC];
  brd_stage(d, camsbuf + buf * d.C * ACS_CAM_STRIDE, posebuf + ((size_t)buf * d.B + b) * 12, obj, s_cam, s_rp, s_X);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
  for (int c = wave; c < d.C; c += nwave) {
    const size_t view = (size_t)b * d.C + c;
    double F = 0.0;
    if (mask[view]) {
      for (int j = lane; j < d.nc; j += 64) {
        ProjOut po;
        fisheye_project<false>(s_cam + c * ACS_CAM_STRIDE, s_X[3 * j], s_X[3 * j + 1], s_X[3 * j + 2], po);
        const double2 m = uv[view * d.nc + j];
        const double ru = po.u - m.x, rv = po.v - m.y;
        F += 0.5 * d.f2 * (log1p(ru * ru / d.f2) + log1p(rv * rv / d.f2));
      }
      F = group_sum<64>(F);
    }
    if (lane == 0) s_f[c] = F;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double f = 0.0;
    for (int c = 0; c < d.C; ++c) f += s_f[c];
    Fp[b] = f;
  }
}

// voff[view] = number of seen views before it, by one block
__global__ __launch_bounds__(256) void k_brd_offsets(int n_views, const uint8_t* __restrict__ mask,
                                                     int* __restrict__ voff) {
  __shared__ int s_cnt[256];
  const int per = (n_views + 255) / 256, v0 = min(n_views, (int)threadIdx.x * per), v1 = min(n_views, v0 + per);
  int n = 0;
  for (int v = v0; v < v1; ++v) n += mask[v] ? 1 : 0;
  s_cnt[threadIdx.x] = n;
  __syncthreads();
  int base = 0;
  for (int t = 0; t < (int)threadIdx.x; ++t) base += s_cnt[t];
  for (int v = v0; v < v1; ++v) {
    voff[v] = base;
    base += mask[v] ? 1 : 0;
  }
}

// residuals of the seen views in (board, camera, corner, row) order
__global__ __launch_bounds__(256) void k_brd_resid(BrdDims d, const double* __restrict__ cams,
                                                   const double* __restrict__ poses, const double* __restrict__ obj,
                                                   const double2* __restrict__ uv, const uint8_t* __restrict__ mask,
                                                   const int* __restrict__ voff, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)d.B * d.C * d.nc) return;
  const int64_t view = i / d.nc;
  const int j = (int)(i % d.nc), b = (int)(view / d.C), c = (int)(view % d.C);
  if (!mask[view]) return;
  const double p[3] = {obj[3 * j], obj[3 * j + 1], obj[3 * j + 2]};
  double rp[3], X[3];
  brd_world(poses + (size_t)b * 12, p, rp, X);
  ProjOut po;
  fisheye_project<false>(cams + c * ACS_CAM_STRIDE, X[0], X[1], X[2], po);
  const double2 m = uv[i];
  double* o = out + ((size_t)voff[view] * d.nc + j) * 2;
  o[0] = po.u - m.x;
  o[1] = po.v - m.y;
}

// =======================================================================================
// Rigid boards with free (hand-labelled) points in the same solve (acs_sba_boards_points).
//
// The problem (the one definition; also in include/acinoset_hip.h and tests/sba_boards_points_ref.py):
//   everything of acs_sba_boards above, and free points X_p, p = 0..n-1, stored densely:
//   pt_uv (n, C, 2), pt_mask (n, C): a camera sees a point at most once (slot = camera, K = C in the
//   terms of sba_ext.hip). The same Cauchy cost and Triggs weights for every residual:
//   F = F_boards + F_points; U and g_c of a camera sum over its board views and its point
//   observations. One LM, the spec of oracle/sba_ext.py and of the solve above joined: Marquardt
//   damping on every diagonal, M_b as above, M_p = (V_p + lam diag V_p + 1e-300 I)^-1 (point_minv),
//     S = sum U + lam D - sum_b W M_b W^T - sum_p W M_p W^T,
//     b = -g_c + sum_b W M_b g_b + sum_p W M_p g_p,
//   db and dX by back-substitution, gmax = max(|g_c|, |g_b|, |g_p|),
//   |d|^2 = sum dc^2 + sum db^2 + sum dX^2, |x|^2 = sum |t_c|^2 + sum |t_b|^2 + sum |X_p|^2;
//   accept / reject, the lambda schedule, EXT_LAM_MIN, the stop tests and the status codes as above.
//   A point without an observation takes no step and contributes nothing (point_minv's rule); a
//   board without a view behaves as above. The 6-DoF rigid gauge stays free.
//
// One iteration: k_brd_linearize, k_ext_linearize; k_brd_schur, k_ext_schur; k_ext_solve;
// k_brd_back, k_ext_back; k_brd_pose, k_ext_cam; k_brd_cost, k_ext_cost; k_ext_lm. The point side is
// sba_ext.hip's kernels on the dense slots (ext_launch_*), with ext_dims(n, C, C, f_scale). The two
// sides meet in flat buffers: part holds the board chunks, then the point chunks; Fp and normp the
// boards, then the points (k_ext_lm sums B + n entries); one ExtState, dc, Sg, bad, camnorm and
// camera double buffer. Device code of its own is what the dense form needs: the camera-id table and
// the residuals of the seen observations. Without points (n = 0) the point launches fall away and what
// is left is acs_sba_boards, bit for bit: the one host path below (brd_solve) serves both.
// =======================================================================================

// camid[p C + c] = c: the dense slots' camera ids
__global__ __launch_bounds__(256) void k_bpt_camid(int64_t n_slots, int C, uint8_t* __restrict__ camid) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_slots) camid[i] = (uint8_t)(i % C);
}

// residuals of the seen (point, camera) pairs in (point, camera, row) order, behind the board part:
// that part's length comes from the boards' offsets (k_brd_offsets), where the mask lives
__global__ __launch_bounds__(256) void k_bpt_resid(int64_t n_slots, int C, int64_t views, int nc,
                                                   const double* __restrict__ cams, const double* __restrict__ pts,
                                                   const double2* __restrict__ uv, const uint8_t* __restrict__ mask,
                                                   const int* __restrict__ poff, const uint8_t* __restrict__ bmask,
                                                   const int* __restrict__ voff, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_slots || !mask[i]) return;
  const int64_t p = i / C;
  const int c = (int)(i % C);
  const size_t base = ((size_t)voff[views - 1] + (bmask[views - 1] ? 1 : 0)) * nc;
  ProjOut po;
  fisheye_project<false>(cams + c * ACS_CAM_STRIDE, pts[3 * p], pts[3 * p + 1], pts[3 * p + 2], po);
  const double2 m = uv[i];
  double* o = out + (base + poff[i]) * 2;
  o[0] = po.u - m.x;
  o[1] = po.v - m.y;
}

// ---------------------------------------------------------------------------------------
// The device buffers of one solve, one allocation: the boards', with part, Fp and normp long enough
// for both sides, and the points' behind them (empty without points).
struct BrdBuffers {
  double *cams, *poses;  // the current and the trial state: [2][C] records, [2][B][12]
  double *Qv, *Vb, *Mb, *gslot, *Fp, *part, *dc, *Sg, *db, *normp, *camnorm;
  ExtState* st;
  int *bad, *voff;
  double *pts, *Q, *Vg;  // [2][n][3], the slot records, the point blocks
  uint8_t* cid;
  int* poff;
  int nchunk, nchunk_p;
};

// the buffers at base; with a null base only the size in bytes (Arena)
static size_t brd_layout(BrdBuffers& b, double* base, const BrdDims& d, const ExtDims& dp) {
  const size_t B = d.B, NC = 6 * d.C, views = B * d.C, n = dp.n, slots = n * d.C;
  Arena a{base};
  b.nchunk = brd_nchunk(d);
  b.nchunk_p = n ? ext_nchunk(dp) : 0;
  b.cams = a.take(2 * (size_t)d.C * ACS_CAM_STRIDE);
  b.poses = a.take(2 * B * 12);
  b.Qv = a.take(views * BRD_Q<true>);
  b.Vb = a.take(B * BRD_V);
  b.Mb = a.take(B * BRD_M);
  b.gslot = a.take(B);
  b.Fp = a.take(B + n);
  b.part = a.take((b.nchunk + b.nchunk_p) * (NC * NC + 3 * NC));
  b.dc = a.take(96);
  b.Sg = a.take(96 * 96);
  b.db = a.take(6 * B);
  b.normp = a.take(2 * (B + n));
  b.camnorm = a.take(64);
  b.st = a.take<ExtState>(16);
  b.bad = a.take<int>(2);
  b.voff = a.take<int>((views + 1) / 2);
  b.pts = a.take(6 * n);
  b.Q = a.take(slots * EXT_Q<true>);
  b.Vg = a.take(n * 10);
  b.cid = a.take<uint8_t>((slots + 7) / 8);
  b.poff = a.take<int>((slots + 1) / 2);
  return a.bytes();
}

// the problem's device arrays: the boards', and the point slots as the kernels of sba_ext.hip take them
struct BrdInputs {
  const double* obj;
  const double2* uv;
  const uint8_t* mask;
  const double2* pt_uv;
  const uint8_t* pt_mask;
};

// the robust cost per board and per point: which = 0 at the current state, 1 at the trial
static void brd_launch_cost(hipStream_t s, const BrdDims& d, const ExtDims& dp, const BrdBuffers& b, const BrdInputs& in,
                            int which) {
  hipLaunchKernelGGL(k_brd_cost, dim3(d.B), dim3(256), 0, s, d, b.st, which, b.cams, b.poses, in.obj, in.uv, in.mask,
                     b.Fp);
  if (dp.n > 0) ext_launch_point_cost(s, dp, b.st, which, b.cams, b.pts, in.pt_uv, in.pt_mask, b.cid, b.Fp + d.B);
}

// one LM iteration; dp: the points' dimensions (n = 0: the board kernels alone), de carries
// (B + n, C) to k_ext_solve / k_ext_cam / k_ext_lm
static void brd_enqueue(hipStream_t s, const BrdDims& d, const ExtDims& dp, const ExtDims& de, const ExtOpts& o,
                        const BrdBuffers& b, const BrdInputs& in) {
  const int bgrid = acs_grid(d.B, 256), NC = 6 * d.C, nE = NC * NC + 3 * NC;
  const bool pts = dp.n > 0;
  hipLaunchKernelGGL(k_brd_linearize, dim3(d.B), dim3(256), 0, s, d, b.st, b.cams, b.poses, in.obj, in.uv, in.mask, b.Qv,
                     b.Vb);
  if (pts) ext_launch_linearize(s, dp, b.st, b.cams, b.pts, in.pt_uv, in.pt_mask, b.cid, b.Q, b.Vg, b.Fp + d.B);
  const int nslice = acs_grid(nE, 256);  // one entry per thread
  hipLaunchKernelGGL(k_brd_schur, dim3(b.nchunk, nslice), dim3(256), brd_schur_lds(d, BRD_M + 6), s, d, b.st, b.Qv, b.Vb,
                     in.mask, b.Mb, b.gslot, b.part);
  if (pts) ext_launch_schur(s, dp, b.st, b.Q, b.Vg, in.pt_mask, b.cid, b.part + (size_t)b.nchunk * nE);
  ext_launch_solve(s, de, b.st, b.part, b.nchunk + b.nchunk_p, pts ? b.Vg : nullptr, dp.n, b.gslot, d.B, b.dc, b.Sg,
                   b.bad);
  hipLaunchKernelGGL(k_brd_back, dim3(bgrid), dim3(256), 0, s, d, b.st, b.Qv, b.Vb, b.Mb, in.mask, b.dc, b.poses, b.db,
                     b.normp);
  if (pts) ext_launch_back(s, dp, b.st, b.Q, b.Vg, in.pt_mask, b.cid, b.dc, b.pts, b.normp + 2 * (size_t)d.B);
  hipLaunchKernelGGL(k_brd_pose, dim3(bgrid), dim3(256), 0, s, d, b.st, b.db, b.poses);
  ext_launch_cam(s, de, b.st, b.dc, b.cams, b.camnorm);
  brd_launch_cost(s, d, dp, b, in, 1);
  ext_launch_lm(s, de, b.st, o, 0, b.Fp, b.normp, b.camnorm);
}

// The solve behind acs_sba_boards (null point arrays, n_pts = 0) and acs_sba_boards_points; fn names
// the entry point in the error texts. Every check comes before anything is staged or allocated.
static int brd_solve(acs_ctx* ctx, const char* fn, double* cams, int32_t n_cams, const double* obj_pts,
                     int32_t n_corners, const double* uv, const uint8_t* mask, int32_t n_boards, double* board_poses,
                     const double* pt_uv, const uint8_t* pt_mask, int32_t n_pts, double* pts,
                     const acs_sba_ext_opts* opts, double* resid_before, double* resid_after,
                     acs_sba_ext_report* report, uint32_t flags) {
  acs_sba_ext_opts op;
  acs_sba_ext_default_opts(&op);
  if (opts) op = *opts;
  ACS_CHECK(ctx, n_cams >= 1 && n_cams <= EXT_MAXC, "%s: n_cams=%d (1..%d)", fn, n_cams, EXT_MAXC);
  ACS_CHECK(ctx, n_corners >= 3 && n_corners <= BRD_MAXNC, "%s: n_corners=%d (3..%d)", fn, n_corners, BRD_MAXNC);
  ACS_CHECK(ctx, n_boards >= 1, "%s: n_boards=%d (>= 1)", fn, n_boards);
  ACS_CHECK(ctx, n_pts >= 0 && (int64_t)n_pts * n_cams < (int64_t)INT32_MAX, "%s: n_pts=%d (>= 0, n_pts n_cams < 2^31)",
            fn, n_pts);
  ACS_CHECK(ctx, op.f_scale > 0, "%s: f_scale=%g (> 0)", fn, op.f_scale);
  ACS_CHECK(ctx, cams && obj_pts && uv && mask && board_poses, "%s: null array", fn);
  ACS_CHECK(ctx, n_pts == 0 || (pt_uv && pt_mask && pts), "%s: null point array with n_pts=%d", fn, n_pts);
  hipStream_t s = ctx->stream;
  const BrdDims d = brd_dims(n_boards, n_cams, n_corners, op.f_scale);
  const ExtDims dp = ext_dims(n_pts, n_cams, n_cams, op.f_scale);
  const ExtDims de{n_boards + n_pts, 1, n_cams, 2, 1, d.f2};
  const size_t views = (size_t)n_boards * n_cams, slots = (size_t)n_pts * n_cams;
  const size_t cam_bytes = sizeof(double) * ACS_CAM_STRIDE * n_cams, pose_bytes = sizeof(double) * 12 * n_boards;
  const size_t pts_bytes = sizeof(double) * 3 * n_pts;
  int rc;
  void *dcams, *dobj, *duv, *dmask, *dposes, *dpuv = nullptr, *dpmask = nullptr, *dpts = nullptr;
  if ((rc = acs_stage_in(ctx, WS_CAMS, cams, cam_bytes, flags, &dcams))) return rc;
  if ((rc = acs_stage_in(ctx, WS_PTS, obj_pts, sizeof(double) * 3 * n_corners, flags, &dobj))) return rc;
  if ((rc = acs_stage_in(ctx, WS_UV, uv, sizeof(double) * 2 * views * n_corners, flags, &duv))) return rc;
  if ((rc = acs_stage_in(ctx, WS_MASK, mask, views, flags, &dmask))) return rc;
  if ((rc = acs_stage_in(ctx, WS_TMP0, board_poses, pose_bytes, flags, &dposes))) return rc;
  if (n_pts > 0) {  // the dense arrays are the slot tensor: slots of their own, beside the boards'
    if ((rc = acs_stage_in(ctx, WS_TMP1, pt_uv, sizeof(double) * 2 * slots, flags, &dpuv))) return rc;
    if ((rc = acs_stage_in(ctx, WS_TMP2, pt_mask, slots, flags, &dpmask))) return rc;
    if ((rc = acs_stage_in(ctx, WS_TMP3, pts, pts_bytes, flags, &dpts))) return rc;
  }
  const BrdInputs in{(const double*)dobj, (const double2*)duv, (const uint8_t*)dmask, (const double2*)dpuv,
                     (const uint8_t*)dpmask};
  BrdBuffers b;
  double* arena = (double*)acs_ws(ctx, WS_FTE6, brd_layout(b, nullptr, d, dp));
  if (!arena) return ACS_E_NOMEM;
  brd_layout(b, arena, d, dp);
  // the residual vectors' length: the seen views and point observations, counted where the masks live
  size_t n_res = 0;
  const int64_t n_thr = (int64_t)views * n_corners;
  if (resid_before || resid_after) {
    hipLaunchKernelGGL(k_brd_offsets, dim3(1), dim3(256), 0, s, (int)views, in.mask, b.voff);
    if (n_pts > 0) hipLaunchKernelGGL(k_brd_offsets, dim3(1), dim3(256), 0, s, (int)slots, in.pt_mask, b.poff);
    if (!(flags & ACS_DEVICE_PTRS)) {  // with device pointers the caller's arrays hold them all
      for (size_t v = 0; v < views; ++v) n_res += mask[v] ? n_corners : 0;
      for (size_t v = 0; v < slots; ++v) n_res += pt_mask[v] ? 1 : 0;
    }
  }
  const size_t res_bytes = sizeof(double) * 2 * n_res;
  for (int k = 0; k < 2; ++k) {
    ACS_HIP(ctx, hipMemcpyAsync(b.cams + k * n_cams * ACS_CAM_STRIDE, dcams, cam_bytes, hipMemcpyDeviceToDevice, s));
    ACS_HIP(ctx, hipMemcpyAsync(b.poses + (size_t)k * n_boards * 12, dposes, pose_bytes, hipMemcpyDeviceToDevice, s));
    if (n_pts > 0)
      ACS_HIP(ctx, hipMemcpyAsync(b.pts + (size_t)k * n_pts * 3, dpts, pts_bytes, hipMemcpyDeviceToDevice, s));
  }
  if (n_pts > 0) hipLaunchKernelGGL(k_bpt_camid, dim3(acs_grid(slots, 256)), dim3(256), 0, s, (int64_t)slots, n_cams, b.cid);
  ACS_HIP(ctx, hipMemsetAsync(b.bad, 0, sizeof(int), s));
  ExtState hs;
  std::memset(&hs, 0, sizeof(hs));
  hs.lam = op.lambda0;
  hs.relin = 1;
  ACS_HIP(ctx, hipMemcpyAsync(b.st, &hs, sizeof(hs), hipMemcpyHostToDevice, s));
  auto resid = [&](const double* c, const double* poses, const double* x, double* out) {
    hipLaunchKernelGGL(k_brd_resid, dim3(acs_grid(n_thr, 256)), dim3(256), 0, s, d, c, poses, in.obj, in.uv, in.mask,
                       b.voff, out);
    if (n_pts > 0)
      hipLaunchKernelGGL(k_bpt_resid, dim3(acs_grid(slots, 256)), dim3(256), 0, s, (int64_t)slots, n_cams,
                         (int64_t)views, n_corners, c, x, in.pt_uv, in.pt_mask, b.poff, in.mask, b.voff, out);
  };
  double* drb = nullptr;
  if (resid_before) {
    drb = (double*)acs_out_buf(ctx, WS_OUT0, resid_before, res_bytes, flags);
    if (!drb) return ACS_E_NOMEM;
    resid(b.cams, b.poses, b.pts, drb);
  }
  ExtOpts o{op.max_iters, op.ftol, op.xtol, op.gtol};
  brd_launch_cost(s, d, dp, b, in, 0);
  ext_launch_lm(s, de, b.st, o, 1, b.Fp, b.normp, b.camnorm);
  ACS_HIP(ctx, hipGetLastError());
  if ((rc = ext_lm_loop(ctx, b.st, op.max_iters, [&] { brd_enqueue(s, d, dp, de, o, b, in); }, &hs))) return rc;
  const double* fcams = b.cams + hs.cur * n_cams * ACS_CAM_STRIDE;
  const double* fposes = b.poses + (size_t)hs.cur * n_boards * 12;
  const double* fpts = b.pts + (size_t)hs.cur * n_pts * 3;
  const hipMemcpyKind kout = (flags & ACS_DEVICE_PTRS) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (resid_after) {
    double* dra = (double*)acs_out_buf(ctx, WS_OUT1, resid_after, res_bytes, flags);
    if (!dra) return ACS_E_NOMEM;
    resid(fcams, fposes, fpts, dra);
    ACS_HIP(ctx, hipGetLastError());
    if ((rc = acs_stage_out(ctx, resid_after, dra, res_bytes, flags))) return rc;
  }
  if (resid_before && (rc = acs_stage_out(ctx, resid_before, drb, res_bytes, flags))) return rc;
  ACS_HIP(ctx, hipMemcpyAsync(cams, fcams, cam_bytes, kout, s));
  ACS_HIP(ctx, hipMemcpyAsync(board_poses, fposes, pose_bytes, kout, s));
  if (n_pts > 0) ACS_HIP(ctx, hipMemcpyAsync(pts, fpts, pts_bytes, kout, s));
  int nbad = 0;
  ACS_HIP(ctx, hipMemcpyAsync(&nbad, b.bad, sizeof(int), hipMemcpyDeviceToHost, s));
  ACS_HIP(ctx, hipStreamSynchronize(s));
  if (report) ext_report(report, hs, nbad);
  return ACS_OK;
}

extern "C" {

int32_t acs_sba_boards_chunk(int32_t n_cams) { return brd_chunk(n_cams); }

int acs_sba_boards(acs_ctx* ctx, double* cams, int32_t n_cams, const double* obj_pts, int32_t n_corners,
                   const double* uv, const uint8_t* mask, int32_t n_boards, double* board_poses,
                   const acs_sba_ext_opts* opts, double* resid_before, double* resid_after,
                   acs_sba_ext_report* report, uint32_t flags) {
  ACS_DEVICE_GUARD(ctx);
  ACS_FISHEYE_ONLY(ctx, flags, "acs_sba_boards");
  return brd_solve(ctx, "acs_sba_boards", cams, n_cams, obj_pts, n_corners, uv, mask, n_boards, board_poses, nullptr,
                   nullptr, 0, nullptr, opts, resid_before, resid_after, report, flags);
}

int acs_sba_boards_points(acs_ctx* ctx, double* cams, int32_t n_cams, const double* obj_pts, int32_t n_corners,
                          const double* uv, const uint8_t* mask, int32_t n_boards, double* board_poses,
                          const double* pt_uv, const uint8_t* pt_mask, int32_t n_pts, double* pts,
                          const acs_sba_ext_opts* opts, double* resid_before, double* resid_after,
                          acs_sba_ext_report* report, uint32_t flags) {
  ACS_DEVICE_GUARD(ctx);
  ACS_FISHEYE_ONLY(ctx, flags, "acs_sba_boards_points");
  return brd_solve(ctx, "acs_sba_boards_points", cams, n_cams, obj_pts, n_corners, uv, mask, n_boards, board_poses,
                   pt_uv, pt_mask, n_pts, pts, opts, resid_before, resid_after, report, flags);
}

}  // extern "C"
