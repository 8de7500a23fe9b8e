// sba_ext.hpp — what the points + extrinsics SBA (sba_ext.hip) and its covariance
// (sba_ext_cov.hip) share: the problem's dimensions, the slot record, an observation's blocks
// (ext_obs_blocks) and the Schur partials (ext_schur_stage, ext_schur_entry); and what the
// rigid-board SBA (sba_boards.hip, through sba_boards.hpp) takes from the solver: the LM state and
// options, the driver loop (ext_lm_loop), the launches of k_ext_solve / k_ext_cam / k_ext_lm and of
// the point side, and the exponential map (EXT_EXP_SO3). The reduced-camera covariance core the two
// covariances share is in sba_cov_cams.hpp.
#pragma once

#include <algorithm>
#include <functional>

#include "common.hpp"

#define EXT_MAXC 16
#define EXT_CHUNK 64
#define EXT_MAXK 64  // observations of one point: one 64-lane group, one slot per lane
#define BRD_MAXNC 256  // corners of a rigid board (sba_boards.hip): four rounds of one wave

// The slot record, EXT_Q doubles per observation slot: U (21 packed upper), W = J_cam^T J_pt (6 x 3)
// and, in the solver's record only (GC = true), the camera gradient g_c (6) behind them.
enum : int { EXT_Q_U = 0, EXT_Q_W = 21, EXT_Q_GC = 39 };
template <bool GC>
constexpr int EXT_Q = GC ? 45 : 39;

// n points of K slots, C cameras; one point = one aligned group of G lanes (ACS_G_SWITCH);
// chunk: points per Schur block; f2 = f_scale^2
struct ExtDims {
  int n, K, C, G, chunk;
  double f2;
};

// chunk: the W M tiles of a Schur block (18 doubles and a camera id per slot, 3 doubles per
// point) must fit ~96 KB of LDS
static inline ExtDims ext_dims(int64_t n_pts, int K, int n_cams, double f_scale) {
  ExtDims d{(int)n_pts, K, n_cams, 2, 0, f_scale * f_scale};
  while (d.G < K) d.G <<= 1;
  d.chunk = std::max(1, std::min(EXT_CHUNK, (int)(96 * 1024 / (148 * K + 24))));
  return d;
}
static inline int ext_nchunk(const ExtDims& d) { return (d.n + d.chunk - 1) / d.chunk; }

// LDS of a Schur block: W M (18 doubles per slot), `per_point` doubles per point, a camera id per slot
static inline size_t ext_schur_lds(const ExtDims& d, int per_point) {
  return sizeof(double) * ((size_t)d.chunk * d.K * 18 + d.chunk * per_point) + sizeof(int) * (size_t)d.chunk * d.K;
}

// damping floor: the gauge is left free (as in the reference: the 7-DoF similarity of the free
// points, the 6-DoF rigid motion of the rigid boards), so the reduced camera system is singular
// up to lambda; below ~1e-8 its gauge directions are resolved by rounding alone. Spec shared
// with oracle/sba_ext.py (LAM_MIN).
#define EXT_LAM_MIN 1e-7

struct ExtState {
  double F, F0, lam, gmax, dnorm, xnorm;
  int cur, status, iters, nacc, relin, pad;
  // rank round protocol (acs_sba_ext_dist_round): first round pending, a trial awaiting
  // its decision, the speculative swap of the state for the next system
  int first, pending, spec_on, save_cur;
  double save_lam;
};

struct ExtOpts {
  int max_iters;
  double ftol, xtol, gtol;
};

// The launches of sba_ext.hip that the rigid-board SBA (sba_boards.hip) takes as they are: the
// camera step from nsys partial systems at sys (k_ext_solve; the gradient maximum of the other
// side from n_gp points of Vg and n_slots values), the trial cameras (k_ext_cam), and the first
// cost (init) or the LM decision over d.n cost and norm entries (k_ext_lm).
void ext_launch_solve(hipStream_t s, const ExtDims& d, ExtState* st, const double* sys, int nsys, const double* Vg,
                      int n_gp, const double* slots, int n_slots, double* dc, double* Sg, int* bad);
void ext_launch_cam(hipStream_t s, const ExtDims& d, const ExtState* st, const double* dc, double* cams,
                    double* camnorm);
void ext_launch_lm(hipStream_t s, const ExtDims& d, ExtState* st, const ExtOpts& o, int init, const double* Fp,
                   const double* normp, const double* camnorm);
void ext_report(acs_sba_ext_report* report, const ExtState& hs, int nbad);

// The LM driver loop of a single-GPU solve (acs_sba_extrinsics, the board solves): the iterations
// that enqueue() puts on the context's stream, in groups of four captured once into a graph (plain
// launches when capture or instantiation fails), the device state st read into *hs after every
// group, until a status is set or max_iters decisions are through. No iteration for max_iters <= 0:
// *hs is then the state as it stands. An ACS_* code.
int ext_lm_loop(acs_ctx* ctx, const ExtState* st, int max_iters, const std::function<void()>& enqueue, ExtState* hs);

// The point side, for the rigid-board SBA with free points (acs_sba_boards_points): k_ext_linearize,
// k_ext_schur (ext_nchunk(d) partials from part), k_ext_back and k_ext_cost as they are, on the
// caller's buffers. cams [2][C] records and pts [2][n][3] are the current and the trial state that
// st->cur selects; uv / mask / camid the slot tensor (n, K); Q (n K EXT_Q<true>), Vg (n, 10),
// Fp (n), normp (2 n).
void ext_launch_linearize(hipStream_t s, const ExtDims& d, const ExtState* st, const double* cams, const double* pts,
                          const double2* uv, const uint8_t* mask, const uint8_t* camid, double* Q, double* Vg,
                          double* Fp);
void ext_launch_schur(hipStream_t s, const ExtDims& d, const ExtState* st, const double* Q, const double* Vg,
                      const uint8_t* mask, const uint8_t* camid, double* part);
void ext_launch_back(hipStream_t s, const ExtDims& d, const ExtState* st, const double* Q, const double* Vg,
                     const uint8_t* mask, const uint8_t* camid, const double* dc, double* pts, double* normp);
void ext_launch_point_cost(hipStream_t s, const ExtDims& d, const ExtState* st, int which, const double* cams,
                           const double* pts, const double2* uv, const uint8_t* mask, const uint8_t* camid,
                           double* Fp);

// double E[9] = exp([w]x), row-major (Rodrigues; the identity below |w| = 1e-300), declared in the
// caller's scope. The text of k_ext_cam's update, shared with k_brd_pose (sba_boards.hip); a macro,
// not a function: as an inlined function the same statements give k_ext_cam other registers.
#define EXT_EXP_SO3(E, w0, w1, w2)                                                                             \
  const double E##_th = sqrt((w0) * (w0) + (w1) * (w1) + (w2) * (w2));                                         \
  double E[9];                                                                                                 \
  if (E##_th < 1e-300) {                                                                                       \
    for (int i = 0; i < 9; ++i) E[i] = (i % 4 == 0) ? 1.0 : 0.0;                                               \
  } else {                                                                                                     \
    const double k0 = (w0) / E##_th, k1 = (w1) / E##_th, k2 = (w2) / E##_th, cs = cos(E##_th), sn = sin(E##_th), \
                 oc = 1.0 - cs;                                                                                \
    E[0] = cs + oc * k0 * k0;                                                                                  \
    E[1] = oc * k0 * k1 - sn * k2;                                                                             \
    E[2] = oc * k0 * k2 + sn * k1;                                                                             \
    E[3] = oc * k1 * k0 + sn * k2;                                                                             \
    E[4] = cs + oc * k1 * k1;                                                                                  \
    E[5] = oc * k1 * k2 - sn * k0;                                                                             \
    E[6] = oc * k2 * k0 - sn * k1;                                                                             \
    E[7] = oc * k2 * k1 + sn * k0;                                                                             \
    E[8] = cs + oc * k2 * k2;                                                                                  \
  }

__device__ __forceinline__ int upk(int i, int j) {  // packed upper-triangular index, 6x6
  if (i > j) {
    const int t = i;
    i = j;
    j = t;
  }
  return i * 6 - i * (i - 1) / 2 + (j - i);
}

// One observation at the camera record c (LDS) of the point X with the measurement m, per image
// row dd: the residual r, the Cauchy weight w = 1 / (1 + z), z = r^2 / f2, the Triggs weight
// wh = max((1 - z) w^2, 0.1 w), J_cam = [-(J_Y [v]x) | J_Y] with v = R X = Y - t, and
// J_pt = J_Y R.
struct ExtObs {
  double r[2], z[2], w[2], wh[2], jc[2][6], jp[2][3];
};
// ... and its camera-side blocks U = sum_dd wh J_cam^T J_cam (packed) and W = sum_dd wh J_cam^T J_pt,
// written to the slot record q
__device__ __forceinline__ void ext_obs_blocks(const double* c, double X0, double X1, double X2, double2 m, double f2,
                                               ExtObs& ob, double* q) {
  double U[21], W[18];
  for (int e = 0; e < 21; ++e) U[e] = 0.0;
  for (int e = 0; e < 18; ++e) W[e] = 0.0;
  ProjOut po;
  fisheye_project<true>(c, X0, X1, X2, po);
  ob.r[0] = po.u - m.x;
  ob.r[1] = po.v - m.y;
  const double v0 = po.Y[0] - c[17], v1 = po.Y[1] - c[18], v2 = po.Y[2] - c[19];
  for (int dd = 0; dd < 2; ++dd) {
    const double* jy = po.JY + 3 * dd;
    double* jc = ob.jc[dd];
    double* jp = ob.jp[dd];
    jc[0] = -(jy[1] * v2 - jy[2] * v1);
    jc[1] = -(jy[2] * v0 - jy[0] * v2);
    jc[2] = -(jy[0] * v1 - jy[1] * v0);
    for (int i = 0; i < 3; ++i) {
      jc[3 + i] = jy[i];
      jp[i] = po.J[3 * dd + i];
    }
    const double z = ob.r[dd] * ob.r[dd] / f2;
    const double w = 1.0 / (1.0 + z);
    const double wh = fmax((1.0 - z) * w * w, 0.1 * w);
    ob.z[dd] = z;
    ob.w[dd] = w;
    ob.wh[dd] = wh;
    for (int i = 0; i < 6; ++i) {
      for (int j = i; j < 6; ++j) U[upk(i, j)] += wh * jc[i] * jc[j];
      for (int j = 0; j < 3; ++j) W[i * 3 + j] += wh * jc[i] * jp[j];
    }
  }
  for (int e = 0; e < 21; ++e) q[EXT_Q_U + e] = U[e];
  for (int e = 0; e < 18; ++e) q[EXT_Q_W + e] = W[e];
}

// The Schur partial of a chunk of np points from p0, S = sum U - sum W M W^T, in two steps.
// ext_schur_stage: every point's W M tiles (sZ, np x K x 18) and camera ids (scam, np x K, -1 = no
// observation or a point that takes no part) into LDS. point_m(p, t, M) gives point p (t-th of
// the chunk) its 3x3 M and returns whether it takes part. Ends with a barrier.
template <bool GC, class PointM>
__device__ __forceinline__ void ext_schur_stage(const ExtDims& d, int p0, int np, const double* __restrict__ Q,
                                                const uint8_t* __restrict__ mask,
                                                const uint8_t* __restrict__ camid, double* sZ, int* scam,
                                                PointM point_m) {
  for (int t = threadIdx.x; t < np; t += blockDim.x) {
    const int p = p0 + t;
    double M[9];
    const bool pok = point_m(p, t, M);
    for (int s = 0; s < d.K; ++s) {
      const int64_t o = (int64_t)p * d.K + s;
      const bool ok = pok && mask[o] && camid[o] < d.C;
      scam[t * d.K + s] = ok ? camid[o] : -1;
      const double* W = Q + (size_t)o * EXT_Q<GC> + EXT_Q_W;
      for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 3; ++j)
          sZ[((size_t)t * d.K + s) * 18 + i * 3 + j] =
              ok ? W[i * 3] * M[j] + W[i * 3 + 1] * M[3 + j] + W[i * 3 + 2] * M[6 + j] : 0.0;
    }
  }
  __syncthreads();
}

// ext_schur_entry: entry (a, b) of S over the chunk, summed in point and slot order by one thread
template <bool GC>
__device__ __forceinline__ double ext_schur_entry(const ExtDims& d, int p0, int np, const double* __restrict__ Q,
                                                  const double* sZ, const int* scam, int a, int b) {
  const int c1 = a / 6, k1 = a % 6, c2 = b / 6, k2 = b % 6;
  double acc = 0.0;
  for (int t = 0; t < np; ++t) {
    const int64_t base = (int64_t)(p0 + t) * d.K;
    for (int s1 = 0; s1 < d.K; ++s1) {
      if (scam[t * d.K + s1] != c1) continue;
      if (c1 == c2) acc += Q[(size_t)(base + s1) * EXT_Q<GC> + EXT_Q_U + upk(k1, k2)];
      const double* z = sZ + ((size_t)t * d.K + s1) * 18 + k1 * 3;
      for (int s2 = 0; s2 < d.K; ++s2) {
        if (scam[t * d.K + s2] != c2) continue;
        const double* w = Q + (size_t)(base + s2) * EXT_Q<GC> + EXT_Q_W + k2 * 3;
        acc -= z[0] * w[0] + z[1] * w[1] + z[2] * w[2];
      }
    }
  }
  return acc;
}
