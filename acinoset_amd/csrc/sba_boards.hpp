// sba_boards.hpp — what the rigid-board SBA (sba_boards.hip) and its covariance
// (sba_boards_cov.hip) share: the problem's dimensions, the view record, the stage of a board into
// LDS (brd_stage), a view's sums over its corners (brd_view_sums) and the Schur partials
// (brd_schur_stage, brd_schur_entry). The shape of ext_obs_blocks / ext_schur_stage /
// ext_schur_entry (sba_ext.hpp) with a 6 x 6 board block where those have a 3 x 3 point block.
#pragma once

#include "sba_ext.hpp"

// The view record, BRD_Q doubles per (board, camera) slot: U (21 packed upper), W = J_cam^T J_brd
// (6 x 6) and, in the solver's record only (GC = true), the camera gradient g_c (6) behind them.
enum : int { BRD_Q_U = 0, BRD_Q_W = 21, BRD_Q_GC = 57 };
template <bool GC>
constexpr int BRD_Q = GC ? 63 : 57;

// B boards of nc corners, C cameras; chunk: boards per Schur block; f2 = f_scale^2
struct BrdDims {
  int B, C, nc, chunk;
  double f2;
};

// chunk: per board the W M tiles (36 doubles per camera), M_b and its flag (37), g_b (6) and a seen
// flag per camera must fit ~96 KB of LDS (as ext_dims); the covariance, which needs less, takes the same
static inline int brd_chunk(int n_cams) {
  return std::max(1, std::min(EXT_CHUNK, (int)(96 * 1024 / (292 * n_cams + 344))));
}
static inline BrdDims brd_dims(int n_boards, int n_cams, int n_corners, double f_scale) {
  return BrdDims{n_boards, n_cams, n_corners, brd_chunk(n_cams), f_scale * f_scale};
}
static inline int brd_nchunk(const BrdDims& d) { return (d.B + d.chunk - 1) / d.chunk; }
// LDS of a Schur block: W M (36 doubles per view), `per_board` doubles per board, a seen flag per view
static inline size_t brd_schur_lds(const BrdDims& d, int per_board) {
  return sizeof(double) * (size_t)d.chunk * (d.C * 36 + per_board) + sizeof(int) * (size_t)d.chunk * d.C;
}

// board pose record: R row-major (9), t (3)
__device__ __forceinline__ void brd_world(const double* pose, const double* p, double rp[3], double X[3]) {
  for (int i = 0; i < 3; ++i) {
    rp[i] = pose[3 * i] * p[0] + pose[3 * i + 1] * p[1] + pose[3 * i + 2] * p[2];
    X[i] = rp[i] + pose[9 + i];
  }
}

// cameras, the board's pose, R_b p_j and X_bj into LDS; ends with a barrier
__device__ __forceinline__ void brd_stage(const BrdDims& d, const double* __restrict__ cams,
                                          const double* __restrict__ pose, const double* __restrict__ obj,
                                          double* s_cam, double* s_rp, double* s_X) {
  for (int i = threadIdx.x; i < d.C * ACS_CAM_STRIDE; i += blockDim.x) s_cam[i] = cams[i];
  for (int j = threadIdx.x; j < d.nc; j += blockDim.x) {
    const double p[3] = {obj[3 * j], obj[3 * j + 1], obj[3 * j + 2]};
    double rp[3], X[3];
    brd_world(pose, p, rp, X);
    for (int i = 0; i < 3; ++i) {
      s_rp[3 * j + i] = rp[i];
      s_X[3 * j + i] = X[i];
    }
  }
  __syncthreads();
}

// The sums of one view over its corners as one wave keeps them: sums(v) adds the group_sum of v over
// the wave's live lanes to entry e and moves on to the next; entry e lives in lane e % 64, acc0 for
// e < 64 and acc1 behind it. A named type, not a lambda in brd_view_sums: with the lambda the same
// statements lose their branches and k_brd_linearize an occupancy step (199 -> 256 VGPRs).
struct BrdLaneSums {
  int lane;
  double acc0 = 0.0, acc1 = 0.0;
  bool live = false;  // this lane has a corner in the round
  int e = 0;          // the next entry of the round
  __device__ void operator()(double v) {
    const double t = group_sum<64>(live ? v : 0.0);
    if ((e & 63) == lane) {
      if (e < 64)
        acc0 += t;
      else
        acc1 += t;
    }
    ++e;
  }
};

// One seen view, by one wave: lanes over the corners in rounds of 64, the rounds in order. Entries in
// order: U (21), W (36), what mid adds, V = sum wh J_brd^T J_brd (21), what tail adds. mid(ob, add)
// and tail(ob, jb, add) call add(v) once per entry of their own, jb being J_brd of the two image
// rows. cam: the camera record, s_rp / s_X: brd_stage's, uv: the view's nc measurements.
template <class Mid, class Tail>
__device__ __forceinline__ void brd_view_sums(const BrdDims& d, const double* cam, const double* s_rp,
                                              const double* s_X, const double2* __restrict__ uv, BrdLaneSums& add,
                                              Mid mid, Tail tail) {
  for (int j0 = 0; j0 < d.nc; j0 += 64) {
    add.live = j0 + add.lane < d.nc;
    const int j = add.live ? j0 + add.lane : d.nc - 1;
    add.e = 0;
    ExtObs ob;
    double qo[EXT_Q<false>];
    ext_obs_blocks(cam, s_X[3 * j], s_X[3 * j + 1], s_X[3 * j + 2], uv[j], d.f2, ob, qo);
    const double v0 = s_rp[3 * j], v1 = s_rp[3 * j + 1], v2 = s_rp[3 * j + 2];
    double jb[2][6];
#pragma unroll
    for (int dd = 0; dd < 2; ++dd) {
      const double* jp = ob.jp[dd];
      jb[dd][0] = -(jp[1] * v2 - jp[2] * v1);
      jb[dd][1] = -(jp[2] * v0 - jp[0] * v2);
      jb[dd][2] = -(jp[0] * v1 - jp[1] * v0);
      jb[dd][3] = jp[0];
      jb[dd][4] = jp[1];
      jb[dd][5] = jp[2];
    }
#pragma unroll
    for (int k = 0; k < 21; ++k) add(qo[EXT_Q_U + k]);
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int k = 0; k < 6; ++k) add(ob.wh[0] * ob.jc[0][i] * jb[0][k] + ob.wh[1] * ob.jc[1][i] * jb[1][k]);
    mid(ob, add);
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int k = i; k < 6; ++k) add(ob.wh[0] * jb[0][i] * jb[0][k] + ob.wh[1] * jb[1][i] * jb[1][k]);
    tail(ob, jb, add);
  }
}

// The Schur partial of a chunk of nb boards from b0, S = sum U - sum W M W^T, in two steps.
// brd_schur_stage: every view's W M tile (sZ, nb x C x 36) into LDS; zeros for a view that is not
// seen (sseen, nb x C) or whose board takes no part. board_m(t) gives the t-th board of the chunk its
// 6 x 6 M (row-major), or null when it takes no part. Ends with a barrier.
template <bool GC, class BoardM>
__device__ __forceinline__ void brd_schur_stage(const BrdDims& d, int b0, int nb, const double* __restrict__ Qv,
                                                const int* sseen, double* sZ, BoardM board_m) {
  for (int i = threadIdx.x; i < nb * d.C * 36; i += blockDim.x) {
    const int t = i / (d.C * 36), r = i % (d.C * 36), c = r / 36, k1 = (r % 36) / 6, k2 = r % 6;
    double z = 0.0;
    const double* M = board_m(t);
    if (sseen[t * d.C + c] && M) {
      const double* W = Qv + ((size_t)(b0 + t) * d.C + c) * BRD_Q<GC> + BRD_Q_W + k1 * 6;
      for (int k = 0; k < 6; ++k) z += W[k] * M[k * 6 + k2];
    }
    sZ[i] = z;
  }
  __syncthreads();
}

// brd_schur_entry: entry (a, b) of S over the chunk, summed in board order by one thread
template <bool GC>
__device__ __forceinline__ double brd_schur_entry(const BrdDims& d, int b0, int nb, const double* __restrict__ Qv,
                                                  const double* sZ, const int* sseen, int a, int b) {
  const int c1 = a / 6, k1 = a % 6, c2 = b / 6, k2 = b % 6;
  double acc = 0.0;
  for (int t = 0; t < nb; ++t) {
    if (!sseen[t * d.C + c1] || !sseen[t * d.C + c2]) continue;
    const double* q1 = Qv + ((size_t)(b0 + t) * d.C + c1) * BRD_Q<GC>;
    if (c1 == c2) acc += q1[BRD_Q_U + upk(k1, k2)];
    const double* z = sZ + ((size_t)t * d.C + c1) * 36 + k1 * 6;
    const double* w = Qv + ((size_t)(b0 + t) * d.C + c2) * BRD_Q<GC> + BRD_Q_W + k2 * 6;
    double s = 0.0;
    for (int k = 0; k < 6; ++k) s += z[k] * w[k];
    acc -= s;
  }
  return acc;
}
