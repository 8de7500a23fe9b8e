// sba_ext.hip — bundle adjustment of points AND camera extrinsics on gfx950.
//
// Replaces bundle_adjust_points_and_extrinsics (src/lib/sba.py:158-178): scipy TRF with
// loss='cauchy' (f_scale 1) over cost_func_points_extrinsics (:142-146), where every
// camera's Rodrigues vector + translation is shared by all of its observations
// (create_bundle_adjustment_jacobian_sparsity_matrix :11-22 with 6 camera columns).
//
// LM with the points eliminated by Schur complement (spec: oracle/sba_ext.py):
//   k_ext_linearize [point groups] per observation (ext_obs_blocks, sba_ext.hpp): residual,
//                   J_pt = J_Y R, J_cam = J_Y [-[R X]x | I] and the slot record's U (6x6), W =
//                   J_cam^T J_pt (6x3); here g_c (6) behind them and per point V (3x3), g_p. One
//                   point = one aligned lane group (ACS_G_SWITCH), butterfly sums (group_sum).
//   k_ext_schur     [point chunks] fixed-order partial reduced camera system (ext_schur_stage,
//                   ext_schur_entry with M = (V + lam D)^-1) S = U - sum W M W^T, and here
//                   b = -g_c + sum W M g_p, diag U, g_c
//   k_ext_solve     [1 block] chunk sums in order, Marquardt damping, SPD inverse
//                   (blocked Gauss-Jordan on f64 MFMA tiles), camera step
//   k_ext_back      [points] point steps dX = -M (g_p + sum W^T dc), trial points
//   k_ext_cam       [1 block] trial cameras R <- exp([dw]x) R, t <- t + dt
//   k_ext_cost      [point groups] robust cost at the trial state
//   k_ext_lm        [1 block] accept / reject, lambda, stop tests
// The iterations run in ext_lm_loop (groups of four, captured once), which the rigid-board solves
// (sba_boards.hip) drive with their own iteration.
// In a multi-GPU run the per-rank partial (S, b) is what one all-reduce would sum.
#include <algorithm>

#include "mfma64.hpp"
#include "sba_ext.hpp"

#define EXT_STATUS_SKIP 100  // a rejected round: no step, the system is re-formed only

template <int G>
__global__ __launch_bounds__(256) void k_ext_linearize(ExtDims d, const ExtState* __restrict__ st,
                                                       const double* __restrict__ camsbuf,
                                                       const double* __restrict__ ptsbuf,
                                                       const double2* __restrict__ uv,
                                                       const uint8_t* __restrict__ mask,
                                                       const uint8_t* __restrict__ camid, double* __restrict__ Q,
                                                       double* __restrict__ Vg, double* __restrict__ Fp) {
  if (st->status != 0 || !st->relin) return;
  const int cur = st->cur;
  const double* cams = camsbuf + cur * d.C * ACS_CAM_STRIDE;
  const double* pts = ptsbuf + (size_t)cur * d.n * 3;
  __shared__ double s_cam[EXT_MAXC * ACS_CAM_STRIDE];
  for (int i = threadIdx.x; i < d.C * ACS_CAM_STRIDE; i += blockDim.x) s_cam[i] = cams[i];
  __syncthreads();
  const int lane = threadIdx.x & (G - 1);
  const int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
  if (p >= d.n) return;
  const double X0 = pts[3 * p], X1 = pts[3 * p + 1], X2 = pts[3 * p + 2];
  double V[6] = {0, 0, 0, 0, 0, 0}, gp[3] = {0, 0, 0}, F = 0.0;
  for (int slot = lane; slot < d.K; slot += G) {
    const int64_t o = p * d.K + slot;
    double* q = Q + (size_t)o * EXT_Q<true>;
    if (!mask[o] || camid[o] >= d.C) {
      for (int e = 0; e < EXT_Q<true>; ++e) q[e] = 0.0;
      continue;
    }
    ExtObs ob;
    ext_obs_blocks(s_cam + camid[o] * ACS_CAM_STRIDE, X0, X1, X2, uv[o], d.f2, ob, q);
    double gc[6] = {0, 0, 0, 0, 0, 0};
    for (int dd = 0; dd < 2; ++dd) {
      const double *jc = ob.jc[dd], *jp = ob.jp[dd];
      const double w = ob.w[dd], wh = ob.wh[dd];
      F += 0.5 * d.f2 * log1p(ob.z[dd]);
      for (int i = 0; i < 6; ++i) gc[i] += w * ob.r[dd] * jc[i];
      for (int i = 0; i < 3; ++i) {
        gp[i] += w * ob.r[dd] * jp[i];
        for (int j = i; j < 3; ++j) V[i == 0 ? j : (i == 1 ? 2 + j : 5)] += wh * jp[i] * jp[j];
      }
    }
    for (int e = 0; e < 6; ++e) q[EXT_Q_GC + e] = gc[e];
  }
  for (int e = 0; e < 6; ++e) V[e] = group_sum<G>(V[e]);
  for (int e = 0; e < 3; ++e) gp[e] = group_sum<G>(gp[e]);
  F = group_sum<G>(F);
  if (lane == 0) {
    double* vg = Vg + (size_t)p * 10;
    for (int e = 0; e < 6; ++e) vg[e] = V[e];
    for (int e = 0; e < 3; ++e) vg[6 + e] = gp[e];
    vg[9] = F;
    Fp[p] = F;
  }
}

// damped point block inverse M = (V + lam diag V)^-1, V packed [00 01 02 11 12 22]
__device__ __forceinline__ void point_minv(const double* V, double lam, double M[9]) {
  const double a = V[0] * (1.0 + lam) + 1e-300, b = V[1], c = V[2];
  const double e = V[3] * (1.0 + lam) + 1e-300, f = V[4], i = V[5] * (1.0 + lam) + 1e-300;
  const double A = e * i - f * f, B = -(b * i - c * f), Cc = b * f - c * e;
  const double det = a * A + b * B + c * Cc;
  if (!(det > 1e-280)) {  // point without observations: no step
    for (int k = 0; k < 9; ++k) M[k] = 0.0;
    return;
  }
  const double id = 1.0 / det;
  M[0] = A * id;
  M[1] = B * id;
  M[2] = Cc * id;
  M[3] = B * id;
  M[4] = (a * i - c * c) * id;
  M[5] = -(a * f - b * c) * id;
  M[6] = Cc * id;
  M[7] = M[5];
  M[8] = (a * e - b * b) * id;
}

// entries of a chunk partial: S (6C x 6C), b (6C), U diagonal (6C), g_c (6C)
__global__ __launch_bounds__(256) void k_ext_schur(ExtDims d, const ExtState* __restrict__ st,
                                                   const double* __restrict__ Q, const double* __restrict__ Vg,
                                                   const uint8_t* __restrict__ mask,
                                                   const uint8_t* __restrict__ camid, double* __restrict__ part) {
  if (st->status != 0) return;
  const int ch = blockIdx.x;
  const int p0 = ch * d.chunk, p1 = min(d.n, p0 + d.chunk), np = p1 - p0;
  const int NC = 6 * d.C, nE = NC * NC + 3 * NC;
  const double lam = st->lam;
  extern __shared__ double lds[];
  double* sZ = lds;                              // np x K x 18  (W M)
  double* sg = sZ + (size_t)d.chunk * d.K * 18;  // np x 3 (g_p)
  int* scam = (int*)(sg + d.chunk * 3);          // np x K camera id (-1 = none)
  ext_schur_stage<true>(d, p0, np, Q, mask, camid, sZ, scam, [&](int p, int t, double* M) {
    point_minv(Vg + (size_t)p * 10, lam, M);
    for (int j = 0; j < 3; ++j) sg[t * 3 + j] = Vg[(size_t)p * 10 + 6 + j];
    return true;
  });
  for (int e = threadIdx.x; e < nE; e += blockDim.x) {
    double acc = 0.0;
    if (e < NC * NC) {
      acc = ext_schur_entry<true>(d, p0, np, Q, sZ, scam, e / NC, e % NC);
    } else {
      const int r = e - NC * NC, kind = r / NC, a = r % NC, c1 = a / 6, k1 = a % 6;
      for (int t = 0; t < np; ++t) {
        const int64_t base = (int64_t)(p0 + t) * d.K;
        for (int s1 = 0; s1 < d.K; ++s1) {
          if (scam[t * d.K + s1] != c1) continue;
          const double* q = Q + (size_t)(base + s1) * EXT_Q<true>;
          if (kind == 0) {  // b = -g_c + Z g_p
            const double* z = sZ + ((size_t)t * d.K + s1) * 18 + k1 * 3;
            acc += -q[EXT_Q_GC + k1] + z[0] * sg[t * 3] + z[1] * sg[t * 3 + 1] + z[2] * sg[t * 3 + 2];
          } else if (kind == 1) {  // U diagonal
            acc += q[EXT_Q_U + upk(k1, k1)];
          } else {  // g_c
            acc += q[EXT_Q_GC + k1];
          }
        }
      }
    }
    part[(size_t)ch * nE + e] = acc;
  }
}

__global__ __launch_bounds__(256) void k_ext_solve(ExtDims d, ExtState* __restrict__ st, int nchunk,
                                                   const double* __restrict__ part, const double* __restrict__ Vg,
                                                   int n_gp, const double* __restrict__ slots, int n_slots,
                                                   double* __restrict__ dc, double* __restrict__ Sg,
                                                   int* __restrict__ bad) {
  // part: nchunk partials of [S | b | diag U | g_c]; the point-gradient max comes from
  // Vg (n_gp points) and/or per-rank slots (distributed: points live on their ranks)
  if (st->status != 0) return;
  const int NC = 6 * d.C, NP = ((NC + 15) / 16) * 16, nE = NC * NC + 3 * NC, LD = NP + 1;
  const double lam = st->lam;
  extern __shared__ double lds[];
  double* sS = lds;               // NP x LD
  double* sb = sS + NP * LD;      // NP
  double* tmp = sb + NP;          // 512
  double* s_red = tmp + 512;      // 256
  for (int e = threadIdx.x; e < NP * NP; e += blockDim.x) {
    const int r = e / NP, c = e % NP;
    double v = 0.0;
    if (r < NC && c < NC) {
      for (int ch = 0; ch < nchunk; ++ch) v += part[(size_t)ch * nE + r * NC + c];
      if (r == c) {
        double u = 0.0;
        for (int ch = 0; ch < nchunk; ++ch) u += part[(size_t)ch * nE + NC * NC + NC + r];
        v += lam * fmax(u, 1e-12);
      }
    } else if (r == c) {
      v = 1.0;
    }
    sS[r * LD + c] = v;
    if (r < NC && c < NC) Sg[r * NC + c] = v;  // kept for the refinement step
  }
  double gm = 0.0;
  for (int r = threadIdx.x; r < NP; r += blockDim.x) {
    double v = 0.0, g = 0.0;
    if (r < NC)
      for (int ch = 0; ch < nchunk; ++ch) {
        v += part[(size_t)ch * nE + NC * NC + r];
        g += part[(size_t)ch * nE + NC * NC + 2 * NC + r];
      }
    sb[r] = v;
    gm = fmax(gm, fabs(g));
  }
  for (int p = threadIdx.x; p < n_gp; p += blockDim.x)
    for (int j = 0; j < 3; ++j) gm = fmax(gm, fabs(Vg[(size_t)p * 10 + 6 + j]));
  for (int t = threadIdx.x; t < n_slots; t += blockDim.x) gm = fmax(gm, slots[t]);
  __syncthreads();
  {  // block max
    s_red[threadIdx.x] = gm;
    __syncthreads();
    for (int h = (int)blockDim.x / 2; h > 0; h >>= 1) {
      if ((int)threadIdx.x < h) s_red[threadIdx.x] = fmax(s_red[threadIdx.x], s_red[threadIdx.x + h]);
      __syncthreads();
    }
    if (threadIdx.x == 0 && st->relin) st->gmax = s_red[0];
    __syncthreads();
  }
  wg_spd_inverse(sS, LD, NP >> 4, tmp, bad);
  // dc = S^-1 b, then one step of iterative refinement dc += S^-1 (b - S dc): with the
  // gauge left free (as in the reference) S is conditioned like 1/lambda at small damping
  double* sx = tmp;  // NC <= 96 < 512
  double* sr = tmp + 256;
  for (int r = threadIdx.x; r < NC; r += blockDim.x) {
    double v = 0.0;
    for (int c = 0; c < NC; ++c) v += sS[r * LD + c] * sb[c];
    sx[r] = v;
  }
  __syncthreads();
  for (int r = threadIdx.x; r < NC; r += blockDim.x) {
    double v = sb[r];
    for (int c = 0; c < NC; ++c) v -= Sg[r * NC + c] * sx[c];
    sr[r] = v;
  }
  __syncthreads();
  for (int r = threadIdx.x; r < NC; r += blockDim.x) {
    double v = sx[r];
    for (int c = 0; c < NC; ++c) v += sS[r * LD + c] * sr[c];
    dc[r] = v;
  }
}

__global__ __launch_bounds__(256) void k_ext_back(ExtDims d, const ExtState* __restrict__ st,
                                                  const double* __restrict__ Q, const double* __restrict__ Vg,
                                                  const uint8_t* __restrict__ mask,
                                                  const uint8_t* __restrict__ camid, const double* __restrict__ dc,
                                                  double* __restrict__ ptsbuf, double* __restrict__ normp) {
  if (st->status != 0) return;
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= d.n) return;
  const int cur = st->cur;
  const double* X = ptsbuf + (size_t)cur * d.n * 3;
  double* Xn = ptsbuf + (size_t)(cur ^ 1) * d.n * 3;
  double M[9];
  point_minv(Vg + (size_t)p * 10, st->lam, M);
  double acc[3] = {Vg[(size_t)p * 10 + 6], Vg[(size_t)p * 10 + 7], Vg[(size_t)p * 10 + 8]};
  for (int s = 0; s < d.K; ++s) {
    const int64_t o = p * d.K + s;
    if (!mask[o] || camid[o] >= d.C) continue;
    const double* W = Q + (size_t)o * EXT_Q<true> + EXT_Q_W;
    const double* dcc = dc + 6 * camid[o];
    for (int j = 0; j < 3; ++j)
      for (int i = 0; i < 6; ++i) acc[j] += W[i * 3 + j] * dcc[i];
  }
  double dn = 0.0, xn = 0.0;
  for (int j = 0; j < 3; ++j) {
    const double dx = -(M[j * 3] * acc[0] + M[j * 3 + 1] * acc[1] + M[j * 3 + 2] * acc[2]);
    Xn[3 * p + j] = X[3 * p + j] + dx;
    dn += dx * dx;
    xn += X[3 * p + j] * X[3 * p + j];
  }
  normp[2 * p] = dn;
  normp[2 * p + 1] = xn;
}

__global__ void k_ext_cam(ExtDims d, const ExtState* __restrict__ st, const double* __restrict__ dc,
                          double* __restrict__ camsbuf, double* __restrict__ camnorm) {
  if (st->status != 0) return;
  const int c = threadIdx.x;
  if (c >= d.C) return;
  const int cur = st->cur;
  const double* cm = camsbuf + (cur * d.C + c) * ACS_CAM_STRIDE;
  double* cn = camsbuf + ((cur ^ 1) * d.C + c) * ACS_CAM_STRIDE;
  for (int i = 0; i < 8; ++i) cn[i] = cm[i];
  const double w0 = dc[6 * c], w1 = dc[6 * c + 1], w2 = dc[6 * c + 2];
  EXT_EXP_SO3(E, w0, w1, w2)
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      cn[8 + i * 3 + j] = E[i * 3] * cm[8 + j] + E[i * 3 + 1] * cm[8 + 3 + j] + E[i * 3 + 2] * cm[8 + 6 + j];
  double dn = 0.0, xn = 0.0;
  for (int i = 0; i < 3; ++i) {
    cn[17 + i] = cm[17 + i] + dc[6 * c + 3 + i];
    dn += dc[6 * c + i] * dc[6 * c + i] + dc[6 * c + 3 + i] * dc[6 * c + 3 + i];
    xn += cm[17 + i] * cm[17 + i];
  }
  camnorm[2 * c] = dn;
  camnorm[2 * c + 1] = xn;
}

template <int G>
__global__ __launch_bounds__(256) void k_ext_cost(ExtDims d, const ExtState* __restrict__ st, int which,
                                                  const double* __restrict__ camsbuf,
                                                  const double* __restrict__ ptsbuf, const double2* __restrict__ uv,
                                                  const uint8_t* __restrict__ mask,
                                                  const uint8_t* __restrict__ camid, double* __restrict__ Fp) {
  if (which == 1 && st->status != 0) return;
  const int buf = which == 1 ? (st->cur ^ 1) : st->cur;
  const double* cams = camsbuf + buf * d.C * ACS_CAM_STRIDE;
  const double* pts = ptsbuf + (size_t)buf * d.n * 3;
  __shared__ double s_cam[EXT_MAXC * ACS_CAM_STRIDE];
  for (int i = threadIdx.x; i < d.C * ACS_CAM_STRIDE; i += blockDim.x) s_cam[i] = cams[i];
  __syncthreads();
  const int lane = threadIdx.x & (G - 1);
  const int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
  if (p >= d.n) return;
  double F = 0.0;
  for (int slot = lane; slot < d.K; slot += G) {
    const int64_t o = p * d.K + slot;
    if (!mask[o] || camid[o] >= d.C) continue;
    ProjOut po;
    fisheye_project<false>(s_cam + camid[o] * ACS_CAM_STRIDE, pts[3 * p], pts[3 * p + 1], pts[3 * p + 2], po);
    const double2 m = uv[o];
    const double ru = po.u - m.x, rv = po.v - m.y;
    F += 0.5 * d.f2 * (log1p(ru * ru / d.f2) + log1p(rv * rv / d.f2));
  }
  F = group_sum<G>(F);
  if (lane == 0) Fp[p] = F;
}

// The LM decision on a trial, by one thread: cost f, the points' step and state norms^2 dn and xn
// (the cameras' are added here); the stop tests, then accept (swap the state, relax the damping)
// or reject (raise it).
__device__ __forceinline__ void ext_lm_decide(const ExtDims& d, ExtState* st, const ExtOpts& o, double f, double dn,
                                              double xn, const double* camnorm) {
  for (int c = 0; c < d.C; ++c) {
    dn += camnorm[2 * c];
    xn += camnorm[2 * c + 1];
  }
  if (st->gmax <= o.gtol) {
    st->status = ACS_STATUS_GTOL;
    return;
  }
  st->iters += 1;
  st->dnorm = sqrt(dn);
  st->xnorm = sqrt(xn);
  const bool small = sqrt(dn) <= o.xtol * (o.xtol + sqrt(xn));
  if (f < st->F) {
    const bool fconv = (st->F - f) <= o.ftol * fabs(st->F);
    st->nacc += 1;
    st->F = f;
    st->cur ^= 1;
    st->lam = fmax(st->lam * 0.1, EXT_LAM_MIN);
    st->relin = 1;
    if (fconv)
      st->status = ACS_STATUS_FTOL;
    else if (small)
      st->status = ACS_STATUS_XTOL;
  } else {
    st->lam *= 10.0;
    st->relin = 0;
    if (st->lam > 1e16) st->status = ACS_STATUS_STALLED;
  }
  if (st->status == 0 && st->iters >= o.max_iters) st->status = ACS_STATUS_MAXITER;
}

__global__ __launch_bounds__(256) void k_ext_lm(ExtDims d, ExtState* __restrict__ st, ExtOpts o, int init,
                                                const double* __restrict__ Fp, const double* __restrict__ normp,
                                                const double* __restrict__ camnorm) {
  __shared__ double s_red[256];
  const int tid = threadIdx.x;
  auto bsum = [&](double v) {
    s_red[tid] = v;
    __syncthreads();
    for (int h = (int)blockDim.x / 2; h > 0; h >>= 1) {
      if (tid < h) s_red[tid] += s_red[tid + h];
      __syncthreads();
    }
    const double r = s_red[0];
    __syncthreads();
    return r;
  };
  double f = 0.0, dn = 0.0, xn = 0.0;
  for (int p = tid; p < d.n; p += blockDim.x) {
    f += Fp[p];
    if (!init) {
      dn += normp[2 * p];
      xn += normp[2 * p + 1];
    }
  }
  f = bsum(f);
  if (init) {
    if (tid == 0) st->F = st->F0 = f;
    return;
  }
  if (st->status != 0) return;
  dn = bsum(dn);
  xn = bsum(xn);
  if (tid == 0) ext_lm_decide(d, st, o, f, dn, xn, camnorm);
}

// ---------------------------------------------------------------------------------------
// The device buffers of one solve, one allocation laid out by ext_layout.
struct ExtBuffers {
  double *cams, *pts;  // the current and the trial state: [2][C] records, [2][n][3]
  double *Q, *Vg, *Fp, *part, *dc, *Sg, *normp, *camnorm;
  ExtState* st;
  int* bad;
  double2* uvp;  // the slot tensor: the workspace's, or (own_slots) a copy behind the rest
  uint8_t *mk, *cid;
  int nchunk;
};

// the buffers at base; with a null base only the size in bytes (Arena)
static size_t ext_layout(ExtBuffers& b, double* base, const ExtDims& d, bool own_slots) {
  const size_t n = d.n, NC = 6 * d.C, slots = n * d.K;
  Arena a{base};
  b.nchunk = ext_nchunk(d);
  b.cams = a.take(2 * (size_t)d.C * ACS_CAM_STRIDE);
  b.pts = a.take(6 * n);
  b.Q = a.take(slots * EXT_Q<true>);
  b.Vg = a.take(n * 10);
  b.Fp = a.take(n);
  b.part = a.take(b.nchunk * (NC * NC + 3 * NC));
  b.dc = a.take(96);
  b.Sg = a.take(96 * 96);
  b.normp = a.take(2 * n);
  b.camnorm = a.take(64);
  b.st = a.take<ExtState>(16);
  b.bad = a.take<int>(2);
  if (own_slots) {
    b.uvp = a.take<double2>(2 * slots);
    b.mk = a.take<uint8_t>((slots + 7) / 8);
    b.cid = a.take<uint8_t>((slots + 7) / 8);
  }
  return a.bytes();
}

// the starting state into both copies, the LM state (first: the rank round protocol's flag)
static int ext_start(acs_ctx* ctx, const ExtDims& d, const ExtBuffers& b, const ObsSlots& in, double lambda0,
                     int first) {
  hipStream_t s = ctx->stream;
  const size_t cam_bytes = sizeof(double) * ACS_CAM_STRIDE * d.C;
  for (int k = 0; k < 2; ++k)
    ACS_HIP(ctx, hipMemcpyAsync(b.cams + k * d.C * ACS_CAM_STRIDE, in.cams, cam_bytes, hipMemcpyDeviceToDevice, s));
  ACS_HIP(ctx, hipMemcpyAsync(b.pts, in.pts, sizeof(double) * 3 * d.n, hipMemcpyDeviceToDevice, s));
  ACS_HIP(ctx, hipMemsetAsync(b.bad, 0, sizeof(int), s));
  ExtState st0;
  std::memset(&st0, 0, sizeof(st0));
  st0.lam = lambda0;
  st0.relin = 1;
  st0.first = first;
  ACS_HIP(ctx, hipMemcpyAsync(b.st, &st0, sizeof(st0), hipMemcpyHostToDevice, s));
  return ACS_OK;
}

// The launches every driver is made of (the single-GPU iteration, the rank phases, the first cost).
// the system at the current state: slot records and point blocks, chunk partials
static void ext_launch_system(hipStream_t s, const ExtDims& d, const ExtBuffers& b) {
  const int blocks = acs_grid((int64_t)d.n * d.G, 256);
#define EXT_LIN(g)                                                                                              \
  hipLaunchKernelGGL((k_ext_linearize<g>), dim3(blocks), dim3(256), 0, s, d, b.st, b.cams, b.pts, b.uvp, b.mk, \
                     b.cid, b.Q, b.Vg, b.Fp)
  ACS_G_SWITCH(d.G, EXT_LIN)
#undef EXT_LIN
  hipLaunchKernelGGL(k_ext_schur, dim3(b.nchunk), dim3(256), ext_schur_lds(d, 3), s, d, b.st, b.Q, b.Vg, b.mk, b.cid,
                     b.part);
}

static size_t ext_solve_lds(int C) {
  const int NP = ((6 * C + 15) / 16) * 16;
  return sizeof(double) * ((size_t)NP * (NP + 1) + NP + 512 + 256);
}

// the launches the rigid-board SBA (sba_boards.hip) shares with this file (declared in sba_ext.hpp)
void ext_launch_solve(hipStream_t s, const ExtDims& d, ExtState* st, const double* sys, int nsys, const double* Vg,
                      int n_gp, const double* slots, int n_slots, double* dc, double* Sg, int* bad) {
  hipLaunchKernelGGL(k_ext_solve, dim3(1), dim3(256), ext_solve_lds(d.C), s, d, st, nsys, sys, Vg, n_gp, slots,
                     n_slots, dc, Sg, bad);
}

void ext_launch_cam(hipStream_t s, const ExtDims& d, const ExtState* st, const double* dc, double* cams,
                    double* camnorm) {
  hipLaunchKernelGGL(k_ext_cam, dim3(1), dim3(64), 0, s, d, st, dc, cams, camnorm);
}

void ext_launch_lm(hipStream_t s, const ExtDims& d, ExtState* st, const ExtOpts& o, int init, const double* Fp,
                   const double* normp, const double* camnorm) {
  hipLaunchKernelGGL(k_ext_lm, dim3(1), dim3(256), 0, s, d, st, o, init, Fp, normp, camnorm);
}

// the camera step from the nsys partial systems at sys (the point-gradient maximum from n_gp
// points of Vg and n_slots per-rank values), the point steps, the trial cameras
static void ext_launch_step(hipStream_t s, const ExtDims& d, const ExtBuffers& b, const double* sys, int nsys,
                            int n_gp, const double* slots, int n_slots) {
  ext_launch_solve(s, d, b.st, sys, nsys, b.Vg, n_gp, slots, n_slots, b.dc, b.Sg, b.bad);
  hipLaunchKernelGGL(k_ext_back, dim3(acs_grid(d.n, 256)), dim3(256), 0, s, d, b.st, b.Q, b.Vg, b.mk, b.cid, b.dc, b.pts,
                     b.normp);
  ext_launch_cam(s, d, b.st, b.dc, b.cams, b.camnorm);
}

// the robust cost per point: which = 0 at the current state, 1 at the trial
static void ext_launch_cost(hipStream_t s, const ExtDims& d, const ExtBuffers& b, int which) {
  const int blocks = acs_grid((int64_t)d.n * d.G, 256);
#define EXT_COST(g)                                                                                            \
  hipLaunchKernelGGL((k_ext_cost<g>), dim3(blocks), dim3(256), 0, s, d, b.st, which, b.cams, b.pts, b.uvp, b.mk, \
                     b.cid, b.Fp)
  ACS_G_SWITCH(d.G, EXT_COST)
#undef EXT_COST
}

// one LM iteration of the single-GPU solve
static void ext_enqueue(hipStream_t s, const ExtDims& d, const ExtOpts& o, const ExtBuffers& b) {
  ext_launch_system(s, d, b);
  ext_launch_step(s, d, b, b.part, b.nchunk, d.n, nullptr, 0);
  ext_launch_cost(s, d, b, 1);
  ext_launch_lm(s, d, b.st, o, 0, b.Fp, b.normp, b.camnorm);
}

// the point side of the rigid-board SBA with free points (sba_boards.hip, declared in sba_ext.hpp):
// the same kernels on the caller's buffers, one launch each
void ext_launch_linearize(hipStream_t s, const ExtDims& d, const ExtState* st, const double* cams, const double* pts,
                          const double2* uv, const uint8_t* mask, const uint8_t* camid, double* Q, double* Vg,
                          double* Fp) {
  const int blocks = acs_grid((int64_t)d.n * d.G, 256);
#define EXT_LIN(g) \
  hipLaunchKernelGGL((k_ext_linearize<g>), dim3(blocks), dim3(256), 0, s, d, st, cams, pts, uv, mask, camid, Q, Vg, Fp)
  ACS_G_SWITCH(d.G, EXT_LIN)
#undef EXT_LIN
}

void ext_launch_schur(hipStream_t s, const ExtDims& d, const ExtState* st, const double* Q, const double* Vg,
                      const uint8_t* mask, const uint8_t* camid, double* part) {
  hipLaunchKernelGGL(k_ext_schur, dim3(ext_nchunk(d)), dim3(256), ext_schur_lds(d, 3), s, d, st, Q, Vg, mask, camid,
                     part);
}

void ext_launch_back(hipStream_t s, const ExtDims& d, const ExtState* st, const double* Q, const double* Vg,
                     const uint8_t* mask, const uint8_t* camid, const double* dc, double* pts, double* normp) {
  hipLaunchKernelGGL(k_ext_back, dim3(acs_grid(d.n, 256)), dim3(256), 0, s, d, st, Q, Vg, mask, camid, dc, pts, normp);
}

void ext_launch_point_cost(hipStream_t s, const ExtDims& d, const ExtState* st, int which, const double* cams,
                           const double* pts, const double2* uv, const uint8_t* mask, const uint8_t* camid,
                           double* Fp) {
  const int blocks = acs_grid((int64_t)d.n * d.G, 256);
#define EXT_COST(g) \
  hipLaunchKernelGGL((k_ext_cost<g>), dim3(blocks), dim3(256), 0, s, d, st, which, cams, pts, uv, mask, camid, Fp)
  ACS_G_SWITCH(d.G, EXT_COST)
#undef EXT_COST
}

void ext_report(acs_sba_ext_report* report, const ExtState& hs, int nbad) {
  report->status = hs.status == 0 ? ACS_STATUS_MAXITER : hs.status;
  report->iters = hs.iters;
  report->n_accepted = hs.nacc;
  report->n_bad_pivots = nbad;
  report->cost_before = hs.F0;
  report->cost_after = hs.F;
  report->grad_max = hs.gmax;
  report->lambda_final = hs.lam;
}

// the iterations in groups of four (a linear chain, captured once), the status read per group.
// Every decision counts an iteration or stops, so max_iters of them end the solve: no replay beyond
// them, and none at all for max_iters <= 0 (the state comes back as it went in)
int ext_lm_loop(acs_ctx* ctx, const ExtState* st, int max_iters, const std::function<void()>& enqueue, ExtState* hs) {
  hipStream_t s = ctx->stream;
  const int group = 4;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  bool use_graph = max_iters > 0 && hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed) == hipSuccess;
  if (use_graph) {
    for (int c = 0; c < group; ++c) enqueue();
    if (hipStreamEndCapture(s, &graph) != hipSuccess ||
        hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) {
      if (graph) (void)hipGraphDestroy(graph);
      (void)hipGetLastError();
      graph = nullptr;
      exec = nullptr;
      use_graph = false;
    }
  }
  for (int it = 0; it < max_iters; it += group) {
    if (use_graph) {
      ACS_HIP(ctx, hipGraphLaunch(exec, s));
    } else {
      for (int c = 0; c < group; ++c) enqueue();
    }
    ACS_HIP(ctx, hipGetLastError());
    ACS_HIP(ctx, hipMemcpyAsync(hs, st, sizeof(*hs), hipMemcpyDeviceToHost, s));
    ACS_HIP(ctx, hipStreamSynchronize(s));
    if (hs->status != 0) break;
  }
  if (exec) (void)hipGraphExecDestroy(exec);
  if (graph) (void)hipGraphDestroy(graph);
  if (max_iters <= 0) {
    ACS_HIP(ctx, hipMemcpyAsync(hs, st, sizeof(*hs), hipMemcpyDeviceToHost, s));
    ACS_HIP(ctx, hipStreamSynchronize(s));
  }
  return ACS_OK;
}

extern "C" {

void acs_sba_ext_default_opts(acs_sba_ext_opts* o) {
  o->max_iters = 500;
  o->reserved = 0;
  o->f_scale = 1.0;
  o->ftol = 1e-12;
  o->xtol = 1e-12;
  o->gtol = 1e-8;
  o->lambda0 = 1e-3;
}

// host only: the dimensions acs_sba_extrinsics launches by (ext_dims, ext_nchunk)
int acs_sba_ext_plan(int64_t n_pts, int32_t K, int32_t* G, int32_t* chunk, int32_t* nchunk) {
  if (n_pts < 1 || n_pts >= (int64_t)INT32_MAX || K < 1 || K > EXT_MAXK || !G || !chunk || !nchunk)
    return ACS_E_INVALID;
  const ExtDims d = ext_dims(n_pts, K, 1, 1.0);
  *G = d.G;
  *chunk = d.chunk;
  *nchunk = ext_nchunk(d);
  return ACS_OK;
}

int acs_sba_extrinsics(acs_ctx* ctx, double* cams, int32_t n_cams, const double* uv, const int32_t* pt_idx,
                       const int32_t* cam_idx, int64_t n_obs, double* pts, int64_t n_pts,
                       const acs_sba_ext_opts* opts, double* resid_before, double* resid_after,
                       acs_sba_ext_report* report, uint32_t flags) {
  ACS_DEVICE_GUARD(ctx);
  ACS_FISHEYE_ONLY(ctx, flags, "acs_sba_extrinsics");
  acs_sba_ext_opts op;
  acs_sba_ext_default_opts(&op);
  if (opts) op = *opts;
  ACS_CHECK(ctx, n_cams >= 1 && n_cams <= EXT_MAXC, "acs_sba_extrinsics: n_cams=%d (1..%d)", n_cams, EXT_MAXC);
  ACS_CHECK(ctx, n_obs >= 1 && n_pts >= 1 && n_obs < (int64_t)INT32_MAX, "acs_sba_extrinsics: bad sizes");
  ACS_CHECK(ctx, op.f_scale > 0 && op.max_iters >= 0, "acs_sba_extrinsics: bad options");
  hipStream_t s = ctx->stream;
  int rc;
  ObsSlots in;
  if ((rc = acs_stage_obs(ctx, "acs_sba_extrinsics", EXT_MAXK, ACS_CAM_STRIDE, cams, n_cams, uv, pt_idx, cam_idx, n_obs,
                          pts, n_pts, flags, &in)))
    return rc;
  double* drb = nullptr;
  if (resid_before) {
    drb = (double*)acs_out_buf(ctx, WS_OUT0, resid_before, sizeof(double) * 2 * n_obs, flags);
    if (!drb || (rc = acs_sba_residuals(ctx, in.cams, n_cams, in.uv, in.pt_idx, in.cam_idx, n_obs, in.pts, n_pts, drb,
                                        ACS_DEVICE_PTRS)))
      return rc ? rc : ACS_E_NOMEM;
  }
  const ExtDims d = ext_dims(n_pts, in.K, n_cams, op.f_scale);
  ExtBuffers b;
  double* arena = (double*)acs_ws(ctx, WS_FTE6, ext_layout(b, nullptr, d, false));
  if (!arena) return ACS_E_NOMEM;
  ext_layout(b, arena, d, false);
  b.uvp = in.uvp;
  b.mk = in.mask;
  b.cid = in.camid;
  if ((rc = ext_start(ctx, d, b, in, op.lambda0, 0))) return rc;
  ExtOpts o{op.max_iters, op.ftol, op.xtol, op.gtol};
  ext_launch_cost(s, d, b, 0);
  ext_launch_lm(s, d, b.st, o, 1, b.Fp, b.normp, b.camnorm);
  ACS_HIP(ctx, hipGetLastError());
  ExtState hs;
  if ((rc = ext_lm_loop(ctx, b.st, op.max_iters, [&] { ext_enqueue(s, d, o, b); }, &hs))) return rc;
  const double* fcams = b.cams + hs.cur * n_cams * ACS_CAM_STRIDE;
  const double* fpts = b.pts + (size_t)hs.cur * n_pts * 3;
  const hipMemcpyKind kout = (flags & ACS_DEVICE_PTRS) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (resid_after) {
    double* dra = (double*)acs_out_buf(ctx, WS_OUT1, resid_after, sizeof(double) * 2 * n_obs, flags);
    if (!dra || (rc = acs_sba_residuals(ctx, fcams, n_cams, in.uv, in.pt_idx, in.cam_idx, n_obs, fpts, n_pts, dra,
                                        ACS_DEVICE_PTRS)))
      return rc ? rc : ACS_E_NOMEM;
    if ((rc = acs_stage_out(ctx, resid_after, dra, sizeof(double) * 2 * n_obs, flags))) return rc;
  }
  if (resid_before && (rc = acs_stage_out(ctx, resid_before, drb, sizeof(double) * 2 * n_obs, flags))) return rc;
  ACS_HIP(ctx, hipMemcpyAsync(cams, fcams, sizeof(double) * ACS_CAM_STRIDE * n_cams, kout, s));
  ACS_HIP(ctx, hipMemcpyAsync(pts, fpts, sizeof(double) * 3 * n_pts, kout, s));
  int nbad = 0;
  ACS_HIP(ctx, hipMemcpyAsync(&nbad, b.bad, sizeof(int), hipMemcpyDeviceToHost, s));
  ACS_HIP(ctx, hipStreamSynchronize(s));
  if (report) ext_report(report, hs, nbad);
  return ACS_OK;
}

}  // extern "C"

// =======================================================================================
// distributed points + extrinsics: points are split over the ranks,
// cameras replicated. Per LM step one all-reduce of the reduced camera system (p1 =
// [S | b | diag U | g_c | per-rank point |g| max]) and one of 3 doubles (cost, point
// step norms). Every rank solves the same camera system and takes the same decision.
// Spec: oracle/sba_ext_dist.py.
// =======================================================================================
__global__ __launch_bounds__(256) void k_ext_pack1(ExtDims d, const ExtState* __restrict__ st, int nchunk,
                                                   const double* __restrict__ part, const double* __restrict__ Vg,
                                                   int rank, double* __restrict__ p1) {
  if (st->status != 0) return;
  __shared__ double s_red[256];
  const int NC = 6 * d.C, nE = NC * NC + 3 * NC;
  for (int e = threadIdx.x; e < nE; e += blockDim.x) {
    double v = 0.0;
    for (int ch = 0; ch < nchunk; ++ch) v += part[(size_t)ch * nE + e];
    p1[e] = v;
  }
  double gm = 0.0;
  for (int p = threadIdx.x; p < d.n; p += blockDim.x)
    for (int j = 0; j < 3; ++j) gm = fmax(gm, fabs(Vg[(size_t)p * 10 + 6 + j]));
  s_red[threadIdx.x] = gm;
  __syncthreads();
  for (int h = (int)blockDim.x / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) s_red[threadIdx.x] = fmax(s_red[threadIdx.x], s_red[threadIdx.x + h]);
    __syncthreads();
  }
  if (threadIdx.x == 0) p1[nE + rank] = s_red[0];
}

__global__ __launch_bounds__(256) void k_ext_pack3(ExtDims d, const ExtState* __restrict__ st, int which,
                                                   const double* __restrict__ Fp, const double* __restrict__ normp,
                                                   double* __restrict__ p3) {
  if (which == 1 && st->status != 0) return;
  __shared__ double s_red[3][256];
  double a = 0.0, b = 0.0, c = 0.0;
  for (int p = threadIdx.x; p < d.n; p += blockDim.x) {
    a += Fp[p];
    if (which) {
      b += normp[2 * p];
      c += normp[2 * p + 1];
    }
  }
  s_red[0][threadIdx.x] = a;
  s_red[1][threadIdx.x] = b;
  s_red[2][threadIdx.x] = c;
  __syncthreads();
  for (int h = (int)blockDim.x / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h)
      for (int k = 0; k < 3; ++k) s_red[k][threadIdx.x] += s_red[k][threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0)
    for (int k = 0; k < 3; ++k) p3[k] = s_red[k][0];
}

// Rank round protocol: the decision on the pending trial from the all-reduced (cost,
// |dX|^2, |X|^2) of the previous round (ext_lm_decide); a rejection marks the round
// SKIP (no step: the system is re-formed at the current state with the raised damping).
__global__ void k_ext_decide(ExtDims d, ExtState* __restrict__ st, ExtOpts o, const double* __restrict__ p3,
                             const double* __restrict__ camnorm) {
  if (threadIdx.x != 0) return;
  if (st->first) {
    st->first = 0;
    st->F = st->F0 = p3[0];
    if (o.max_iters <= 0) st->status = ACS_STATUS_MAXITER;  // no step at all
    return;
  }
  if (st->status != 0 || !st->pending) return;
  st->pending = 0;
  ext_lm_decide(d, st, o, p3[0], p3[1], p3[2], camnorm);
  if (st->status == 0 && !st->relin) st->status = EXT_STATUS_SKIP;
}

// Around the system of a round: a round that took a step forms the next system at its trial
// state (points / cameras copy cur ^ 1) with the damping an acceptance sets (speculation:
// the next round's decision keeps it or discards it); the LM state is swapped for those
// kernels and restored after them. A rejected round re-linearises at the current state
// (the speculative system overwrote its linearisation).
__global__ void k_ext_spec(ExtState* __restrict__ st, int enter) {
  if (threadIdx.x != 0) return;
  if (enter) {
    if (st->status == EXT_STATUS_SKIP) {
      st->status = 0;
      st->relin = 1;
    } else if (st->status == 0) {
      st->pending = 1;
      st->spec_on = 1;
      st->save_cur = st->cur;
      st->save_lam = st->lam;
      st->cur ^= 1;
      st->lam = fmax(st->lam * 0.1, EXT_LAM_MIN);
      st->relin = 1;
    }
  } else if (st->spec_on) {
    st->spec_on = 0;
    st->cur = st->save_cur;
    st->lam = st->save_lam;
  }
}

#define EXT_DIST_RING 4

struct acs_sba_ext_dist {
  acs_ctx* ctx;
  void* own = nullptr;
  ExtDims d;
  ExtOpts o;
  int R, rank;
  ExtBuffers b;
  // status after each round: pinned ring with completion events (acs_sba_ext_dist_poll)
  int32_t* snap = nullptr;
  hipEvent_t snap_ev[EXT_DIST_RING] = {};
  int64_t rounds = 0;
};

extern "C" {

int acs_sba_ext_dist_create(acs_ctx* ctx, const double* cams, int32_t n_cams, const double* uv,
                            const int32_t* pt_idx, const int32_t* cam_idx, int64_t n_obs, const double* pts,
                            int64_t n_pts, const acs_sba_ext_opts* opts, int32_t rank, int32_t world,
                            acs_sba_ext_dist** out, int64_t* payload_sizes, uint32_t flags) {
  ACS_DEVICE_GUARD(ctx);
  ACS_FISHEYE_ONLY(ctx, flags, "acs_sba_ext_dist_create");
  acs_sba_ext_opts op;
  acs_sba_ext_default_opts(&op);
  if (opts) op = *opts;
  ACS_CHECK(ctx, n_cams >= 1 && n_cams <= EXT_MAXC, "sba_ext_dist: n_cams=%d (1..%d)", n_cams, EXT_MAXC);
  ACS_CHECK(ctx, n_obs >= 1 && n_pts >= 1 && n_obs < (int64_t)INT32_MAX, "sba_ext_dist: bad sizes");
  ACS_CHECK(ctx, op.f_scale > 0 && op.max_iters >= 0, "sba_ext_dist: bad options");
  ACS_CHECK(ctx, world >= 1 && rank >= 0 && rank < world, "sba_ext_dist: rank %d / world %d", rank, world);
  hipStream_t s = ctx->stream;
  int rc;
  ObsSlots in;
  if ((rc = acs_stage_obs(ctx, "sba_ext_dist", EXT_MAXK, ACS_CAM_STRIDE, cams, n_cams, uv, pt_idx, cam_idx, n_obs, pts,
                          n_pts, flags, &in)))
    return rc;
  acs_sba_ext_dist* h = new acs_sba_ext_dist();
  h->ctx = ctx;
  h->d = ext_dims(n_pts, in.K, n_cams, op.f_scale);
  h->R = world;
  h->rank = rank;
  h->o = ExtOpts{op.max_iters, op.ftol, op.xtol, op.gtol};
  const int NC = 6 * n_cams, nE = NC * NC + 3 * NC;
  ExtBuffers& b = h->b;
  if (acs_dev_malloc(&h->own, ext_layout(b, nullptr, h->d, true)) != hipSuccess) {
    delete h;
    return acs_fail(ctx, ACS_E_NOMEM, "sba_ext_dist: allocation failed");
  }
  ext_layout(b, (double*)h->own, h->d, true);
  const size_t slots = (size_t)n_pts * in.K;
  ACS_HIP(ctx, hipMemcpyAsync(b.uvp, in.uvp, sizeof(double2) * slots, hipMemcpyDeviceToDevice, s));
  ACS_HIP(ctx, hipMemcpyAsync(b.mk, in.mask, slots, hipMemcpyDeviceToDevice, s));
  ACS_HIP(ctx, hipMemcpyAsync(b.cid, in.camid, slots, hipMemcpyDeviceToDevice, s));
  if ((rc = ext_start(ctx, h->d, b, in, op.lambda0, 1))) return rc;
  ACS_HIP(ctx, hipStreamSynchronize(s));
  bool snap_ok = acs_host_malloc((void**)&h->snap, sizeof(int32_t) * EXT_DIST_RING, hipHostMallocDefault) == hipSuccess;
  for (auto& e : h->snap_ev)
    if (snap_ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
      e = nullptr;
      snap_ok = false;
    }
  if (!snap_ok) {
    acs_sba_ext_dist_destroy(h);
    return acs_fail(ctx, ACS_E_HIP, "sba_ext_dist: pinned status ring allocation failed");
  }
  if (payload_sizes) {
    payload_sizes[0] = nE + world + 3;  // [reduced camera system | (cost, |dX|^2, |X|^2)]
    payload_sizes[1] = 3;
  }
  *out = h;
  return ACS_OK;
}

int acs_sba_ext_dist_destroy(acs_sba_ext_dist* h) {
  ACS_DEVICE_GUARD(h ? h->ctx : nullptr);
  if (!h) return ACS_OK;
  (void)hipStreamSynchronize(h->ctx->stream);
  for (auto& e : h->snap_ev)
    if (e) (void)hipEventDestroy(e);
  if (h->snap) (void)acs_host_free(h->snap);
  if (h->own) (void)acs_dev_free(h->own);
  delete h;
  return ACS_OK;
}

}  // extern "C"

// the rank's reduced camera system at the current state (payload part 1, zeroed first)
static int ext_dist_system(acs_sba_ext_dist* h, double* p1) {
  acs_ctx* ctx = h->ctx;
  hipStream_t s = ctx->stream;
  const ExtDims& d = h->d;
  const ExtBuffers& b = h->b;
  const int NC = 6 * d.C, nE = NC * NC + 3 * NC;
  ACS_HIP(ctx, hipMemsetAsync(p1, 0, sizeof(double) * (nE + h->R), s));
  ext_launch_system(s, d, b);
  hipLaunchKernelGGL(k_ext_pack1, dim3(1), dim3(256), 0, s, d, b.st, b.nchunk, b.part, b.Vg, h->rank, p1);
  ACS_HIP(ctx, hipGetLastError());
  return ACS_OK;
}

// solve the summed system p1, step cameras and this rank's points, (cost, |dX|^2, |X|^2) of
// the trial into p3
static int ext_dist_step(acs_sba_ext_dist* h, const double* p1, double* p3) {
  acs_ctx* ctx = h->ctx;
  hipStream_t s = ctx->stream;
  const ExtDims& d = h->d;
  const ExtBuffers& b = h->b;
  const int NC = 6 * d.C, nE = NC * NC + 3 * NC;
  ext_launch_step(s, d, b, p1, 1, 0, p1 + nE, h->R);
  ext_launch_cost(s, d, b, 1);
  hipLaunchKernelGGL(k_ext_pack3, dim3(1), dim3(256), 0, s, d, b.st, 1, b.Fp, b.normp, p3);
  ACS_HIP(ctx, hipGetLastError());
  return ACS_OK;
}

extern "C" {

// payload [p1 | p3] of the starting state: its system and its cost
int acs_sba_ext_dist_init(acs_sba_ext_dist* h, double* payload) {
  ACS_DEVICE_GUARD(h ? h->ctx : nullptr);
  hipStream_t s = h->ctx->stream;
  const int NC = 6 * h->d.C, n1 = NC * NC + 3 * NC + h->R;
  ext_launch_cost(s, h->d, h->b, 0);
  hipLaunchKernelGGL(k_ext_pack3, dim3(1), dim3(256), 0, s, h->d, h->b.st, 0, h->b.Fp, h->b.normp, payload + n1);
  ACS_HIP(h->ctx, hipGetLastError());
  return ext_dist_system(h, payload);
}

// One round: decide on the pending trial (in: all-reduced payload of the previous round),
// step from its system, and the next system (speculatively at the trial state) with the
// trial's cost into out - one all-reduce per LM step, the status polled a round late.
int acs_sba_ext_dist_round(acs_sba_ext_dist* h, const double* in, double* out) {
  ACS_DEVICE_GUARD(h ? h->ctx : nullptr);
  acs_ctx* ctx = h->ctx;
  ACS_CHECK(ctx, in && out && in != out, "sba_ext_dist_round: in and out must be distinct buffers");
  hipStream_t s = ctx->stream;
  const int NC = 6 * h->d.C, n1 = NC * NC + 3 * NC + h->R;
  int rc;
  hipLaunchKernelGGL(k_ext_decide, dim3(1), dim3(64), 0, s, h->d, h->b.st, h->o, in + n1, (const double*)h->b.camnorm);
  if ((rc = ext_dist_step(h, in, out + n1))) return rc;
  hipLaunchKernelGGL(k_ext_spec, dim3(1), dim3(64), 0, s, h->b.st, 1);
  if ((rc = ext_dist_system(h, out))) return rc;
  hipLaunchKernelGGL(k_ext_spec, dim3(1), dim3(64), 0, s, h->b.st, 0);
  ACS_HIP(ctx, hipGetLastError());
  const int slot = (int)(h->rounds % EXT_DIST_RING);
  ACS_HIP(ctx, hipMemcpyAsync(h->snap + slot, &h->b.st->status, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  ACS_HIP(ctx, hipEventRecord(h->snap_ev[slot], s));
  h->rounds++;
  return ACS_OK;
}

// LM status after round r (waits for that round only)
int acs_sba_ext_dist_poll(acs_sba_ext_dist* h, int64_t round, int32_t* status) {
  ACS_DEVICE_GUARD(h ? h->ctx : nullptr);
  ACS_CHECK(h ? h->ctx : nullptr, h && status && round >= 0 && round < h->rounds && round >= h->rounds - EXT_DIST_RING,
            "sba_ext_dist_poll: round %lld not among the last %d enqueued", (long long)round, EXT_DIST_RING);
  const int slot = (int)(round % EXT_DIST_RING);
  ACS_HIP(h->ctx, hipEventSynchronize(h->snap_ev[slot]));
  *status = h->snap[slot];
  return ACS_OK;
}

int acs_sba_ext_dist_result(acs_sba_ext_dist* h, double* cams, double* pts, acs_sba_ext_report* report,
                            uint32_t flags) {
  ACS_DEVICE_GUARD(h ? h->ctx : nullptr);
  acs_ctx* ctx = h->ctx;
  hipStream_t s = ctx->stream;
  const ExtDims& d = h->d;
  ExtState hs;
  ACS_HIP(ctx, hipMemcpyAsync(&hs, h->b.st, sizeof(hs), hipMemcpyDeviceToHost, s));
  ACS_HIP(ctx, hipStreamSynchronize(s));
  const hipMemcpyKind kout = (flags & ACS_DEVICE_PTRS) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (cams)
    ACS_HIP(ctx, hipMemcpyAsync(cams, h->b.cams + hs.cur * d.C * ACS_CAM_STRIDE, sizeof(double) * ACS_CAM_STRIDE * d.C,
                                kout, s));
  if (pts) ACS_HIP(ctx, hipMemcpyAsync(pts, h->b.pts + (size_t)hs.cur * d.n * 3, sizeof(double) * 3 * d.n, kout, s));
  int nbad = 0;
  ACS_HIP(ctx, hipMemcpyAsync(&nbad, h->b.bad, sizeof(int), hipMemcpyDeviceToHost, s));
  ACS_HIP(ctx, hipStreamSynchronize(s));
  if (report) ext_report(report, hs, nbad);
  return ACS_OK;
}

}  // extern "C"
