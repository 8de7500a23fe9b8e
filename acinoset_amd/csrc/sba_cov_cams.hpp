// sba_cov_cams.hpp — the reduced-camera covariance core that k_extcov_cams (sba_ext_cov.hip, seven
// gauge generators) and k_brdcov_cams (sba_boards_cov.hip, six) share: one block of 256 threads on
// S (6C x 6C, NP = 6C rounded up to the MFMA tile) in LDS. In the kernels' numbering: 1 the chunk sums
// (cov_cams_sum_chunks), 3-5 Gram-Schmidt of the generators, mu, Jacobi scaling and the pivot test
// (cov_cams_factor), 6-8 the SPD inverse, its refinement step, unscale and - Q Q^T / mu
// (cov_cams_invert), and the report's reduction (cov_cams_totals). Each kernel keeps its generator
// fill (2), its anchor constraint (9), its symmetrisation (10) and its report.
#pragma once

#include "mfma64.hpp"

#define COV_CAMS_PIVOT_TOL 1e-9  // pivots of the unit-diagonal reduced camera system

// sum over the 64 lanes of a wave, the same bits in every lane
__device__ __forceinline__ double wave_sum64(double v) {
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// LDS of a cams kernel in doubles: S (NP x (NP + 1)), Q, K, MC (NP x 8 each), CM (8 x NP),
// scale (NP), tile-inverse scratch (512), reductions (256), small (128), the report's counts (1024)
static size_t cov_cams_lds(int NP) {
  return sizeof(double) * ((size_t)NP * (NP + 1) + 4 * (size_t)NP * 8 + NP + 512 + 256 + 128 + 1024);
}

struct CovCamsLds {
  double* sS;     // NP x LD, LD = NP + 1
  double* sQ;     // NP x 8: G, then its orthonormal basis
  double* sK;     // NP x 8: Q (Cm Q)^-1
  double* sMC;    // NP x 8: M Cm^T
  double* sCM;    // 8 x NP: Cm M
  double* ssc;    // NP: Jacobi scaling
  double* tmp;    // 512
  double* s_red;  // 256
  double* s_sm;   // 128: [0] gauge rank flag, [1] mu, [2] anchor flag, from 8 the kernel's own
};
__device__ __forceinline__ CovCamsLds cov_cams_carve(double* lds, int NP) {
  CovCamsLds L;
  L.sS = lds;
  L.sQ = L.sS + NP * (NP + 1);
  L.sK = L.sQ + NP * 8;
  L.sMC = L.sK + NP * 8;
  L.sCM = L.sMC + NP * 8;
  L.ssc = L.sCM + 8 * NP;
  L.tmp = L.ssc + NP;
  L.s_red = L.tmp + 512;
  L.s_sm = L.s_red + 256;
  return L;
}

// 1. chunk sums in order (raw S to T1), then the symmetrised S to LDS
__device__ __forceinline__ void cov_cams_sum_chunks(const CovCamsLds& L, int NC, int NP, int nchunk,
                                                    const double* __restrict__ part, double* __restrict__ T1) {
  const int LD = NP + 1, nE = NC * NC, tid = threadIdx.x;
  for (int e = tid; e < nE; e += blockDim.x) {
    double v = 0.0;
    for (int ch = 0; ch < nchunk; ++ch) v += part[(size_t)ch * nE + e];
    T1[e] = v;
  }
  __syncthreads();
  for (int e = tid; e < NP * NP; e += blockDim.x) {
    const int r = e / NP, c = e % NP;
    L.sS[r * LD + c] = (r < NC && c < NC) ? 0.5 * (T1[r * NC + c] + T1[c * NC + r]) : 0.0;
  }
}

// 3-5 on the NG generators in sQ (a barrier behind the fill is the caller's). Returns whether the
// problem is degenerate: gbad (G of rank < NG) or a failed pivot. mu, and minp lowered from the
// caller's start value; Ah is left in Ag.
template <int NG>
__device__ __forceinline__ bool cov_cams_factor(const CovCamsLds& L, int NC, int NP, double* __restrict__ Ag,
                                                double& mu_out, double& minp, bool& gbad) {
  const int LD = NP + 1, tid = threadIdx.x;
  double *sS = L.sS, *sQ = L.sQ, *ssc = L.ssc, *s_sm = L.s_sm;
  // 3. wave 0: two-pass Gram-Schmidt (lane l owns rows l and l + 64) and mu = max diag S
  if (tid < 64) {
    const int r0 = tid, r1 = tid + 64;
    const bool h0 = r0 < NC, h1 = r1 < NC;  // rows past NC are not this lane's to touch
    int gb = 0;
    for (int k = 0; k < NG; ++k) {
      double x0 = h0 ? sQ[r0 * 8 + k] : 0.0, x1 = h1 ? sQ[r1 * 8 + k] : 0.0;
      const double n0 = sqrt(wave_sum64(x0 * x0 + x1 * x1));
      for (int pass = 0; pass < 2; ++pass)
        for (int j = 0; j < k; ++j) {
          const double q0 = h0 ? sQ[r0 * 8 + j] : 0.0, q1 = h1 ? sQ[r1 * 8 + j] : 0.0;
          const double dot = wave_sum64(q0 * x0 + q1 * x1);
          x0 -= dot * q0;
          x1 -= dot * q1;
        }
      const double n1 = sqrt(wave_sum64(x0 * x0 + x1 * x1));
      const bool ok = n1 > 1e-8 * n0;  // a column in the span of the earlier ones: rank < NG
      const double inv = ok ? 1.0 / n1 : 0.0;
      gb |= ok ? 0 : 1;
      if (h0) sQ[r0 * 8 + k] = x0 * inv;
      if (h1) sQ[r1 * 8 + k] = x1 * inv;
    }
    double mu = h0 ? sS[r0 * LD + r0] : 0.0;
    if (h1) mu = fmax(mu, sS[r1 * LD + r1]);
    for (int m = 32; m > 0; m >>= 1) mu = fmax(mu, __shfl_xor(mu, m, 64));
    if (tid == 0) {
      s_sm[0] = (double)gb;
      s_sm[1] = mu > 0.0 ? mu : 1.0;
      s_sm[2] = 0.0;
    }
  }
  __syncthreads();
  const double mu = s_sm[1];
  // 4. A = S + mu Q Q^T, scaled to unit diagonal (a diagonal entry that is not > 0 zeroes its row
  //    and column, which the pivot test then fails)
  for (int r = tid; r < NP; r += blockDim.x) {
    double sc = 1.0;
    if (r < NC) {
      double qq = 0.0;
      for (int k = 0; k < NG; ++k) qq += sQ[r * 8 + k] * sQ[r * 8 + k];
      const double dd = sS[r * LD + r] + mu * qq;
      sc = dd > 0.0 ? 1.0 / sqrt(dd) : 0.0;
    }
    ssc[r] = sc;
  }
  __syncthreads();
  for (int e = tid; e < NP * NP; e += blockDim.x) {
    const int r = e / NP, c = e % NP;
    double v = r == c ? 1.0 : 0.0;
    if (r < NC && c < NC) {
      double qq = 0.0;
      for (int k = 0; k < NG; ++k) qq += sQ[r * 8 + k] * sQ[c * 8 + k];
      v = (sS[r * LD + c] + mu * qq) * ssc[r] * ssc[c];
    }
    sS[r * LD + c] = v;
    Ag[e] = v;  // kept for the inverse and its refinement
  }
  __syncthreads();
  // 5. pivot test: scalar right-looking LDL^T of Ah in natural order, in place (Ah is reloaded)
  bool pbad = false;
  for (int k = 0; k < NC; ++k) {
    const double dk = sS[k * LD + k];      // uniform
    if (!(dk > COV_CAMS_PIVOT_TOL)) {      // a NaN fails
      pbad = true;
      minp = dk < minp ? dk : (dk != dk ? dk : minp);
      break;
    }
    minp = fmin(minp, dk);
    const double inv = 1.0 / dk;
    const int m = NC - k - 1;
    for (int e = tid; e < m * m; e += blockDim.x) {
      const int i = k + 1 + e / m, j = k + 1 + e % m;
      sS[i * LD + j] -= sS[i * LD + k] * inv * sS[k * LD + j];
    }
    __syncthreads();
  }
  __syncthreads();
  gbad = s_sm[0] != 0.0;
  mu_out = mu;
  return pbad || gbad;  // uniform
}

// 6-8: sS <- (S + mu Q Q^T)^-1 - Q Q^T / mu from Ah in Ag; T1, T2 (NP x NP) scratch
template <int NG>
__device__ __forceinline__ void cov_cams_invert(const CovCamsLds& L, int NC, int NP, double mu,
                                                const double* __restrict__ Ag, double* __restrict__ T1,
                                                double* __restrict__ T2, int* __restrict__ bad) {
  const int LD = NP + 1, nE = NC * NC, tid = threadIdx.x;
  double *sS = L.sS, *sQ = L.sQ, *ssc = L.ssc;
  // 6. SPD inverse on the MFMA tiles
  for (int e = tid; e < NP * NP; e += blockDim.x) sS[(e / NP) * LD + e % NP] = Ag[e];
  __syncthreads();
  wg_spd_inverse(sS, LD, NP >> 4, L.tmp, bad);
  // 7. one refinement step X <- X + X (I - Ah X)
  wg_mgemm<false, false>(T1, NP, Ag, NP, sS, LD, NP, NP, NP, -1.0, 0.0);
  for (int r = tid; r < NP; r += blockDim.x) T1[r * NP + r] += 1.0;
  __syncthreads();
  wg_mgemm<false, false>(T2, NP, sS, LD, T1, NP, NP, NP, NP, 1.0, 0.0);
  for (int e = tid; e < NP * NP; e += blockDim.x) sS[(e / NP) * LD + e % NP] += T2[e];
  __syncthreads();
  // 8. unscale, minus Q Q^T / mu
  const double imu = 1.0 / mu;
  for (int e = tid; e < nE; e += blockDim.x) {
    const int r = e / NC, c = e % NC;
    double qq = 0.0;
    for (int k = 0; k < NG; ++k) qq += sQ[r * 8 + k] * sQ[c * 8 + k];
    sS[r * LD + c] = sS[r * LD + c] * ssc[r] * ssc[c] - qq * imu;
  }
  __syncthreads();
}

// The report's sums over the block, fixed-order trees: the largest rotation and translation sd of
// sqrt(s2 diag sS) (zero on camera zero_cam, on every camera with all_zero), and over the n records
// (points or boards) the status counts, sum w r^2 and the number of residuals. Every thread returns them.
struct CovCamsTotals {
  double wr2, rot_sd_max, trans_sd_max;
  long long n_ok, n_noobs, n_degenerate, n_res;
};
__device__ __forceinline__ CovCamsTotals cov_cams_totals(const CovCamsLds& L, int NC, int NP, double s2, int zero_cam,
                                                         bool all_zero, int n, const int32_t* __restrict__ status,
                                                         const double* __restrict__ wr2,
                                                         const int32_t* __restrict__ nres) {
  const int LD = NP + 1, tid = threadIdx.x;
  double rs = 0.0, ts = 0.0, sw = 0.0;
  long long cnt[3] = {0, 0, 0}, m = 0;
  for (int r = tid; r < NC; r += blockDim.x) {
    double v = s2 * L.sS[r * LD + r];
    if (all_zero || r / 6 == zero_cam) v = 0.0;
    const double sd = sqrt(v);
    if (r % 6 < 3)
      rs = fmax(rs, sd);
    else
      ts = fmax(ts, sd);
  }
  for (int i = tid; i < n; i += blockDim.x) {
    const int s = status[i];
    if (s >= 0 && s < 3) cnt[s]++;
    sw += wr2[i];
    m += nres[i];
  }
  __syncthreads();
  double* rd = L.tmp;                          // 256 x 2: sum w r^2 and the rotation sd maximum
  double* s_red = L.s_red;
  long long* ri = (long long*)(L.s_sm + 128);  // 256 x 4
  rd[tid] = sw;
  rd[256 + tid] = rs;
  s_red[tid] = ts;
  for (int k = 0; k < 3; ++k) ri[tid * 4 + k] = cnt[k];
  ri[tid * 4 + 3] = m;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) {
      rd[tid] += rd[tid + h];
      rd[256 + tid] = fmax(rd[256 + tid], rd[256 + tid + h]);
      s_red[tid] = fmax(s_red[tid], s_red[tid + h]);
      for (int k = 0; k < 4; ++k) ri[tid * 4 + k] += ri[(tid + h) * 4 + k];
    }
    __syncthreads();
  }
  return CovCamsTotals{rd[0], rd[256], s_red[0], ri[0], ri[1], ri[2], ri[3]};
}
