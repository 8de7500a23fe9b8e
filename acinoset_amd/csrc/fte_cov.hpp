// fte_cov.hpp — covariance of the FTE estimate (acs_fte_covariance), included by fte.hip.
//
// cov = the inverse of the undamped Gauss-Newton normal matrix H at (X, tau), read off block
// by block (selected inversion) on the elimination tree of the solve's block cyclic reduction:
// H is block tridiagonal in the 3-frame super-blocks D_i (BP rows) with the couplings
// E_i = H(i, i - 1) and a dense border G_i (BP x GR) / T (GR x GR) for the constant shutter
// delays. Input: Dc (whole tiles), Ec, GBc and the per-frame border blocks Tc, as
// fte_launch_lin + cr_launch_assemble_build leave them at damping 0.
//
// Up pass, one launch per level (step s = 2^level), one workgroup per eliminated block
// i = s (2m + 1) with the active neighbours l = i - s and r = i + s (r may not exist):
//   Dinv_i = D_i^-1,  W_l = Dinv_i E_il,  W_r = Dinv_i E_ir,  W_g = Dinv_i G_i,
//   D_l -= E_li W_l,  D_r -= E_ri W_r,  E_rl = -E_ri W_l,  G_l -= E_li W_g,  G_r -= E_ri W_g,
//   T -= G_i^T W_g.
// Two eliminated blocks update the same survivor, so each writes its terms to buffers of its
// own (UL_i for l, UR_i for r) and the survivor subtracts them, left term first, when the
// next level loads it (the same launch carries one workgroup per survivor for that). The T
// terms are per-block partials summed in block order by chunks (k_cov_tsum), no atomics.
// Top: block 0 is left; [[D_0, G_0], [G_0^T, T]] (at most 96 + 32 rows) is inverted in LDS.
// Down pass, one launch per level in reverse order, one workgroup per block i of that level,
// every input from the coarser level:
//   S_il = -(W_l S_ll + W_r S_rl + W_g S_gl),  S_ir = -(W_l S_lr + W_r S_rr + W_g S_gr),
//   S_ig = -(W_l S_lg + W_r S_rg + W_g S_gg),
//   S_ii = Dinv_i - S_il W_l^T - S_ir W_r^T - S_ig W_g^T.
// (l, i) and (i, r) are the next level's adjacent pairs, so a level keeps S_ii, S_i,next and
// S_ig per active block: S_lr is replaced by S_li, and S_ir is new.
// A held delay (camera 0, or tau_held at (tau, gradient)) is a constant: its row and column
// of the border are the identity before the up pass and zero in cov_tau. Padding rows carry
// the identity of the build. Non-positive pivots are counted (wg_gj_inverse<true>) and
// returned; nothing is clamped.
// Per-frame shutter delays (sd_mode 1) are not covered: the build eliminates them inside the
// blocks, and their covariances need a back-substitution of their own.
//
// Memory kept in the context (ctx->fte_cov, grown on first use): Dinv/S_ii, S_i,next, W_l,
// W_r (n_blk BP^2 each), W_g, S_ig (n_blk BP GR each) and the small border buffers. The up
// pass's scratch (update terms, the couplings of the next level, T partials) is the solve
// arena's dL, dR, Ec2 and Tau, free during this call.
#pragma once

#define COV_THREADS 1024

struct CovMat {
  const double* p;
  int rs, cs;  // element (r, c) = p[r rs + c cs]
};
__device__ __forceinline__ CovMat cov_mat(const double* p, int ld) { return CovMat{p, ld, 1}; }
__device__ __forceinline__ CovMat cov_mat_t(const double* p, int ld) { return CovMat{p, 1, ld}; }

// acc += A[i0 .. i0+15][0 .. K) B[0 .. K)[j0 .. j0+15]  (one wave, f64 MFMA 16x16x4)
__device__ __forceinline__ dbl4 cov_tile(dbl4 acc, const CovMat& A, const CovMat& B, int i0, int j0, int K) {
  const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  const double* a = A.p + (size_t)(i0 + li) * A.rs + (size_t)lk * A.cs;
  const double* b = B.p + (size_t)lk * B.rs + (size_t)(j0 + li) * B.cs;
  for (int k = 0; k < K; k += 4) acc = mfma64(a[(size_t)k * A.cs], b[(size_t)k * B.rs], acc);
  return acc;
}
// tile (i0, j0) of C <- sc * acc; C element (r, c) at C[r rs + c cs]
__device__ __forceinline__ void cov_put(double* C, int rs, int cs, int i0, int j0, const dbl4& acc, double sc) {
  const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) C[(size_t)(i0 + lk + 4 * r) * rs + (size_t)(j0 + li) * cs] = sc * acc[r];
}

struct CovBufs {
  // kept in the context
  double *Sii, *Snx, *Wl, *Wr, *Wg, *Sg, *Sgg, *T0, *partA, *partT, *vmm, *rep;
  int* held;  // GR flags, then n_tau_free, then the pivot count
  // scratch of the up pass (solve arena)
  double *D, *E0, *E1, *G, *ULd, *ULg, *URd, *URg, *Tp;
};
#define COV_NFREE(c, GR) ((c).held + (GR))
#define COV_BAD(c, GR) ((c).held + (GR) + 1)

// chunk sums of the per-frame border blocks and delay gradients (k_fte_linearize's compact
// copy Tc), frames in index order inside a chunk
__global__ __launch_bounds__(256) void k_cov_frame_sums(FteDims d, const double* __restrict__ Tc,
                                                        double* __restrict__ partA) {
  const int ch = blockIdx.x, st = tc_stride(d.Cg);
  const int fc = (d.N + CR_NCHUNK - 1) / CR_NCHUNK, k0 = ch * fc, k1 = min(d.N, k0 + fc);
  for (int e = threadIdx.x; e < st; e += blockDim.x) {
    double v = 0.0;
    for (int k = k0; k < k1; ++k) v += Tc[(size_t)k * st + e];
    partA[(size_t)ch * st + e] = v;
  }
}

// Held delays, the border at the start of the up pass, and the blocks as the up pass reads
// them: the columns of G of held delays, the gradient column and the padding zeroed; the
// strictly lower tiles of E (which the build does not store) zeroed.
__global__ __launch_bounds__(256) void k_cov_prep(FteDims d, const double* __restrict__ tau, CovBufs c) {
  const int i = blockIdx.x, tid = threadIdx.x, BP = d.BP, GR = d.GR, Cg = d.Cg, st = tc_stride(Cg);
  __shared__ int s_held[32];
  if (tid < 32) {
    bool h = true;
    if (tid < Cg) {
      double g = 0.0;
      for (int ch = 0; ch < CR_NCHUNK; ++ch) g += c.partA[(size_t)ch * st + Cg * Cg + tid];
      h = tau_held(tau[tid], g, d.Ts, tid);
    }
    s_held[tid] = h ? 1 : 0;
  }
  __syncthreads();
  double* G = c.G + (size_t)i * BP * GR;
  for (int e = tid; e < BP * GR; e += blockDim.x)
    if (s_held[e % GR]) G[e] = 0.0;
  double* E = c.E0 + (size_t)i * BP * BP;
  for (int e = tid; e < BP * BP; e += blockDim.x) {
    const int r = e / BP, q = e - r * BP;
    if ((r >> 4) > (q >> 4)) E[e] = 0.0;
  }
  if (i == 0) {
    for (int e = tid; e < GR * GR; e += blockDim.x) {
      const int r = e / GR, q = e - r * GR;
      double v = r == q ? 1.0 : 0.0;
      if (!s_held[r] && !s_held[q]) {
        v = 0.0;
        for (int ch = 0; ch < CR_NCHUNK; ++ch) v += c.partA[(size_t)ch * st + r * Cg + q];
      }
      c.T0[e] = v;
    }
    if (tid < GR) c.held[tid] = s_held[tid];
    if (tid == 0) {
      int nf = 0;
      for (int q = 0; q < Cg; ++q) nf += s_held[q] ? 0 : 1;
      *COV_NFREE(c, GR) = nf;
      *COV_BAD(c, GR) = 0;
    }
  }
}

// Block j subtracts the terms of the level of step hs from its two eliminated neighbours
// (left first); every thread of the workgroup, ends with a barrier.
__device__ void cov_apply_pending(const FteDims& d, const CovBufs& c, int j, int hs, bool hasg) {
  const int BP = d.BP, GR = d.GR, n = d.nblk;
  const bool hl = j - hs >= 0, hr = j + hs < n;
  double* D = c.D + (size_t)j * BP * BP;
  const double* ur = c.URd + (size_t)(hl ? j - hs : 0) * BP * BP;
  const double* ul = c.ULd + (size_t)(hr ? j + hs : 0) * BP * BP;
  for (int e = threadIdx.x; e < BP * BP; e += blockDim.x) {
    double v = D[e];
    if (hl) v -= ur[e];
    if (hr) v -= ul[e];
    D[e] = v;
  }
  if (hasg) {
    double* G = c.G + (size_t)j * BP * GR;
    const double* gr = c.URg + (size_t)(hl ? j - hs : 0) * BP * GR;
    const double* gl = c.ULg + (size_t)(hr ? j + hs : 0) * BP * GR;
    for (int e = threadIdx.x; e < BP * GR; e += blockDim.x) {
      double v = G[e];
      if (hl) v -= gr[e];
      if (hr) v -= gl[e];
      G[e] = v;
    }
  }
  __syncthreads();
}

// One level of the up pass: workgroups [0, ne) eliminate the blocks i = s (2m + 1), the rest
// bring the survivors j = 2 s m up to date with the level below. Ein / Eout: the couplings
// H(j, j - s) of this level and H(j, j - 2s) of the next.
__global__ __launch_bounds__(COV_THREADS) void k_cov_up(FteDims d, int s, int ne, int hasg, CovBufs c,
                                                        const double* __restrict__ Ein, double* __restrict__ Eout) {
  const int BP = d.BP, GR = d.GR, n = d.nblk, NB = BP >> 4, LD = BP + 1;
  const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if ((int)blockIdx.x >= ne) {
    cov_apply_pending(d, c, 2 * s * ((int)blockIdx.x - ne), s >> 1, hasg);
    return;
  }
  const int i = s * (2 * (int)blockIdx.x + 1), r = i + s;
  const bool hr = r < n;
  if (s > 1) cov_apply_pending(d, c, i, s >> 1, hasg);
  extern __shared__ double lds[];
  double* sD = lds;                    // D_i, then Dinv_i
  double* sW = lds + (size_t)BP * LD;  // W_l, W_r, W_g in turn
  const size_t bb = (size_t)BP * BP, bg = (size_t)BP * GR;
  const double* Di = c.D + i * bb;
  for (int e = threadIdx.x; e < BP * BP; e += blockDim.x) sD[(e / BP) * LD + e % BP] = Di[e];
  __syncthreads();
  wg_gj_inverse<true>(sD, LD, NB, nullptr, COV_BAD(c, GR));
  double* Dinv = c.Sii + i * bb;
  for (int e = threadIdx.x; e < BP * BP; e += blockDim.x) Dinv[e] = sD[(e / BP) * LD + e % BP];
  const CovMat mD = cov_mat(sD, LD), mW = cov_mat(sW, LD);
  const CovMat Ei = cov_mat(Ein + i * bb, BP), EiT = cov_mat_t(Ein + i * bb, BP);
  const CovMat Er = cov_mat(Ein + (hr ? r : i) * bb, BP), ErT = cov_mat_t(Ein + (hr ? r : i) * bb, BP);
  const dbl4 z = {0.0, 0.0, 0.0, 0.0};
  const int nt = NB * NB;
  // W_l = Dinv E_i;  UL_i = E_i^T W_l;  E'_r = -E_r W_l
  for (int t = wave; t < nt; t += nw) {
    const int i0 = (t / NB) << 4, j0 = (t % NB) << 4;
    const dbl4 a = cov_tile(z, mD, Ei, i0, j0, BP);
    cov_put(sW, LD, 1, i0, j0, a, 1.0);
    cov_put(c.Wl + i * bb, BP, 1, i0, j0, a, 1.0);
  }
  __syncthreads();
  for (int t = wave; t < nt; t += nw) {
    const int i0 = (t / NB) << 4, j0 = (t % NB) << 4;
    cov_put(c.ULd + i * bb, BP, 1, i0, j0, cov_tile(z, EiT, mW, i0, j0, BP), 1.0);
    if (hr) cov_put(Eout + r * bb, BP, 1, i0, j0, cov_tile(z, Er, mW, i0, j0, BP), -1.0);
  }
  __syncthreads();
  // W_r = Dinv E_r^T;  UR_i = E_r W_r
  if (hr) {
    for (int t = wave; t < nt; t += nw) {
      const int i0 = (t / NB) << 4, j0 = (t % NB) << 4;
      const dbl4 a = cov_tile(z, mD, ErT, i0, j0, BP);
      cov_put(sW, LD, 1, i0, j0, a, 1.0);
      cov_put(c.Wr + i * bb, BP, 1, i0, j0, a, 1.0);
    }
    __syncthreads();
    for (int t = wave; t < nt; t += nw) {
      const int i0 = (t / NB) << 4, j0 = (t % NB) << 4;
      cov_put(c.URd + i * bb, BP, 1, i0, j0, cov_tile(z, Er, mW, i0, j0, BP), 1.0);
    }
    __syncthreads();
  }
  if (!hasg) return;
  // W_g = Dinv G_i;  the border columns of UL_i, UR_i;  T_i = G_i^T W_g
  const int NG = GR >> 4, ntg = NB * NG;
  const CovMat Gi = cov_mat(c.G + i * bg, GR), GiT = cov_mat_t(c.G + i * bg, GR);
  for (int t = wave; t < ntg; t += nw) {
    const int i0 = (t / NG) << 4, j0 = (t % NG) << 4;
    const dbl4 a = cov_tile(z, mD, Gi, i0, j0, BP);
    cov_put(sW, LD, 1, i0, j0, a, 1.0);
    cov_put(c.Wg + i * bg, GR, 1, i0, j0, a, 1.0);
  }
  __syncthreads();
  for (int t = wave; t < ntg; t += nw) {
    const int i0 = (t / NG) << 4, j0 = (t % NG) << 4;
    cov_put(c.ULg + i * bg, GR, 1, i0, j0, cov_tile(z, EiT, mW, i0, j0, BP), 1.0);
    if (hr) cov_put(c.URg + i * bg, GR, 1, i0, j0, cov_tile(z, Er, mW, i0, j0, BP), 1.0);
  }
  for (int t = wave; t < NG * NG; t += nw) {
    const int i0 = (t / NG) << 4, j0 = (t % NG) << 4;
    cov_put(c.Tp + (size_t)i * GR * GR, GR, 1, i0, j0, cov_tile(z, GiT, mW, i0, j0, BP), 1.0);
  }
}

// chunk sums of the eliminated blocks' border terms T_i, i = 1 .. n - 1 in index order
__global__ __launch_bounds__(256) void k_cov_tsum(FteDims d, CovBufs c) {
  const int ch = blockIdx.x, GG = d.GR * d.GR, nb = d.nblk - 1;
  const int bc = (nb + CR_NCHUNK - 1) / CR_NCHUNK, b0 = 1 + ch * bc, b1 = min(d.nblk, b0 + bc);
  for (int e = threadIdx.x; e < GG; e += blockDim.x) {
    double v = 0.0;
    for (int b = b0; b < b1; ++b) v += c.Tp[(size_t)b * GG + e];
    c.partT[(size_t)ch * GG + e] = v;
  }
}

// The surviving block 0 with the border: S_00, S_0g, S_gg = blocks of [[D_0, G_0], [G_0^T, T]]^-1
__global__ __launch_bounds__(COV_THREADS) void k_cov_top(FteDims d, int hs, int hasg, CovBufs c) {
  const int BP = d.BP, GR = d.GR, NA = BP + GR, LD = NA + 1, GG = GR * GR;
  if (hs > 0) cov_apply_pending(d, c, 0, hs, hasg);
  extern __shared__ double lds[];
  for (int e = threadIdx.x; e < NA * NA; e += blockDim.x) {
    const int r = e / NA, q = e - r * NA;
    double v;
    if (r < BP && q < BP) {
      v = c.D[(size_t)r * BP + q];
    } else if (r < BP) {
      v = hasg ? c.G[(size_t)r * GR + q - BP] : 0.0;
    } else if (q < BP) {
      v = hasg ? c.G[(size_t)q * GR + r - BP] : 0.0;
    } else {
      const int g = (r - BP) * GR + q - BP;
      v = r == q ? 1.0 : 0.0;
      if (hasg) {
        double t = 0.0;
        for (int ch = 0; ch < CR_NCHUNK; ++ch) t += c.partT[(size_t)ch * GG + g];
        v = c.T0[g] - t;
      }
    }
    lds[r * LD + q] = v;
  }
  __syncthreads();
  wg_gj_inverse<true>(lds, LD, NA >> 4, nullptr, COV_BAD(c, GR));
  for (int e = threadIdx.x; e < NA * NA; e += blockDim.x) {
    const int r = e / NA, q = e - r * NA;
    const double v = lds[r * LD + q];
    if (r < BP && q < BP)
      c.Sii[(size_t)r * BP + q] = v;
    else if (r < BP)
      c.Sg[(size_t)r * GR + q - BP] = v;
    else if (q >= BP)
      c.Sgg[(r - BP) * GR + q - BP] = v;
  }
}

// One level of the down pass (step s): block i = s (2 blockIdx + 1) from l = i - s, r = i + s.
__global__ __launch_bounds__(COV_THREADS) void k_cov_down(FteDims d, int s, int hasg, CovBufs c) {
  const int BP = d.BP, GR = d.GR, n = d.nblk, NB = BP >> 4, NG = GR >> 4, LD = BP + 1;
  const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int i = s * (2 * (int)blockIdx.x + 1), l = i - s, r = i + s;
  const bool hr = r < n;
  const size_t bb = (size_t)BP * BP, bg = (size_t)BP * GR;
  extern __shared__ double lds[];
  double* sX = lds;                    // S_lr
  double* sY = lds + (size_t)BP * LD;  // S_il, S_ir, S_ig in turn
  const CovMat Wl = cov_mat(c.Wl + i * bb, BP), WlT = cov_mat_t(c.Wl + i * bb, BP);
  const CovMat Wr = cov_mat(c.Wr + i * bb, BP), WrT = cov_mat_t(c.Wr + i * bb, BP);
  const CovMat Wg = cov_mat(c.Wg + i * bg, GR), WgT = cov_mat_t(c.Wg + i * bg, GR);
  const CovMat Sll = cov_mat(c.Sii + l * bb, BP), Srr = cov_mat(c.Sii + (hr ? r : l) * bb, BP);
  const CovMat Slg = cov_mat(c.Sg + l * bg, GR), SlgT = cov_mat_t(c.Sg + l * bg, GR);
  const CovMat Srg = cov_mat(c.Sg + (hr ? r : l) * bg, GR), SrgT = cov_mat_t(c.Sg + (hr ? r : l) * bg, GR);
  const CovMat Sgg = cov_mat(c.Sgg, GR);
  const CovMat Slr = cov_mat(sX, LD), SlrT = cov_mat_t(sX, LD), mY = cov_mat(sY, LD);
  const dbl4 z = {0.0, 0.0, 0.0, 0.0};
  if (hr) {
    const double* src = c.Snx + l * bb;
    for (int e = threadIdx.x; e < BP * BP; e += blockDim.x) sX[(e / BP) * LD + e % BP] = src[e];
  }
  __syncthreads();
  const int nt = NB * NB;
  // the upper tiles of S_ii, at most COV_UT per wave, accumulated in registers over the phases
  constexpr int COV_UT = 2;  // 21 upper tiles at BP = 96 over 16 waves
  const int nut = NB * (NB + 1) / 2;
  dbl4 sacc[COV_UT];
  int ui[COV_UT], uj[COV_UT];
#pragma unroll
  for (int q = 0; q < COV_UT; ++q) {
    int t = wave + q * nw, I = 0;
    ui[q] = uj[q] = -1;
    if (t < nut) {
      while (t >= NB - I) {
        t -= NB - I;
        ++I;
      }
      ui[q] = I << 4;
      uj[q] = (I + t) << 4;
      const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) sacc[q][rr] = -c.Sii[i * bb + (size_t)(ui[q] + lk + 4 * rr) * BP + uj[q] + li];
    }
  }
  // S_il = -(W_l S_ll + W_r S_lr^T + W_g S_lg^T): kept as S_li = S_il^T for the pair (l, i)
  for (int t = wave; t < nt; t += nw) {
    const int i0 = (t / NB) << 4, j0 = (t % NB) << 4;
    dbl4 a = cov_tile(z, Wl, Sll, i0, j0, BP);
    if (hr) a = cov_tile(a, Wr, SlrT, i0, j0, BP);
    if (hasg) a = cov_tile(a, Wg, SlgT, i0, j0, GR);
    cov_put(sY, LD, 1, i0, j0, a, -1.0);
    cov_put(c.Snx + l * bb, 1, BP, i0, j0, a, -1.0);
  }
  __syncthreads();
  // the sign of sacc is flipped: sacc = -Dinv + S_il W_l^T + ...
#pragma unroll
  for (int q = 0; q < COV_UT; ++q)
    if (ui[q] >= 0) sacc[q] = cov_tile(sacc[q], mY, WlT, ui[q], uj[q], BP);
  __syncthreads();
  if (hr) {
    // S_ir = -(W_l S_lr + W_r S_rr + W_g S_rg^T)
    for (int t = wave; t < nt; t += nw) {
      const int i0 = (t / NB) << 4, j0 = (t % NB) << 4;
      dbl4 a = cov_tile(z, Wl, Slr, i0, j0, BP);
      a = cov_tile(a, Wr, Srr, i0, j0, BP);
      if (hasg) a = cov_tile(a, Wg, SrgT, i0, j0, GR);
      cov_put(sY, LD, 1, i0, j0, a, -1.0);
      cov_put(c.Snx + i * bb, BP, 1, i0, j0, a, -1.0);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < COV_UT; ++q)
      if (ui[q] >= 0) sacc[q] = cov_tile(sacc[q], mY, WrT, ui[q], uj[q], BP);
    __syncthreads();
  }
  if (hasg) {
    // S_ig = -(W_l S_lg + W_r S_rg + W_g S_gg)
    for (int t = wave; t < NB * NG; t += nw) {
      const int i0 = (t / NG) << 4, j0 = (t % NG) << 4;
      dbl4 a = cov_tile(z, Wl, Slg, i0, j0, BP);
      if (hr) a = cov_tile(a, Wr, Srg, i0, j0, BP);
      a = cov_tile(a, Wg, Sgg, i0, j0, GR);
      cov_put(sY, LD, 1, i0, j0, a, -1.0);
      cov_put(c.Sg + i * bg, GR, 1, i0, j0, a, -1.0);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < COV_UT; ++q)
      if (ui[q] >= 0) sacc[q] = cov_tile(sacc[q], mY, WgT, ui[q], uj[q], GR);
  }
  // S_ii: the upper tiles and their mirror images
#pragma unroll
  for (int q = 0; q < COV_UT; ++q)
    if (ui[q] >= 0) {
      cov_put(c.Sii + i * bb, BP, 1, ui[q], uj[q], sacc[q], -1.0);
      if (ui[q] != uj[q]) cov_put(c.Sii + i * bb, 1, BP, ui[q], uj[q], sacc[q], -1.0);
    }
}

// cov_x row f = the P x P diagonal sub-block of frame f in S_ii of its super-block (the two
// triangles averaged: exactly symmetric), and the extreme variances of the row
__global__ __launch_bounds__(256) void k_cov_gather(FteDims d, CovBufs c, double* __restrict__ cov_x) {
  const int f = blockIdx.x, P = d.P, BP = d.BP, a0 = (f % 3) * P;
  const double* S = c.Sii + (size_t)(f / 3) * BP * BP;
  double* o = cov_x + (size_t)f * P * P;
  for (int e = threadIdx.x; e < P * P; e += blockDim.x) {
    const int p = e / P, q = e - p * P;
    o[e] = 0.5 * (S[(size_t)(a0 + p) * BP + a0 + q] + S[(size_t)(a0 + q) * BP + a0 + p]);
  }
  if (threadIdx.x == 0) {
    double lo = S[(size_t)a0 * BP + a0], hi = lo;
    for (int p = 1; p < P; ++p) {
      const double v = S[(size_t)(a0 + p) * BP + a0 + p];
      lo = fmin(lo, v);
      hi = fmax(hi, v);
    }
    c.vmm[2 * f] = lo;
    c.vmm[2 * f + 1] = hi;
  }
}

// cov_tau (held rows and columns zero) and the report {pivots, free delays, var_min, var_max}
__global__ __launch_bounds__(256) void k_cov_report(FteDims d, int hasg, CovBufs c, double* __restrict__ cov_tau) {
  const int C = d.C, GR = d.GR, tid = threadIdx.x;
  if (cov_tau)
    for (int e = tid; e < C * C; e += blockDim.x) {
      const int r = e / C, q = e - r * C;
      double v = 0.0;
      if (hasg && !c.held[r] && !c.held[q]) v = 0.5 * (c.Sgg[r * GR + q] + c.Sgg[q * GR + r]);
      cov_tau[e] = v;
    }
  __shared__ double s_lo[256], s_hi[256];
  double lo = INFINITY, hi = -INFINITY;
  for (int f = 2 + tid; f < d.M; f += blockDim.x) {
    lo = fmin(lo, c.vmm[2 * f]);
    hi = fmax(hi, c.vmm[2 * f + 1]);
  }
  s_lo[tid] = lo;
  s_hi[tid] = hi;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) {
      s_lo[tid] = fmin(s_lo[tid], s_lo[tid + h]);
      s_hi[tid] = fmax(s_hi[tid], s_hi[tid + h]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    c.rep[0] = (double)*COV_BAD(c, GR);
    c.rep[1] = (double)(hasg ? *COV_NFREE(c, GR) : 0);
    c.rep[2] = s_lo[0];
    c.rep[3] = s_hi[0];
  }
}

// cov_marker[k][m] = J S J^T: J the 3 x P Jacobian of marker m at x = X row k + 2 (fk.hpp; no
// delay shift), S = cov_x row k + 2
__global__ __launch_bounds__(256) void k_cov_marker(FteDims d, const int* __restrict__ I, const double* __restrict__ Rl,
                                                    const double* __restrict__ X, const double* __restrict__ cov_x,
                                                    double* __restrict__ out) {
  __shared__ FkShared sh;
  __shared__ double sJ[FK_MAXN * 3 * FK_MAXP], sT[FK_MAXN * 3 * FK_MAXP], sS[FK_MAXP * FK_MAXP];
  const SkelView s = skel_view(I, Rl);
  const int k = blockIdx.x, tid = threadIdx.x, P = s.P, L = s.L;
  fk_frame(s, X + (size_t)(k + 2) * P, sh, tid, blockDim.x);
  const double* S = cov_x + (size_t)(k + 2) * P * P;
  for (int e = tid; e < P * P; e += blockDim.x) sS[e] = S[e];
  __syncthreads();
  for (int e = tid; e < L * P; e += blockDim.x) {
    const int m = e / P, q = e - m * P;
    double dd[3];
    fk_dpos(s, sh, s.outn[m], q, dd);
    sJ[(3 * m) * P + q] = dd[0];
    sJ[(3 * m + 1) * P + q] = dd[1];
    sJ[(3 * m + 2) * P + q] = dd[2];
  }
  __syncthreads();
  for (int e = tid; e < 3 * L * P; e += blockDim.x) {
    const int r = e / P, q = e - r * P;
    double v = 0.0;
    for (int p = 0; p < P; ++p) v = fma(sJ[r * P + p], sS[p * P + q], v);
    sT[e] = v;
  }
  __syncthreads();
  for (int e = tid; e < L * 9; e += blockDim.x) {
    const int m = e / 9, a = (e - 9 * m) / 3, b = e - 9 * m - 3 * a;
    double v = 0.0;
    for (int p = 0; p < P; ++p) v = fma(sT[(3 * m + a) * P + p], sJ[(3 * m + b) * P + p], v);
    out[((size_t)k * L + m) * 9 + 3 * a + b] = v;
  }
}

// the context's covariance store (grow-only; its own allocation, not the solve arena)
static double* cov_store(acs_ctx* ctx, size_t bytes) {
  if (ctx->fte_cov_bytes >= bytes) return (double*)ctx->fte_cov;
  if (ctx->fte_cov) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)acs_dev_free(ctx->fte_cov);
    ctx->fte_cov = nullptr;
    ctx->fte_cov_bytes = 0;
  }
  if (acs_dev_malloc(&ctx->fte_cov, bytes) != hipSuccess) {
    ctx->fte_cov = nullptr;
    acs_fail(ctx, ACS_E_NOMEM, "hipMalloc(%zu) failed for the FTE covariance store", bytes);
    return nullptr;
  }
  ctx->fte_cov_bytes = bytes;
  return (double*)ctx->fte_cov;
}

extern "C" int acs_fte_covariance(acs_ctx* ctx, const int32_t* skel_ints, int64_t n_ints, const double* skel_reals,
                                  int64_t n_reals, const double* cams, int32_t n_cams, const double* meas,
                                  const double* w, int32_t n_frames, int32_t shutter_delay, double Ts,
                                  const double* qinv, int32_t sd_mode, int32_t intermode, const double* X,
                                  const double* tau, double* cov_x, double* cov_tau, double* cov_marker,
                                  acs_fte_cov_report* report, uint32_t flags) {
  ACS_DEVICE_GUARD(ctx);
  ACS_FISHEYE_ONLY(ctx, flags, "acs_fte_covariance");
  ACS_CHECK(ctx, X && cov_x, "acs_fte_covariance: null X or cov_x");
  ACS_CHECK(ctx, !(shutter_delay && sd_mode == 1),
            "acs_fte_covariance: shutter_delay_mode 'variable' is not supported (the per-frame delays are "
            "eliminated inside the block build); use 'const' or no shutter delay");
  ACS_CHECK(ctx, !shutter_delay || tau, "acs_fte_covariance: shutter_delay needs tau");
  const FteProblem pb{skel_ints, n_ints, skel_reals, n_reals, cams, n_cams, meas, w, n_frames, shutter_delay, Ts, qinv,
                      sd_mode, intermode, X, tau, flags};
  FteSetup S;
  int rc;
  if ((rc = fte_setup(ctx, S, pb))) return rc;
  const FteDims& d = S.d;
  FteBuffers& b = S.b;
  hipStream_t s = ctx->stream;
  const int n = d.nblk, BP = d.BP, GR = d.GR, M = d.M, P = d.P, hasg = d.Cg > 0 ? 1 : 0;
  const size_t bb = (size_t)n * BP * BP, bg = (size_t)n * BP * GR, GG = (size_t)GR * GR;
  size_t off = 0;
  auto take = [&](size_t cnt) {
    const size_t o = off;
    off += (cnt + 31) / 32 * 32;
    return o;
  };
  const size_t oSii = take(bb), oSnx = take(bb), oWl = take(bb), oWr = take(bb), oWg = take(bg), oSg = take(bg),
               oSgg = take(GG), oT0 = take(GG), opA = take((size_t)CR_NCHUNK * std::max(tc_stride(d.Cg), 1)),
               opT = take((size_t)CR_NCHUNK * GG), ovm = take(2 * (size_t)M), orep = take(4), ohe = take(GR + 2);
  double* base = cov_store(ctx, off * sizeof(double));
  if (!base) return ACS_E_NOMEM;
  CovBufs c;
  c.Sii = base + oSii;
  c.Snx = base + oSnx;
  c.Wl = base + oWl;
  c.Wr = base + oWr;
  c.Wg = base + oWg;
  c.Sg = base + oSg;
  c.Sgg = base + oSgg;
  c.T0 = base + oT0;
  c.partA = base + opA;
  c.partT = base + opT;
  c.vmm = base + ovm;
  c.rep = base + orep;
  c.held = (int*)(base + ohe);
  c.D = b.Dc;
  c.E0 = b.Ec;
  c.E1 = b.Ec2;
  c.G = b.GBc;
  c.ULd = b.dL;
  c.ULg = b.dL + bb;
  c.URd = b.dR;
  c.URg = b.dR + bb;
  c.Tp = b.Tau;
  double* dcx = (double*)acs_out_buf(ctx, WS_OUT0, cov_x, sizeof(double) * M * P * P, flags);
  double* dct = cov_tau ? (double*)acs_out_buf(ctx, WS_OUT1, cov_tau, sizeof(double) * d.C * d.C, flags) : nullptr;
  double* dcm = cov_marker
                    ? (double*)acs_out_buf(ctx, WS_TMP0, cov_marker, sizeof(double) * (size_t)d.N * d.L * 9, flags)
                    : nullptr;
  if (!dcx || (cov_tau && !dct) || (cov_marker && !dcm)) return ACS_E_NOMEM;
  // the linearisation and the undamped blocks, D stored whole (acs_fte_debug_blocks' route)
  if ((rc = fte_upload_state(ctx, S, 0.0))) return rc;
  fte_launch_lin(d, s, b, 1, 0, d.N);
  cr_launch_assemble_build(d, S.n_cu, s, b, 1);
  if (hasg) hipLaunchKernelGGL(k_cov_frame_sums, dim3(CR_NCHUNK), dim3(256), 0, s, d, b.Tc, c.partA);
  hipLaunchKernelGGL(k_cov_prep, dim3(n), dim3(256), 0, s, d, b.tau, c);
  const size_t lds2 = sizeof(double) * 2 * (size_t)BP * (BP + 1);
  const size_t ldst = sizeof(double) * (size_t)(BP + GR) * (BP + GR + 1);
  const double* Ein = c.E0;
  double* Eout = c.E1;
  int sl = 1;
  for (int lv = 0; lv < d.nlev; ++lv, sl <<= 1) {
    const int ne = ((n - 1) / sl + 1) / 2, ns = sl > 1 ? (n - 1) / (2 * sl) + 1 : 0;
    hipLaunchKernelGGL(k_cov_up, dim3(ne + ns), dim3(COV_THREADS), lds2, s, d, sl, ne, hasg, c, Ein, Eout);
    double* t = const_cast<double*>(Ein);
    Ein = Eout;
    Eout = t;
  }
  if (hasg) hipLaunchKernelGGL(k_cov_tsum, dim3(CR_NCHUNK), dim3(256), 0, s, d, c);
  hipLaunchKernelGGL(k_cov_top, dim3(1), dim3(COV_THREADS), ldst, s, d, sl >> 1, hasg, c);
  for (int lv = d.nlev - 1; lv >= 0; --lv) {
    sl = 1 << lv;
    const int ne = ((n - 1) / sl + 1) / 2;
    hipLaunchKernelGGL(k_cov_down, dim3(ne), dim3(COV_THREADS), lds2, s, d, sl, hasg, c);
  }
  hipLaunchKernelGGL(k_cov_gather, dim3(M), dim3(256), 0, s, d, c, dcx);
  hipLaunchKernelGGL(k_cov_report, dim3(1), dim3(256), 0, s, d, hasg, c, dct);
  if (dcm)
    hipLaunchKernelGGL(k_cov_marker, dim3(d.N), dim3(256), 0, s, d, b.I, b.Rl, b.X, (const double*)dcx, dcm);
  ACS_HIP(ctx, hipGetLastError());
  if ((rc = acs_stage_out(ctx, cov_x, dcx, sizeof(double) * M * P * P, flags))) return rc;
  if (cov_tau && (rc = acs_stage_out(ctx, cov_tau, dct, sizeof(double) * d.C * d.C, flags))) return rc;
  if (cov_marker && (rc = acs_stage_out(ctx, cov_marker, dcm, sizeof(double) * (size_t)d.N * d.L * 9, flags)))
    return rc;
  if (report) {
    double rep[4];
    ACS_HIP(ctx, hipMemcpyAsync(rep, c.rep, sizeof(rep), hipMemcpyDeviceToHost, s));
    ACS_HIP(ctx, hipStreamSynchronize(s));
    report->n_bad_pivots = (int32_t)rep[0];
    report->n_tau_free = (int32_t)rep[1];
    report->var_min = rep[2];
    report->var_max = rep[3];
  } else if (!(flags & ACS_DEVICE_PTRS)) {
    ACS_HIP(ctx, hipStreamSynchronize(s));
  }
  return ACS_OK;
}
