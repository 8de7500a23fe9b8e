// sba.hip — points-only sparse bundle adjustment on gfx950.
//
// Replaces the numeric body of bundle_adjust_points_only (src/lib/sba.py:181-195):
// scipy least_squares(trf, loss='cauchy', f_scale=50) over cost_func_points_only
// (src/lib/sba.py:149-153). With the cameras fixed the Jacobian sparsity
// (src/lib/sba.py:11-22) is block-diagonal per 3-D point, so the solve is a batch of
// independent 3-parameter robust least-squares problems.
//
// Mapping: one point = one aligned group of G lanes (G = next pow2 of the observation
// slots, <= 64) — lane l owns slot l (+ j*G). Observations are an (n_pts, K) slot tensor
// (slot = camera for the dense core.sba layout) read once, coalesced, into registers;
// the camera records are staged in LDS (the HOIST instance loads each lane's record into its
// registers instead). Each LM iteration: every lane projects its
// observation(s) and forms its contribution to the gradient g = sum rho'(z) r J (3), the
// Gauss-Newton matrix H = sum max(rho' + 2 z rho'', 0.1 rho') J^T J (6; Triggs-corrected,
// which converges quadratically where IRLS weights only converge linearly) and the Cauchy
// cost (1); a butterfly __shfl_xor reduction inside the group gives every lane
// bit-identical sums, so all lanes take the same accept/reject decision with no LDS
// round trip and no atomics. The whole LM loop runs inside one launch: HBM traffic is
// the observation tensor once plus the points in and out.
// Small dense problems (3..8 slots, at most one wave per SIMD) take the ROW instances instead:
// one point per 16-lane DPP row and the same sums, in the butterfly's own order, by row
// broadcast (common.hpp), bit-identical and 30 issue slots per pass shorter.
//
// LM spec (shared with oracle/sba.py): lam0 = 1e-3, Marquardt damping H + lam*diag(H),
// xtol default 1e-9 (scipy's default, used by the reference, is 1e-8),
// accept on strict decrease (lam /= 10, floor 1e-15), reject (lam *= 10); stop on
// gtol / ftol / xtol / lam > 1e16 / max_iters.
#include <hipcub/hipcub.hpp>

#include "common.hpp"

// The ten sums of one linearisation (6 H, 3 g, the cost) inside an aligned group of G lanes,
// issued stage by stage: every value takes stage 1, then every value stage 2, and so on, so
// that no DPP move reads a register the add just before it wrote (a read-after-write hazard
// the hardware covers with s_nop wait states: issue slots of the lone wave). The additions and
// their order are those of group_sum<G> on each value. The last stage's addition is left to
// the caller for the first nine (v[i] + p[i] is the total): the LM pass adds them only where
// the step is accepted; v[9], the cost, is complete.
template <int G, int K>
__device__ __forceinline__ double group_partner(double v) {
  if constexpr (K == 0) return dpp_f64<0xB1>(v);        // quad_perm [1,0,3,2]
  else if constexpr (K == 1) return dpp_f64<0x4E>(v);   // quad_perm [2,3,0,1]
  else if constexpr (K == 2) return dpp_f64<0x141>(v);  // row_half_mirror
  else if constexpr (K == 3) return dpp_f64<0x140>(v);  // row_mirror
  else return __shfl_xor(v, 1 << K, G);
}
template <int G, int K = 0>
__device__ __forceinline__ void group_sum10(double (&v)[10], double (&p)[9]) {
  constexpr bool last = (2 << K) == G;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const double q = group_partner<G, K>(v[i]);
    if (last && i < 9)
      p[i] = q;
    else
      v[i] += q;
  }
  if constexpr (!last) group_sum10<G, K + 1>(v, p);
}

// (The row-broadcast sums of the ROW instances, row_pairs_cost / row_sums9 and the ACS_ROW_* pieces
// of the accept statement below, are in common.hpp, where the probe under tools/probe shares them.)
struct SbaParams {
  int max_iters;
  double f_scale, ftol, xtol, gtol;
};

// Diagnostic build only (tools/probe/lm_timeline_probe.hip defines ACS_LM_STAMPS and includes this
// file; the library is never built with it): the ROW instances read the shader clock at seven
// points of the wave's life and lane 0 of the wave stores them. ACS_STAMP_AFTER names the values the
// program has to hold at that point, so that the stamp stands behind their waits and arithmetic.
#ifdef ACS_LM_STAMPS
static unsigned long long* g_lm_stamps = nullptr;  // 8 words per wave, set by acs_sba_lm_stamps (probe)
#define ACS_STAMP(i) \
  if constexpr (ROW != 0) tk[i] = __builtin_amdgcn_s_memtime()
#define ACS_STAMP_AFTER(i, ...)              \
  if constexpr (ROW != 0) {                  \
    asm volatile("" ::__VA_ARGS__);          \
    tk[i] = __builtin_amdgcn_s_memtime();    \
  }
#define ACS_STAMPS_PARAM , unsigned long long* __restrict__ stamps
#define ACS_STAMPS_ARG(p) , p
#else
#define ACS_STAMP(i)
#define ACS_STAMP_AFTER(i, ...)
#define ACS_STAMPS_PARAM
#define ACS_STAMPS_ARG(p)
#endif

// HOIST: each lane keeps its camera record in registers for the whole LM loop instead of
// re-reading it from LDS in every projection (196 VGPRs: 2 waves per SIMD), chosen for
// grids of at most 2 waves per SIMD, where nothing else would fill the SIMD anyway.
// The other instances are not occupancy-bound either: <4, 3> (the configs[4] shape) holds 186
// VGPRs, 2 waves per SIMD, and register budgets for 2 / 3 / 4 waves per SIMD
// (amdgpu_waves_per_eu) ran it in 0.270 / 0.273 / 0.454 ms against 0.268-0.272 unconstrained
// (profiles/r06/bench_sba_w*_r06h.log): three independent slot chains per lane already keep the
// VALU issuing, and the 4-wave budget spills.
// Parameter order: the arguments the first vector loads need come first (observation, mask,
// point count, point, camera records, then the two counts), and the solution pointer right
// behind them, so that the kernel-argument preload this file is built with (build.py) hands all
// of them to the wave at launch: 14 dwords, as many as the user SGPRs hold, with no scalar load
// and its round trip ahead of the first address, and none ahead of the final store either (the
// last thing the slowest wave does; nothing in the wave has touched that line of the
// kernel-argument segment before, and each graph node has a segment of its own). camid, null
// in every instance without camera ids and read after the first round only, comes behind the
// preloaded ones with the LM parameters and the report's pointers.
// ROW (0, or the number of lane pairs 2..4): the row-broadcast sums of common.hpp in place of the
// butterfly. G = 16 (one point per DPP row), S = 1, no camera ids, HOIST only: the instance for
// latency-bound grids, where a wave of 4 points instead of 8 costs nothing (run_lm).
// MODEL (ACS_MODEL_*): the projection, the record stride and the place of the null record's 1.0.
// The standard model has the LDS-staged butterfly instances only: the HOIST and ROW instances'
// null-record moves are written out for the 20 doubles of a fisheye record.
template <int G, int S, bool CAMID, bool HOIST, int ROW = 0, int MODEL = ACS_MODEL_FISHEYE>
__global__ __launch_bounds__(256) void k_sba_lm(const double2* __restrict__ uv,
                                                const uint8_t* __restrict__ mask, int64_t n_pts,
                                                const double* pts_in, const double* __restrict__ cams,
                                                int K, int C,
                                                double* pts,  // may alias pts_in
                                                const uint8_t* __restrict__ camid, SbaParams prm,
                                                double* __restrict__ cost0, double* __restrict__ cost1,
                                                int* __restrict__ stat ACS_STAMPS_PARAM) {
#ifdef ACS_LM_STAMPS
  [[maybe_unused]] unsigned long long tk[7] = {0, 0, 0, 0, 0, 0, 0};
  [[maybe_unused]] const unsigned long long rt0 = __builtin_amdgcn_s_memrealtime();
#endif
  ACS_STAMP(0);  // entry
  static_assert(ROW == 0 || (G == 16 && S == 1 && !CAMID && HOIST), "ROW: 16-lane rows, one slot per lane, hoisted records");
  static_assert(MODEL == 0 || (!HOIST && ROW == 0), "standard model: LDS-staged butterfly instances only");
  constexpr int CS = CamRec<MODEL>::stride;
  extern __shared__ double s_cam[];
  // every kernel argument the address computations need, requested before the first scalar
  // wait: left alone, the compiler loads each where the first branch that uses it begins,
  // three dependent scalar-load rounds ahead of the two vector rounds
  // (the HOIST instances are launched in blocks of one wave: the block size is then no hidden
  // argument to load either, and with the preload none of these is a load)
  const unsigned bdim = HOIST ? 64u : blockDim.x;
  asm volatile("" ::"s"(cams), "s"(uv), "s"(mask), "s"(pts_in), "s"(n_pts), "s"(C), "s"(K), "s"(bdim));
  const int lane = threadIdx.x & (G - 1);
  const int64_t p = ((int64_t)blockIdx.x * bdim + threadIdx.x) / G;
  const bool live = p < n_pts;
  // the slot's observation, its mask and camera id, and the point (none depends on another),
  // then the camera records: two round trips, since the compiler ends the block below with a
  // wait for the mask byte and issues the point's and the records' loads behind it. One round
  // from clamped indices, with slot < K and the mask as selects, was measured for the HOIST
  // instances and not kept.
  double2 q[S];
  uint8_t mk[S], cid[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int slot = lane + s * G;
    q[s] = double2{0.0, 0.0};
    mk[s] = 0;
    cid[s] = (uint8_t)slot;
    if (live && slot < K) {
      const int64_t o = p * K + slot;
      mk[s] = mask[o];
      q[s] = uv[o];
      if (CAMID) cid[s] = camid[o];
    }
  }
  ACS_STAMP_AFTER(1, "v"((int)mk[0]));  // after the first vector wait (the mask byte)
  double x0 = 0.0, x1 = 0.0, x2 = 0.0;
  if (live) {
    x0 = pts_in[3 * p];
    x1 = pts_in[3 * p + 1];
    x2 = pts_in[3 * p + 2];
  }
  // the null camera (record C): R = 0, t = (0, 0, 1), K = 0. Slots without an observation
  // project through it to u = v = 0 with a zero Jacobian, so with a zero observation they add
  // exact zeros to every sum: linearize() needs no branch around its projection
  double cr[HOIST ? S : 1][ACS_CAM_STRIDE];
  if constexpr (HOIST) {
    // S = 1 and slot = camera: the lane's record is loaded from global memory (L2-resident,
    // C x 160 B) in the same round trip as the observation, straight into its registers; no
    // LDS copy and no barrier ahead of the LM loop
    const double* cg = cams + (size_t)(lane < C ? lane : C - 1) * ACS_CAM_STRIDE;
#pragma unroll
    for (int i = 0; i < ACS_CAM_STRIDE; ++i) cr[0][i] = cg[i];
    if (!live) return;  // whole group leaves together
  } else {
    for (int i = threadIdx.x; i < C * CS; i += blockDim.x) s_cam[i] = cams[i];
    if (threadIdx.x < CS) s_cam[C * CS + threadIdx.x] = threadIdx.x == CS - 1 ? 1.0 : 0.0;
    __syncthreads();
    if (!live) return;  // whole group leaves together
  }

  double ou[S], ov[S];
  const double* oc[S];
  bool ok[S];
  int mine = 0;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int slot = lane + s * G;
    const int cam = cid[s];
    ok[s] = slot < K && mk[s] && cam < C;
    ou[s] = ok[s] ? q[s].x : 0.0;
    ov[s] = ok[s] ? q[s].y : 0.0;
    oc[s] = s_cam + (ok[s] ? cam : C) * CS;
    mine += ok[s] ? 1 : 0;
  }
  // a point without any observation: no lane of its group has one (the lanes of a dead
  // group have left, and a ballot counts them as zero). It takes no path of its own ahead of
  // the loop, where the branch would stand between the loads and everything that can run
  // under their latency: all its slots are the null camera, its sums are exact zeros, a
  // max_iters of 0 ends it at the first exit of the first pass with its point untouched, and
  // its report is set right after the loop.
  const unsigned long long has = __ballot(mine > 0);
  const unsigned long long grp = G == 64 ? ~0ull : (1ull << (G & 63)) - 1ull;
  const bool noobs = ((has >> (threadIdx.x & 63 & ~(G - 1))) & grp) == 0ull;
  const int max_iters = noobs ? 0 : prm.max_iters;
  // f_scale is not preloaded: its scalar load is waited for where the value is first used. The
  // HOIST instances pass it through the null-record statement below, so that this wait and the
  // f_scale^2, 1 / f_scale^2 chain stand behind the constant set-up that runs under the load
  // latency, not ahead of it
  double fs = prm.f_scale;
  if constexpr (HOIST) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
      // the null record over the loaded one: 20 64-bit moves under one saved exec mask, in
      // place of 40 32-bit selects and the moves that hold their constants. One asm statement
      // and no branch, so that the scheduler still places it, and the wait for the record's
      // loads that it needs, behind the constant set-up that runs under the load latency.
      static_assert(ACS_CAM_STRIDE == 20, "the null-record moves below are written out for 20 doubles");
      const unsigned long long nul = __ballot(!ok[s]);
      unsigned long long sv;
      double* c = cr[s];
      asm("s_and_saveexec_b64 %[sv], %[nul]\n\t"
          "v_mov_b64 %0, 0\n\tv_mov_b64 %1, 0\n\tv_mov_b64 %2, 0\n\tv_mov_b64 %3, 0\n\t"
          "v_mov_b64 %4, 0\n\tv_mov_b64 %5, 0\n\tv_mov_b64 %6, 0\n\tv_mov_b64 %7, 0\n\t"
          "v_mov_b64 %8, 0\n\tv_mov_b64 %9, 0\n\tv_mov_b64 %10, 0\n\tv_mov_b64 %11, 0\n\t"
          "v_mov_b64 %12, 0\n\tv_mov_b64 %13, 0\n\tv_mov_b64 %14, 0\n\tv_mov_b64 %15, 0\n\t"
          "v_mov_b64 %16, 0\n\tv_mov_b64 %17, 0\n\tv_mov_b64 %18, 0\n\tv_mov_b64 %19, 1.0\n\t"
          "s_mov_b64 exec, %[sv]"
          : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(c[4]), "+v"(c[5]), "+v"(c[6]), "+v"(c[7]),
            "+v"(c[8]), "+v"(c[9]), "+v"(c[10]), "+v"(c[11]), "+v"(c[12]), "+v"(c[13]), "+v"(c[14]), "+v"(c[15]),
            "+v"(c[16]), "+v"(c[17]), "+v"(c[18]), "+v"(c[19]), [sv] "=&s"(sv), "+s"(fs)
          : [nul] "s"(nul)
          : "scc");
    }
  }
  const double f2 = fs * fs;
  const double if2 = 1.0 / f2;
  // after the last vector wait: the point, the observation and (through the statement above) the record
  ACS_STAMP_AFTER(2, "v"(x0), "v"(x1), "v"(x2), "v"(ou[0]), "v"(ov[0]), "v"(cr[0][0]), "v"(cr[0][19]));

  // One pass over the observations at X: robust cost, Triggs-weighted GN matrix (packed
  // upper 3x3) and IRLS gradient, group-reduced. The trial point of every LM iteration is
  // linearised speculatively, so an accepted step (the common case) costs one projection.
  auto linearize = [&](double X0, double X1, double X2, double (&v)[10], double (&vp)[9], double& Fo) {
    double Ho[6], go[3];
#pragma unroll
    for (int i = 0; i < 6; ++i) Ho[i] = 0.0;
    go[0] = go[1] = go[2] = 0.0;
    double Fl;
    // S > 1: the lane's slots share one logarithm too. With T = prod_s (1 + t_s) - 1 formed as
    // T + t + T t (exact algebra, relative rounding only), sum_s log1p(t_s) = log1p(T), and
    // prod_s 1 / (1 + t_s) is the reciprocal it needs. An empty slot (t = 0, 1 / (1 + t) = 1)
    // leaves both unchanged exactly.
    double Tl = 0.0, rTl = 1.0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      // slots without an observation: the null camera, exact zero contributions
      double pu, pv, J[6];
      if constexpr (MODEL == ACS_MODEL_STANDARD)
        standard_uvj(oc[s], X0, X1, X2, pu, pv, J);
      else if constexpr (HOIST)
        fisheye_uvj(cr[s], X0, X1, X2, pu, pv, J);
      else
        fisheye_uvj(oc[s], X0, X1, X2, pu, pv, J);
      const double r[2] = {pu - ou[s], pv - ov[s]};
      const double zu = r[0] * r[0] * if2, zv = r[1] * r[1] * if2;
      // log1p(zu) + log1p(zv) with one logarithm, and the two Cauchy weights 1 / (1 + z) from
      // the logarithm's own reciprocal of (1 + zu)(1 + zv)
      const double t = zu + zv + zu * zv, u1 = 1.0 + t, ru = rcp_nr(u1);
      if constexpr (S == 1) {
        Fl = log1p_pos_ur(t, u1, ru);
      } else {
        Tl = s == 0 ? t : fma(Tl, t, Tl + t);
        rTl = s == 0 ? ru : rTl * ru;
      }
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        const double z = d ? zv : zu;
        const double w = (d ? 1.0 + zu : 1.0 + zv) * ru;    // rho'(z): gradient weight
        const double wh = fmax((1.0 - z) * w * w, 0.1 * w);  // rho' + 2 z rho'' (Triggs), floored
        const double j0 = J[3 * d], j1 = J[3 * d + 1], j2 = J[3 * d + 2];
        const double hj0 = wh * j0, hj1 = wh * j1, hj2 = wh * j2;
        Ho[0] += hj0 * j0;
        Ho[1] += hj0 * j1;
        Ho[2] += hj0 * j2;
        Ho[3] += hj1 * j1;
        Ho[4] += hj1 * j2;
        Ho[5] += hj2 * j2;
        const double wr = w * r[d];
        go[0] += wr * j0;
        go[1] += wr * j1;
        go[2] += wr * j2;
      }
    }
    if constexpr (S > 1) Fl = log1p_pos_ur(Tl, 1.0 + Tl, rTl);
#pragma unroll
    for (int i = 0; i < 6; ++i) v[i] = Ho[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) v[6 + i] = go[i];
    v[9] = Fl;
    if constexpr (ROW) {
      // the compiler places the 32-bit quad_perm moves (and sees their hazards); v becomes the
      // pair sums, vp stays unused
      double qp[10];
#pragma unroll
      for (int i = 0; i < 10; ++i) qp[i] = dpp_f64<0xB1>(v[i]);
      Fo = 0.5 * f2 * row_pairs_cost<ROW>(v, qp, 1.0);
    } else {
      group_sum10<G>(v, vp);
      Fo = 0.5 * f2 * v[9];
    }
    // the cost is this rounded product wherever it is used: not fused into F - Fn of the ftol test
    asm("" : "+v"(Fo));
  };

  double H[6], g[3], F;
  {
    double v[10], vp[9];
    linearize(x0, x1, x2, v, vp, F);
    if constexpr (ROW) {
      row_sums9<ROW>(H, g, v, 1.0);
    } else {
#pragma unroll
      for (int i = 0; i < 6; ++i) H[i] = v[i] + vp[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) g[i] = v[6 + i] + vp[6 + i];
    }
  }
  const double F_before = F;
  double lam = 1e-3;
  int status = ACS_STATUS_RUNNING, iters = 0, nfev = 1;
  ACS_STAMP_AFTER(3, "v"(F), "v"(H[0]), "v"(H[1]), "v"(H[2]), "v"(H[3]), "v"(H[4]), "v"(H[5]), "v"(g[0]), "v"(g[1]),
                  "v"(g[2]));  // loop entry
  // One pass = solve, stopping tests on the solve, trial linearisation, accept / reject. The
  // pass is straight-line code with two exits (after the solve; at the end): a lone wave pays
  // an issue slot for every exec-mask instruction and branch, so a pass that cannot step (not
  // positive definite) is a predicate on the same code, not a path of its own.
  while (true) {
    const double gmax = fmax(fabs(g[0]), fmax(fabs(g[1]), fabs(g[2])));
    // |x| for the xtol test of this pass depends on x alone: formed here, its reciprocal square
    // root (a seed and seven dependent operations) issues in the stalls of the Cholesky's own
    // dependent chain instead of standing as a chain of its own behind the trial.
    // |x| = xx / sqrt(xx) without a branch or select for xx = 0: the smallest normal number
    // stands in for it, and 0 times its finite reciprocal root is exactly 0 (an xx below it
    // is an |x| below 1.5e-154, which xtol + |x| rounds away either way)
    const double xx = x0 * x0 + x1 * x1 + x2 * x2;
    double xs = prm.xtol + xx * rsq_nr(fmax(xx, 2.2250738585072014e-308));  // xtol + |x|
    asm volatile("" : "+v"(xs));  // stays here: not sunk behind the first exit again
    // Cholesky of H + lam*diag(H)
    const double dl = 1.0 + lam;
    const double a00 = H[0] * dl, a11 = H[3] * dl, a22 = H[5] * dl;
    // reciprocal Cholesky diagonal, unguarded: a pivot that is not positive makes its
    // reciprocal square root, and all that follows from it, infinite or NaN garbage, and
    // clears pd, the predicate on every use of the step below (uniform over the group: it
    // comes from the group-summed H)
    const double i00 = rsq_nr(a00);
    const double L10 = H[1] * i00, L20 = H[2] * i00;
    const double d11 = a11 - L10 * L10;
    const double i11 = rsq_nr(d11);
    const double L21 = (H[4] - L20 * L10) * i11;
    const double d22 = a22 - L20 * L20 - L21 * L21;
    const double i22 = rsq_nr(d22);
    const bool pd = a00 > 0.0 && d11 > 0.0 && d22 > 0.0;
    // pd as a wave mask, for the ROW instances' accept statement
    [[maybe_unused]] const unsigned long long pdm = ROW ? __ballot(pd) : 0ull;
    const double y0 = -g[0] * i00;
    const double y1 = (-g[1] - L10 * y0) * i11;
    const double y2 = (-g[2] - L20 * y0 - L21 * y1) * i22;
    double dx2 = y2 * i22;
    double dx1 = (y1 - L21 * dx2) * i11;
    double dx0 = (y0 - L10 * dx1 - L20 * dx2) * i00;
    // the step's products are rounded before anything is added to them (x + dx below is an
    // addition of the rounded step, never a multiply-add fused with the last product above)
    asm volatile("" : "+v"(dx0), "+v"(dx1), "+v"(dx2));
    // model decrease of the step, -g.dx - dx.H.dx/2: below the resolution of the
    // float64 cost the step can only be accepted or rejected by rounding -> converged.
    // From the damped system the step solves, (H + lam D) dx = -g with D = diag(H):
    // dx.H.dx = -g.dx - lam dx.D.dx, so the decrease is sum_i dx_i (lam H_ii dx_i - g_i) / 2,
    // no H.dx and no difference of two nearly equal sums. Only used under pd, where the step
    // is that solution.
    const double pred = 0.5 * (dx0 * (lam * H[0] * dx0 - g[0]) + dx1 * (lam * H[3] * dx1 - g[1]) +
                               dx2 * (lam * H[5] * dx2 - g[2]));
    // first exit: max_iters, gtol or the cost resolution; which of them is sorted out after
    // the loop (status is still RUNNING here), not with three selects in every pass
    if ((iters >= max_iters) | (gmax <= prm.gtol) | (pd & (pred <= ACS_COST_RES * F))) break;
    ++iters;
    const double n0 = x0 + dx0, n1 = x1 + dx1, n2 = x2 + dx2;
    double vn[10], vq[9], Fn;
    linearize(n0, n1, n2, vn, vq, Fn);
    // not positive definite: no step, so the trial does not count, there is no xtol test, and
    // lam rises as for a rejection
    nfev += pd ? 1 : 0;
    // |dx| <= xtol (xtol + |x|), compared squared
    const double xb = prm.xtol * xs;
    const bool small = pd && dx0 * dx0 + dx1 * dx1 + dx2 * dx2 <= xb * xb;
    const bool acc = pd && Fn < F;
    const bool fconv = acc && (F - Fn) <= prm.ftol * F;
    lam = acc ? fmax(lam * 0.1, 1e-15) : lam * 10.0;
    // An accepted step, without a branch and without a copy: x and F move once and the last
    // stage of the nine H and g sums is added, all into their own registers (tied operands)
    // under the exec mask of the accepting lanes, so that "keep the old value" is the absence
    // of a write. Written as assignments under if (acc), the compiler keeps a second copy of
    // x and F for the loop's two exits (four moves before the trial, four in the block and
    // four behind it, in every pass) and pays the branch's mask bookkeeping around it.
    // ROW: the nine sums themselves are taken under that mask (a row accepts or rejects as a
    // whole, so every lane a broadcast reads is enabled): the first term's v_mov_b64_dpp is the
    // move into H and g, and a rejected pass pays for no sum but the cost's.
    if constexpr (ROW) {
      // the accepting lanes as the wave mask of the comparison itself, and pd's mask formed with
      // the solve: the ballot of their conjunction is a select and a compare more, on the chain
      // from the cost's sum to the first instruction under the mask
      const unsigned long long am = __builtin_amdgcn_ballot_w64(Fn < F) & pdm;
      unsigned long long sv;
      const double one = 1.0;
      const double(&s)[10] = vn;
#define ACS_ROW_ACCEPT(SUMS, ...)                                                                          \
  asm("s_and_saveexec_b64 %[sv], %[am]\n\t"                                                                \
      "v_mov_b64 %[x0], %[n0]\n\tv_mov_b64 %[x1], %[n1]\n\tv_mov_b64 %[x2], %[n2]\n\t"                    \
      "v_mov_b64 %[F], %[Fn]\n\t" SUMS "s_mov_b64 exec, %[sv]"                                             \
      : [x0] "+v"(x0), [x1] "+v"(x1), [x2] "+v"(x2), [F] "+v"(F), ACS_ROW_H("+v"), [sv] "=&s"(sv) __VA_ARGS__ \
      : [am] "s"(am), [n0] "v"(n0), [n1] "v"(n1), [n2] "v"(n2), [Fn] "v"(Fn), ACS_ROW_S                    \
      : "scc")
      if constexpr (ROW == 2) {
        ACS_ROW_ACCEPT(ACS_ROW_SUMS2);
      } else if constexpr (ROW == 3) {
        ACS_ROW_ACCEPT(ACS_ROW_SUMS3);
      } else {
        double t[9];
        ACS_ROW_ACCEPT(ACS_ROW_SUMS4, , ACS_ROW_T);
      }
#undef ACS_ROW_ACCEPT
    } else {
      const unsigned long long am = __ballot(acc);
      unsigned long long sv;
      asm("s_and_saveexec_b64 %[sv], %[am]\n\t"
          "v_mov_b64 %[x0], %[n0]\n\tv_mov_b64 %[x1], %[n1]\n\tv_mov_b64 %[x2], %[n2]\n\t"
          "v_mov_b64 %[F], %[Fn]\n\t"
          "v_add_f64 %[h0], %[a0], %[b0]\n\tv_add_f64 %[h1], %[a1], %[b1]\n\t"
          "v_add_f64 %[h2], %[a2], %[b2]\n\tv_add_f64 %[h3], %[a3], %[b3]\n\t"
          "v_add_f64 %[h4], %[a4], %[b4]\n\tv_add_f64 %[h5], %[a5], %[b5]\n\t"
          "v_add_f64 %[g0], %[a6], %[b6]\n\tv_add_f64 %[g1], %[a7], %[b7]\n\t"
          "v_add_f64 %[g2], %[a8], %[b8]\n\t"
          "s_mov_b64 exec, %[sv]"
          : [x0] "+v"(x0), [x1] "+v"(x1), [x2] "+v"(x2), [F] "+v"(F), [h0] "+v"(H[0]), [h1] "+v"(H[1]),
            [h2] "+v"(H[2]), [h3] "+v"(H[3]), [h4] "+v"(H[4]), [h5] "+v"(H[5]), [g0] "+v"(g[0]), [g1] "+v"(g[1]),
            [g2] "+v"(g[2]), [sv] "=&s"(sv)
          : [am] "s"(am), [n0] "v"(n0), [n1] "v"(n1), [n2] "v"(n2), [Fn] "v"(Fn), [a0] "v"(vn[0]), [a1] "v"(vn[1]),
            [a2] "v"(vn[2]), [a3] "v"(vn[3]), [a4] "v"(vn[4]), [a5] "v"(vn[5]), [a6] "v"(vn[6]), [a7] "v"(vn[7]),
            [a8] "v"(vn[8]), [b0] "v"(vq[0]), [b1] "v"(vq[1]), [b2] "v"(vq[2]), [b3] "v"(vq[3]), [b4] "v"(vq[4]),
            [b5] "v"(vq[5]), [b6] "v"(vq[6]), [b7] "v"(vq[7]), [b8] "v"(vq[8])
          : "scc");
    }
    // second exit, rising priority: stalled (lam only passes 1e16 on a pass without an
    // accepted step), xtol, ftol of an accepted step
    status = lam > 1e16 ? ACS_STATUS_STALLED : ACS_STATUS_RUNNING;
    status = small ? ACS_STATUS_XTOL : status;
    status = fconv ? ACS_STATUS_FTOL : status;
    if (status != ACS_STATUS_RUNNING) break;
  }
  ACS_STAMP_AFTER(4, "v"(x0), "v"(x1), "v"(x2), "v"(F), "v"(status), "v"(iters));  // loop exit
  ACS_STAMP(5);                                                                     // before the wait ahead of the store
  if (lane == 0) {
    ACS_STAMP_AFTER(6, "s"(pts));  // after it
#ifdef ACS_LM_STAMPS
    if constexpr (ROW != 0) {
      if (stamps && threadIdx.x == 0) {  // one wave per block
        unsigned long long* w = stamps + 8 * (size_t)blockIdx.x;
        for (int i = 0; i < 7; ++i) w[i] = tk[i];
        w[7] = __builtin_amdgcn_s_memrealtime() - rt0;
      }
    }
#endif
    pts[3 * p] = x0;
    pts[3 * p + 1] = x1;
    pts[3 * p + 2] = x2;
    // the per-point costs and status feed k_sba_report only: not written (28 B per point)
    // when no report is asked for, and the status of a first-exit leave is not resolved then
    if (stat) {
      if (status == ACS_STATUS_RUNNING) {
        // left at the first exit (g is the one tested there), in the order of its tests
        const double gmax = fmax(fabs(g[0]), fmax(fabs(g[1]), fabs(g[2])));
        status = iters >= max_iters ? ACS_STATUS_MAXITER : gmax <= prm.gtol ? ACS_STATUS_GTOL : ACS_STATUS_FTOL;
      }
      cost0[p] = noobs ? 0.0 : F_before;
      cost1[p] = noobs ? 0.0 : F;
      stat[3 * p] = noobs ? ACS_STATUS_NOOBS : status;
      stat[3 * p + 1] = iters;
      stat[3 * p + 2] = noobs ? 0 : nfev;
    }
  }
}

// Deterministic single-block reduction of the per-point outputs into an acs_report.
__global__ __launch_bounds__(256) void k_sba_report(const double* __restrict__ cost0,
                                                    const double* __restrict__ cost1,
                                                    const int* __restrict__ stat, int64_t n,
                                                    acs_report* __restrict__ rep) {
  __shared__ double s_c0[256], s_c1[256];
  __shared__ long long s_i[256][ACS_N_STATUS + 3];
  const int t = threadIdx.x;
  double c0 = 0.0, c1 = 0.0;
  long long cnt[ACS_N_STATUS] = {0}, isum = 0, imax = 0, nf = 0;
  for (int64_t i = t; i < n; i += 256) {
    c0 += cost0[i];
    c1 += cost1[i];
    int s = stat[3 * i];
    if (s >= 0 && s < ACS_N_STATUS) cnt[s]++;
    isum += stat[3 * i + 1];
    imax = max(imax, (long long)stat[3 * i + 1]);
    nf += stat[3 * i + 2];
  }
  s_c0[t] = c0;
  s_c1[t] = c1;
  for (int k = 0; k < ACS_N_STATUS; ++k) s_i[t][k] = cnt[k];
  s_i[t][ACS_N_STATUS] = isum;
  s_i[t][ACS_N_STATUS + 1] = imax;
  s_i[t][ACS_N_STATUS + 2] = nf;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) {
      s_c0[t] += s_c0[t + h];
      s_c1[t] += s_c1[t + h];
      for (int k = 0; k < ACS_N_STATUS + 3; ++k) {
        if (k == ACS_N_STATUS + 1)
          s_i[t][k] = max(s_i[t][k], s_i[t + h][k]);
        else
          s_i[t][k] += s_i[t + h][k];
      }
    }
    __syncthreads();
  }
  if (t == 0) {
    rep->n_problems = n;
    for (int k = 0; k < ACS_N_STATUS; ++k) rep->status_counts[k] = s_i[0][k];
    rep->iters_sum = s_i[0][ACS_N_STATUS];
    rep->iters_max = s_i[0][ACS_N_STATUS + 1];
    rep->nfev_sum = s_i[0][ACS_N_STATUS + 2];
    rep->cost_before = s_c0[0];
    rep->cost_after = s_c1[0];
  }
}

// ------------------------------------------------------------------------------------
// obs list -> (n_pts, K) slot tensor, deterministic (stable radix sort by point index)
// ------------------------------------------------------------------------------------
__global__ void k_iota(int32_t* v, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = (int32_t)i;
}
__global__ void k_count(const int32_t* __restrict__ key, int64_t n, int32_t* __restrict__ cnt, int64_t n_pts,
                        int32_t* __restrict__ bad) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int32_t k = key[i];
  if (k < 0 || k >= n_pts) {
    atomicAdd(bad, 1);
    return;
  }
  atomicAdd(&cnt[k], 1);
}
__global__ void k_scatter_slots(const int32_t* __restrict__ skey, const int32_t* __restrict__ sval, int64_t n,
                                const int32_t* __restrict__ start, const double2* __restrict__ uv,
                                const int32_t* __restrict__ cam_idx, int K, int n_cams,
                                double2* __restrict__ uv_pad, uint8_t* __restrict__ mask,
                                uint8_t* __restrict__ camid) {
  int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int32_t p = skey[j];
  const int32_t o = sval[j];
  const int64_t slot = j - start[p];
  const int64_t d = (int64_t)p * K + slot;
  const int c = cam_idx[o];
  uv_pad[d] = uv[o];
  camid[d] = (uint8_t)(c >= 0 && c < n_cams ? c : 255);
  mask[d] = (c >= 0 && c < n_cams) ? 1 : 0;
}


// residual vector in the caller's observation order (cost_func_points_only, src/lib/sba.py:149-153)
template <int MODEL>
__global__ __launch_bounds__(256) void k_residuals_ext(const double* __restrict__ cams, int n_cams,
                                                       const double* __restrict__ uvobs,
                                                       const int32_t* __restrict__ pt_idx,
                                                       const int32_t* __restrict__ cam_idx, int64_t n_obs,
                                                       const double* __restrict__ pts, int64_t n_pts,
                                                       double* __restrict__ res) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_obs) return;
  const int c = cam_idx[i];
  const int64_t p = pt_idx[i];
  if (c < 0 || c >= n_cams || p < 0 || p >= n_pts) {
    res[2 * i] = res[2 * i + 1] = __builtin_nan("");
    return;
  }
  ProjOut o;
  model_project<MODEL, false>(cams + c * CamRec<MODEL>::stride, pts[3 * p], pts[3 * p + 1], pts[3 * p + 2], o);
  res[2 * i] = o.u - uvobs[2 * i];
  res[2 * i + 1] = o.v - uvobs[2 * i + 1];
}

static int next_pow2(int v) {
  int g = 1;
  while (g < v) g <<= 1;
  return g;
}

template <int G, int S, bool CAMID, int MODEL>
static void launch_lm_t(acs_ctx* ctx, int blocks, int block, const double* cams, int C, int K, const double2* uv,
                        const uint8_t* mask, const uint8_t* camid, int64_t n_pts, const double* pts_in, double* pts,
                        SbaParams prm, double* c0, double* c1, int* st) {
  // register-resident camera records when the grid holds at most 2 waves per SIMD
  const int64_t waves = (n_pts * G + 63) / 64;
  // (fisheye records only: the standard model always takes the LDS-staged instance)
  const bool hoist = MODEL == ACS_MODEL_FISHEYE && S == 1 && !CAMID && G <= 16 && waves <= 8 * (int64_t)ctx->n_cu;
  if constexpr (MODEL == ACS_MODEL_FISHEYE && S == 1 && !CAMID && G <= 16) {
    if (hoist) {
      // one wave per block, the size the kernel assumes (what run_lm picks for every grid of
      // fewer than 2 waves per SIMD anyway)
      block = 64;
      blocks = acs_grid(n_pts * G, block);
      hipLaunchKernelGGL((k_sba_lm<G, S, CAMID, true>), dim3(blocks), dim3(block),
                         sizeof(double) * ACS_CAM_STRIDE * (C + 1), ctx->stream, uv, mask, n_pts, pts_in, cams, K, C, pts,
                         camid, prm, c0, c1, st ACS_STAMPS_ARG(nullptr));
      return;
    }
  }
  hipLaunchKernelGGL((k_sba_lm<G, S, CAMID, false, 0, MODEL>), dim3(blocks), dim3(block),
                     sizeof(double) * CamRec<MODEL>::stride * (C + 1), ctx->stream, uv, mask, n_pts, pts_in, cams, K, C,
                     pts, camid, prm, c0, c1, st ACS_STAMPS_ARG(nullptr));
}

template <int S, bool CAMID, int MODEL>
static int launch_lm_g(acs_ctx* ctx, int G, int blocks, int block, const double* cams, int C, int K,
                       const double2* uv, const uint8_t* mask, const uint8_t* camid, int64_t n_pts,
                       const double* pts_in, double* pts, SbaParams prm, double* c0, double* c1, int* st) {
  switch (G) {
#define ACS_G(g)                                                                                      \
  case g:                                                                                             \
    launch_lm_t<g, S, CAMID, MODEL>(ctx, blocks, block, cams, C, K, uv, mask, camid, n_pts, pts_in, pts, prm, c0, c1, st); \
    break;
    ACS_G(2) ACS_G(4) ACS_G(8) ACS_G(16) ACS_G(32) ACS_G(64)
#undef ACS_G
    default:
      return acs_fail(ctx, ACS_E_INVALID, "unsupported group size %d", G);
  }
  return ACS_OK;
}

// The row instance (k_sba_lm's ROW flag) is legal without camera ids for 3 to 8 slots (with 2
// slots and above 8 the broadcast form is no shorter than the butterfly), and chosen for
// latency-bound grids: at one point per 16-lane row, at most one wave per SIMD. There the
// kernel lasts as long as its slowest wave, and the lanes a row leaves empty cost nothing.
// ctx->sba_lm_layout (acs_sba_set_lm_layout) forces either instance where both are legal.
// Never legal for the standard model, which has no ROW (or HOIST) instance.
static bool lm_row_selected(const acs_ctx* ctx, int K, int64_t n_pts, bool camid, int model = ACS_MODEL_FISHEYE) {
  const bool legal = model == ACS_MODEL_FISHEYE && !camid && K >= 3 && K <= 8;
  if (!legal || ctx->sba_lm_layout == ACS_SBA_LM_BUTTERFLY) return false;
  if (ctx->sba_lm_layout == ACS_SBA_LM_ROW) return true;
  return (n_pts * 16 + 63) / 64 <= 4 * (int64_t)ctx->n_cu;
}

static void launch_lm_row(acs_ctx* ctx, const double* cams, int C, int K, const double2* uv, const uint8_t* mask,
                          int64_t n_pts, const double* pts_in, double* pts, SbaParams prm, double* c0, double* c1,
                          int* st) {
  const dim3 grid(acs_grid(n_pts * 16, 64)), block(64);  // the block size the HOIST instances assume
  const size_t lds = sizeof(double) * ACS_CAM_STRIDE * (C + 1);
#define ACS_ROW_LAUNCH(r)                                                                                        \
  hipLaunchKernelGGL((k_sba_lm<16, 1, false, true, r>), grid, block, lds, ctx->stream, uv, mask, n_pts, pts_in, cams, \
                     K, C, pts, (const uint8_t*)nullptr, prm, c0, c1, st ACS_STAMPS_ARG(g_lm_stamps))
  switch ((K + 1) / 2) {
    case 2: ACS_ROW_LAUNCH(2); break;
    case 3: ACS_ROW_LAUNCH(3); break;
    default: ACS_ROW_LAUNCH(4); break;
  }
#undef ACS_ROW_LAUNCH
}

// The S and camera-id instances of one model.
template <int MODEL>
static int launch_lm_s(acs_ctx* ctx, int S, int G, int blocks, int block, const double* dcams, int C, int K,
                       const double2* duv, const uint8_t* dmask, const uint8_t* dcamid, int64_t n_pts,
                       const double* dpts_in, double* dpts, SbaParams prm, double* c0, double* c1, int* st) {
#define ACS_LM_ARGS ctx, G, blocks, block, dcams, C, K, duv, dmask, dcamid, n_pts, dpts_in, dpts, prm, c0, c1, st
  if (dcamid)
    return (S == 1) ? launch_lm_g<1, true, MODEL>(ACS_LM_ARGS)
           : (S == 3) ? launch_lm_g<3, true, MODEL>(ACS_LM_ARGS)
                      : launch_lm_g<4, true, MODEL>(ACS_LM_ARGS);
  return (S == 1) ? launch_lm_g<1, false, MODEL>(ACS_LM_ARGS)
         : (S == 3) ? launch_lm_g<3, false, MODEL>(ACS_LM_ARGS)
                    : launch_lm_g<4, false, MODEL>(ACS_LM_ARGS);
#undef ACS_LM_ARGS
}

// Launch the LM kernel over an (n_pts, K) slot tensor already on the device; initial points
// from dpts_in, solution to dpts (may alias). model: ACS_MODEL_* of the camera records.
static int run_lm(acs_ctx* ctx, int model, const double* dcams, int C, int K, const double2* duv, const uint8_t* dmask,
                  const uint8_t* dcamid, int64_t n_pts, const double* dpts_in, double* dpts,
                  const acs_sba_opts* opts, bool report, double** c0_out,
                  double** c1_out, int** st_out) {
  acs_sba_opts o;
  acs_sba_default_opts(&o);
  if (opts) o = *opts;
  ACS_CHECK(ctx, o.f_scale > 0 && o.max_iters >= 0, "bad acs_sba_opts");
  ACS_CHECK(ctx, K >= 1 && K <= 256, "observations per point (%d) must be in [1, 256]", K);
  ACS_CHECK(ctx, C >= 1 && C <= 255, "n_cams (%d) must be in [1, 255]", C);
  SbaParams prm{o.max_iters, o.f_scale, o.ftol, o.xtol, o.gtol};
  double *c0 = nullptr, *c1 = nullptr;
  int* st = nullptr;
  if (report) {
    c0 = (double*)acs_ws(ctx, WS_PERPT_F0, sizeof(double) * n_pts);
    c1 = (double*)acs_ws(ctx, WS_PERPT_F1, sizeof(double) * n_pts);
    st = (int*)acs_ws(ctx, WS_PERPT_I, sizeof(int) * 3 * n_pts);
    if (!c0 || !c1 || !st) return ACS_E_NOMEM;
  }
  if (lm_row_selected(ctx, K, n_pts, dcamid != nullptr, model)) {
    launch_lm_row(ctx, dcams, C, K, duv, dmask, n_pts, dpts_in, dpts, prm, c0, c1, st);
    ACS_HIP(ctx, hipGetLastError());
    *c0_out = c0;
    *c1_out = c1;
    *st_out = st;
    return ACS_OK;
  }
  int G = next_pow2(K < 2 ? 2 : K);
  int S = 1;
  if (G > 64) {
    G = 64;
    S = 4;
  } else if (G > K && (int64_t)((n_pts * G + 63) / 64) > 16 * (int64_t)ctx->n_cu) {
    // a throughput-bound grid (more than 4 waves per SIMD) whose slot count is not a power of
    // two: three slots per lane in groups of G / 4 lanes wherever that wastes fewer lanes
    // (K = 12: 4 lanes x 3 slots, where 16-lane groups ran 4 lanes per point through the null
    // camera record; the per-point LM arithmetic is also repeated by 4 lanes instead of 16)
    const int g3 = next_pow2((K + 2) / 3);
    if (3 * g3 < G) {
      G = g3 < 2 ? 2 : g3;
      S = 3;
    }
  }
  const int64_t threads = n_pts * G;
  int block = 256;
  if (threads < (int64_t)256 * 2 * ctx->n_cu) block = 64;  // small problem: spread over more CUs
  const int blocks = acs_grid(threads, block);
  const int rc = model == ACS_MODEL_STANDARD
                     ? launch_lm_s<ACS_MODEL_STANDARD>(ctx, S, G, blocks, block, dcams, C, K, duv, dmask, dcamid, n_pts,
                                                       dpts_in, dpts, prm, c0, c1, st)
                     : launch_lm_s<ACS_MODEL_FISHEYE>(ctx, S, G, blocks, block, dcams, C, K, duv, dmask, dcamid, n_pts,
                                                      dpts_in, dpts, prm, c0, c1, st);
  if (rc) return rc;
  ACS_HIP(ctx, hipGetLastError());
  *c0_out = c0;
  *c1_out = c1;
  *st_out = st;
  return ACS_OK;
}

static int run_report(acs_ctx* ctx, const double* c0, const double* c1, const int* st, int64_t n,
                      acs_report* report) {
  acs_report* drep = (acs_report*)acs_ws(ctx, WS_REPORT, sizeof(acs_report));
  if (!drep) return ACS_E_NOMEM;
  hipLaunchKernelGGL(k_sba_report, dim3(1), dim3(256), 0, ctx->stream, c0, c1, st, n, drep);
  ACS_HIP(ctx, hipGetLastError());
  ACS_HIP(ctx, hipMemcpyAsync(report, drep, sizeof(acs_report), hipMemcpyDeviceToHost, ctx->stream));
  ACS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ACS_OK;
}

int acs_sba_dense_enqueue(acs_ctx* ctx, const double* dcams, int C, const double2* duv, const uint8_t* dmask,
                          int64_t n_pts, const double* dpts_in, double* dpts_out, const acs_sba_opts* opts,
                          acs_report* report, int model) {
  if (n_pts == 0) {
    if (report) std::memset(report, 0, sizeof(*report));
    return ACS_OK;
  }
  double *c0, *c1;
  int* st;
  int rc;
  if ((rc = run_lm(ctx, model, dcams, C, C, duv, dmask, nullptr, n_pts, dpts_in, dpts_out, opts, report != nullptr, &c0, &c1,
                   &st)))
    return rc;
  if (report) return run_report(ctx, c0, c1, st, n_pts, report);
  return ACS_OK;
}

// Observation list -> slot tensor (ObsSlots, common.hpp); the messages name the entry point fn
static int obs_to_slots(acs_ctx* ctx, const char* fn, int max_K, int64_t n_obs, int64_t n_pts, int n_cams,
                        ObsSlots* o) {
  hipStream_t s = ctx->stream;
  // stable sort of observation ids by point id
  int32_t* skey = (int32_t*)acs_ws(ctx, WS_SORT0, sizeof(int32_t) * n_obs);
  int32_t* vin = (int32_t*)acs_ws(ctx, WS_SORT1, sizeof(int32_t) * n_obs);
  int32_t* sval = (int32_t*)acs_ws(ctx, WS_SORT2, sizeof(int32_t) * n_obs);
  int32_t* cnt = (int32_t*)acs_ws(ctx, WS_TMP0, sizeof(int32_t) * (n_pts + 2));
  int32_t* start = (int32_t*)acs_ws(ctx, WS_TMP1, sizeof(int32_t) * (n_pts + 1));
  if (!skey || !vin || !sval || !cnt || !start) return ACS_E_NOMEM;
  hipLaunchKernelGGL(k_iota, dim3(acs_grid(n_obs, 256)), dim3(256), 0, s, vin, n_obs);
  size_t tb0 = 0, tb1 = 0, tb2 = 0;
  ACS_HIP(ctx, hipcub::DeviceRadixSort::SortPairs(nullptr, tb0, o->pt_idx, skey, (const int32_t*)vin, sval,
                                                   (int)n_obs, 0, 32, s));
  ACS_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, tb1, cnt, start, (int)n_pts, s));
  ACS_HIP(ctx, hipcub::DeviceReduce::Max(nullptr, tb2, cnt, cnt + n_pts, (int)n_pts, s));
  size_t tb = std::max(tb0, std::max(tb1, tb2));
  void* tmp = acs_ws(ctx, WS_SORT3, tb);
  if (!tmp) return ACS_E_NOMEM;
  ACS_HIP(ctx, hipcub::DeviceRadixSort::SortPairs(tmp, tb, o->pt_idx, skey, (const int32_t*)vin, sval,
                                                   (int)n_obs, 0, 32, s));
  ACS_HIP(ctx, hipMemsetAsync(cnt, 0, sizeof(int32_t) * (n_pts + 2), s));
  hipLaunchKernelGGL(k_count, dim3(acs_grid(n_obs, 256)), dim3(256), 0, s, o->pt_idx, n_obs, cnt, n_pts,
                     cnt + n_pts + 1);
  ACS_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(tmp, tb, cnt, start, (int)n_pts, s));
  ACS_HIP(ctx, hipcub::DeviceReduce::Max(tmp, tb, cnt, cnt + n_pts, (int)n_pts, s));
  int32_t hk[2] = {0, 0};
  ACS_HIP(ctx, hipMemcpyAsync(hk, cnt + n_pts, sizeof(int32_t) * 2, hipMemcpyDeviceToHost, s));
  ACS_HIP(ctx, hipStreamSynchronize(s));
  ACS_CHECK(ctx, hk[1] == 0, "%s: %d point indices out of [0, %lld)", fn, hk[1], (long long)n_pts);
  const int K = hk[0] < 1 ? 1 : hk[0];
  ACS_CHECK(ctx, K <= max_K, "%s: a point has %d observations (max %d)", fn, K, max_K);
  o->uvp = (double2*)acs_ws(ctx, WS_TMP2, sizeof(double2) * n_pts * K);
  o->mask = (uint8_t*)acs_ws(ctx, WS_TMP3, (size_t)n_pts * K);
  o->camid = (uint8_t*)acs_ws(ctx, WS_TMP4, (size_t)n_pts * K);
  if (!o->uvp || !o->mask || !o->camid) return ACS_E_NOMEM;
  ACS_HIP(ctx, hipMemsetAsync(o->mask, 0, (size_t)n_pts * K, s));
  hipLaunchKernelGGL(k_scatter_slots, dim3(acs_grid(n_obs, 256)), dim3(256), 0, s, skey, sval, n_obs, start,
                     (const double2*)o->uv, o->cam_idx, K, n_cams, o->uvp, o->mask, o->camid);
  ACS_HIP(ctx, hipGetLastError());
  o->K = K;
  return ACS_OK;
}

int acs_stage_obs(acs_ctx* ctx, const char* fn, int max_K, int cam_stride, const double* cams, int n_cams,
                  const double* uv, const int32_t* pt_idx, const int32_t* cam_idx, int64_t n_obs, const double* pts,
                  int64_t n_pts, uint32_t flags, ObsSlots* o) {
  int rc;
  if ((rc = acs_stage_in(ctx, WS_CAMS, cams, sizeof(double) * cam_stride * n_cams, flags, (void**)&o->cams))) return rc;
  if ((rc = acs_stage_in(ctx, WS_PTS, pts, sizeof(double) * 3 * n_pts, flags, (void**)&o->pts))) return rc;
  if (n_obs == 0) {
    o->uvp = (double2*)acs_ws(ctx, WS_TMP2, sizeof(double2) * n_pts);
    o->mask = (uint8_t*)acs_ws(ctx, WS_TMP3, (size_t)n_pts);
    o->camid = (uint8_t*)acs_ws(ctx, WS_TMP4, (size_t)n_pts);
    if (!o->uvp || !o->mask || !o->camid) return ACS_E_NOMEM;
    ACS_HIP(ctx, hipMemsetAsync(o->mask, 0, (size_t)n_pts, ctx->stream));
    return ACS_OK;
  }
  if ((rc = acs_stage_in(ctx, WS_UV, uv, sizeof(double) * 2 * n_obs, flags, (void**)&o->uv))) return rc;
  if ((rc = acs_stage_in(ctx, WS_PTIDX, pt_idx, sizeof(int32_t) * n_obs, flags, (void**)&o->pt_idx))) return rc;
  if ((rc = acs_stage_in(ctx, WS_CAMIDX, cam_idx, sizeof(int32_t) * n_obs, flags, (void**)&o->cam_idx))) return rc;
  return obs_to_slots(ctx, fn, max_K, n_obs, n_pts, n_cams, o);
}

extern "C" {

int acs_sba_set_lm_layout(acs_ctx* ctx, int32_t layout) {
  if (!ctx) return ACS_E_INVALID;
  ACS_CHECK(ctx, layout == ACS_SBA_LM_AUTO || layout == ACS_SBA_LM_BUTTERFLY || layout == ACS_SBA_LM_ROW,
            "acs_sba_set_lm_layout: layout %d", layout);
  ctx->sba_lm_layout = layout;
  return ACS_OK;
}

int acs_sba_lm_layout(const acs_ctx* ctx, int32_t n_slots, int64_t n_pts, int32_t with_cam_ids, int32_t* n_cu) {
  if (!ctx || n_slots < 1 || n_pts < 0) return -1;
  if (n_cu) *n_cu = ctx->n_cu;
  return lm_row_selected(ctx, n_slots, n_pts, with_cam_ids != 0) ? ACS_SBA_LM_ROW : ACS_SBA_LM_BUTTERFLY;
}

int acs_sba_lm_layout_flags(const acs_ctx* ctx, int32_t n_slots, int64_t n_pts, int32_t with_cam_ids, int32_t* n_cu,
                            uint32_t flags) {
  if (!ctx || n_slots < 1 || n_pts < 0) return -1;
  if (n_cu) *n_cu = ctx->n_cu;
  return lm_row_selected(ctx, n_slots, n_pts, with_cam_ids != 0, acs_flags_model(flags)) ? ACS_SBA_LM_ROW
                                                                                         : ACS_SBA_LM_BUTTERFLY;
}

int acs_sba_points_dense_io(acs_ctx* ctx, const double* cams, int32_t n_cams, const double* uv,
                            const uint8_t* mask, int64_t n_pts, const double* pts_in, double* pts_out,
                            const acs_sba_opts* opts, acs_report* report, uint32_t flags) {
  ACS_DEVICE_GUARD(ctx);
  ACS_CHECK(ctx, n_pts >= 0 && n_cams >= 1 && n_cams <= 64, "acs_sba_points_dense: n_pts=%lld n_cams=%d (1..64)",
            (long long)n_pts, n_cams);
  if (n_pts == 0) {
    if (report) std::memset(report, 0, sizeof(*report));
    return ACS_OK;
  }
  void *dc, *duv, *dm, *dpi;
  int rc;
  const int model = acs_flags_model(flags);
  if ((rc = acs_stage_in(ctx, WS_CAMS, cams, sizeof(double) * acs_cam_stride(model) * n_cams, flags, &dc))) return rc;
  if ((rc = acs_stage_in(ctx, WS_UV, uv, sizeof(double) * 2 * n_pts * n_cams, flags, &duv))) return rc;
  if ((rc = acs_stage_in(ctx, WS_MASK, mask, (size_t)n_pts * n_cams, flags, &dm))) return rc;
  if ((rc = acs_stage_in(ctx, WS_PTS, pts_in, sizeof(double) * 3 * n_pts, flags, &dpi))) return rc;
  double* dpo = (double*)acs_out_buf(ctx, WS_OUT0, pts_out, sizeof(double) * 3 * n_pts, flags);
  if (!dpo) return ACS_E_NOMEM;
  double *c0, *c1;
  int* st;
  if ((rc = run_lm(ctx, model, (const double*)dc, n_cams, n_cams, (const double2*)duv, (const uint8_t*)dm, nullptr, n_pts,
                   (const double*)dpi, dpo, opts, report != nullptr, &c0, &c1, &st)))
    return rc;
  if ((rc = acs_stage_out(ctx, pts_out, dpo, sizeof(double) * 3 * n_pts, flags))) return rc;
  if (report) {
    if ((rc = run_report(ctx, c0, c1, st, n_pts, report))) return rc;
  } else if (!(flags & ACS_DEVICE_PTRS)) {
    ACS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return ACS_OK;
}

int acs_sba_points_dense(acs_ctx* ctx, const double* cams, int32_t n_cams, const double* uv, const uint8_t* mask,
                         int64_t n_pts, double* pts, const acs_sba_opts* opts, acs_report* report, uint32_t flags) {
  ACS_DEVICE_GUARD(ctx);
  return acs_sba_points_dense_io(ctx, cams, n_cams, uv, mask, n_pts, pts, pts, opts, report, flags);
}

int acs_sba_points(acs_ctx* ctx, const double* cams, int32_t n_cams, const double* uv, const int32_t* pt_idx,
                   const int32_t* cam_idx, int64_t n_obs, double* pts, int64_t n_pts, const acs_sba_opts* opts,
                   double* resid_before, double* resid_after, acs_report* report, uint32_t flags) {
  ACS_DEVICE_GUARD(ctx);
  ACS_CHECK(ctx, n_obs >= 0 && n_pts >= 0 && n_cams >= 1 && n_cams <= 255, "acs_sba_points: bad sizes");
  ACS_CHECK(ctx, n_obs < (int64_t)INT32_MAX, "acs_sba_points: n_obs too large");
  if (n_pts == 0 || n_obs == 0) {
    if (report) std::memset(report, 0, sizeof(*report));
    return ACS_OK;
  }
  int rc;
  const int model = acs_flags_model(flags);
  const auto k_res = model == ACS_MODEL_STANDARD ? k_residuals_ext<ACS_MODEL_STANDARD> : k_residuals_ext<ACS_MODEL_FISHEYE>;
  ObsSlots o;
  if ((rc = acs_stage_obs(ctx, "acs_sba_points", 256, acs_cam_stride(model), cams, n_cams, uv, pt_idx, cam_idx, n_obs,
                          pts, n_pts, flags, &o)))
    return rc;
  hipStream_t s = ctx->stream;

  // residuals at the initial points (residuals['before'])
  double* drb = nullptr;
  if (resid_before) {
    drb = (double*)acs_out_buf(ctx, WS_OUT0, resid_before, sizeof(double) * 2 * n_obs, flags);
    if (!drb) return ACS_E_NOMEM;
    hipLaunchKernelGGL(k_res, dim3(acs_grid(n_obs, 256)), dim3(256), 0, s, o.cams, n_cams, o.uv, o.pt_idx, o.cam_idx,
                       n_obs, (const double*)o.pts, n_pts, drb);
    ACS_HIP(ctx, hipGetLastError());
  }

  double *c0, *c1;
  int* st;
  if ((rc = run_lm(ctx, model, o.cams, n_cams, o.K, o.uvp, o.mask, o.camid, n_pts, o.pts, o.pts, opts, report != nullptr,
                   &c0, &c1, &st)))
    return rc;

  double* dra = nullptr;
  if (resid_after) {
    dra = (double*)acs_out_buf(ctx, WS_OUT1, resid_after, sizeof(double) * 2 * n_obs, flags);
    if (!dra) return ACS_E_NOMEM;
    hipLaunchKernelGGL(k_res, dim3(acs_grid(n_obs, 256)), dim3(256), 0, s, o.cams, n_cams, o.uv, o.pt_idx, o.cam_idx,
                       n_obs, (const double*)o.pts, n_pts, dra);
    ACS_HIP(ctx, hipGetLastError());
  }
  if ((rc = acs_stage_out(ctx, pts, o.pts, sizeof(double) * 3 * n_pts, flags))) return rc;
  if (resid_before && (rc = acs_stage_out(ctx, resid_before, drb, sizeof(double) * 2 * n_obs, flags))) return rc;
  if (resid_after && (rc = acs_stage_out(ctx, resid_after, dra, sizeof(double) * 2 * n_obs, flags))) return rc;
  if (report) {
    if ((rc = run_report(ctx, c0, c1, st, n_pts, report))) return rc;
  } else if (!(flags & ACS_DEVICE_PTRS)) {
    ACS_HIP(ctx, hipStreamSynchronize(s));
  }
  return ACS_OK;
}

}  // extern "C"
