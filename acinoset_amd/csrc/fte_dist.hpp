// fte_dist.hpp — frame-window distributed FTE solve: its kernels, the handle, the three phase
// bodies and the acs_fte_dist_* entry points. Included by fte.hip after fte_host.hpp.
#pragma once

// =======================================================================================
// frame-window distributed solve (spec: oracle/fte_dist.py)
//
// Super-blocks are split into R chains [a_r, a_r + 2^k] that share their end blocks
// (a_r = r 2^k; blocks past the sequence are phantoms). A term is owned by the chain
// containing its lowest row, so every term is counted on exactly one rank and the
// chain-end blocks hold partial sums. Per LM iteration:
//   phase 1  linearise owned frames, assemble chain rows, block cyclic reduction of the
//            chain interior down to its two ends (ends undamped), pack the ends' blocks,
//            raw diagonals / gradients, tau partial sums and an interior |g| max into
//            payload 1 (zeros elsewhere)                                 -> all-reduce
//   phase 2  every rank: reduced block-tridiagonal system over the R+1 chain ends + tau
//            (damped with the summed raw diagonals), solved with the same CR kernels;
//            back substitution down its own chain; its rows of delta into payload 2
//                                                                        -> all-reduce
//   phase 3  trial state on every rank (replicated X), cost of the owned terms
//                                                        -> all-reduce (2 doubles)
//   phase 4  the same accept/reject decision on every rank
// =======================================================================================
struct DistLayout {
  size_t oD, oE, oG, oGraw, oRdiag, oTau, oGmax, n1, n2, n3;
};

static DistLayout dist_layout(const FteDims& d, int R) {
  DistLayout L;
  const size_t nb = R + 1, BP = d.BP, GR = d.GR, nE = (size_t)d.Cg * d.Cg + d.Cg + (size_t)GR * GR;
  L.oD = 0;
  L.oE = L.oD + nb * BP * BP;
  L.oG = L.oE + nb * BP * BP;
  L.oGraw = L.oG + nb * BP * GR;
  L.oRdiag = L.oGraw + nb * BP;
  L.oTau = L.oRdiag + nb * BP;
  L.oGmax = L.oTau + nE;
  L.n1 = L.oGmax + R;
  L.n2 = (size_t)d.nblk * BP + (d.var ? (size_t)d.NT : 0);  // solution rows (+ per-frame delays)
  L.n3 = 4;
  return L;
}

// chain ends -> payload slots `rank` (left end a0) and `rank + 1` (right end bend)
__global__ __launch_bounds__(256) void k_dist_pack(FteDims d, const FteState* __restrict__ st, DistLayout Lo,
                                                   int rank, int a0, int bend, const double* __restrict__ Dc,
                                                   const double* __restrict__ Ec, const double* __restrict__ GBc,
                                                   const double* __restrict__ rdiag, const double* __restrict__ gb,
                                                   double* __restrict__ p1) {
  if (st->status != 0) return;
  const int side = blockIdx.y;  // 0 left end, 1 right end
  const int blk = side ? bend : a0, q = rank + side;
  if (blk >= d.nblk) return;
  const int BP = d.BP, GR = d.GR, P = d.P;
  const size_t nBB = (size_t)BP * BP;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < nBB; e += (size_t)gridDim.x * blockDim.x) {
    p1[Lo.oD + q * nBB + e] = Dc[(size_t)blk * nBB + e];
    if (side) p1[Lo.oE + q * nBB + e] = Ec[(size_t)blk * nBB + e];
  }
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < (size_t)BP * GR;
       e += (size_t)gridDim.x * blockDim.x)
    p1[Lo.oG + (size_t)q * BP * GR + e] = GBc[(size_t)blk * BP * GR + e];
  if (blockIdx.x == 0) {
    for (int r = threadIdx.x; r < BP; r += blockDim.x) {
      const int fr = 3 * blk + r / P, pr = r % P;
      const bool in = r < 3 * P && fr < d.M;
      p1[Lo.oGraw + (size_t)q * BP + r] = in ? gb[(size_t)fr * P + pr] : 0.0;
      p1[Lo.oRdiag + (size_t)q * BP + r] = in ? rdiag[(size_t)fr * P + pr] : 0.0;
    }
  }
}

// tau partial sums of the chain (fixed chunk order) and the |g| max of its interior rows
__global__ __launch_bounds__(256) void k_dist_pack_small(FteDims d, const FteState* __restrict__ st, DistLayout Lo,
                                                         int rank, int a0, int bend,
                                                         const double* __restrict__ part,
                                                         const double* __restrict__ gmaxp,
                                                         double* __restrict__ p1,
                                                         const double* __restrict__ gmaxt = nullptr) {
  if (st->status != 0) return;
  __shared__ double s_red[256];
  const int nE = d.Cg * d.Cg + d.Cg + d.GR * d.GR;
  for (int e = threadIdx.x; e < nE; e += blockDim.x) {
    double v = 0.0;
    for (int ch = 0; ch < CR_NCHUNK; ++ch) v += part[(size_t)ch * nE + e];
    p1[Lo.oTau + e] = v;
  }
  const int f0 = 3 * (a0 + 1), f1 = min(3 * min(bend, d.nblk), d.M);
  double mx = 0.0;
  mx = strided_max(gmaxp, f0 + (int)threadIdx.x, f1, blockDim.x, mx);
  // per-frame delays: every owned frame's (rows of the whole chain; other frames give 0)
  if (gmaxt) mx = strided_max(gmaxt, 3 * a0 + (int)threadIdx.x, min(3 * min(bend, d.nblk - 1) + 3, d.M), blockDim.x, mx);
  mx = block_max(mx, s_red);
  if (threadIdx.x == 0) p1[Lo.oGmax + rank] = mx;
}

// reduced system over the chain ends e_q = q 2^k (q = 0..R) from the summed payload
__global__ __launch_bounds__(256) void k_red_build(FteDims d, const FteState* __restrict__ st, DistLayout Lo, int R,
                                                   int span, const double* __restrict__ p1, double* __restrict__ Dr,
                                                   double* __restrict__ Er, double* __restrict__ GBr,
                                                   double* __restrict__ gmaxr) {
  if (st->status != 0) return;
  __shared__ double s_red[256];
  const int q = blockIdx.x, e = q * span;
  const int BP = d.BP, GR = d.GR, P = d.P;
  const size_t nBB = (size_t)BP * BP;
  const double lam = st->lam;
  // rows of block x that are real unknowns (not padding / phantom)
  auto live = [&](int x, int r) { return x >= 0 && x < d.nblk && r < 3 * P && 3 * x + r / P < d.M; };
  for (size_t x = threadIdx.x; x < nBB; x += blockDim.x) {
    const int r = (int)(x / BP), c = (int)(x % BP);
    double v = (r == c) ? 1.0 : 0.0;
    if (live(e, r) && live(e, c)) {
      v = p1[Lo.oD + q * nBB + x];
      if (r == c) v += lam * fmax(p1[Lo.oRdiag + (size_t)q * BP + r], 1e-12);
    }
    Dr[q * nBB + x] = v;
    Er[q * nBB + x] = (q > 0 && live(e, r) && live(e - span, c)) ? p1[Lo.oE + q * nBB + x] : 0.0;
  }
  for (size_t x = threadIdx.x; x < (size_t)BP * GR; x += blockDim.x) {
    const int r = (int)(x / GR);
    GBr[(size_t)q * BP * GR + x] = live(e, r) ? p1[Lo.oG + (size_t)q * BP * GR + x] : 0.0;
  }
  if (q == 0) {
    double mx = 0.0;
    for (int t = threadIdx.x; t < R; t += blockDim.x) mx = fmax(mx, p1[Lo.oGmax + t]);
    for (int t = threadIdx.x; t < (R + 1) * BP; t += blockDim.x) {
      const int qq = t / BP, r = t % BP, ee = qq * span;
      if (ee < d.nblk && r < 3 * P && 3 * ee + r / P < d.M) mx = fmax(mx, fabs(p1[Lo.oGraw + t]));
    }
    mx = block_max(mx, s_red);
    if (threadIdx.x == 0) gmaxr[0] = mx;
  }
}

__global__ void k_red_part(int nE, const DistLayout Lo, const FteState* __restrict__ st,
                           const double* __restrict__ p1, double* __restrict__ partr) {
  if (st->status != 0) return;
  for (int e = threadIdx.x; e < nE; e += blockDim.x) partr[e] += p1[Lo.oTau + e];
}

__global__ void k_dist_scatter(FteDims d, const FteState* __restrict__ st, int rank, int a0, int bend,
                               const double* __restrict__ dcvr, double* __restrict__ dcv) {
  if (st->status != 0) return;
  for (int r = threadIdx.x; r < d.BP; r += blockDim.x) {
    if (a0 < d.nblk) dcv[(size_t)a0 * d.BP + r] = dcvr[(size_t)rank * d.BP + r];
    if (bend < d.nblk) dcv[(size_t)bend * d.BP + r] = dcvr[(size_t)(rank + 1) * d.BP + r];
  }
}

// p3 = (measurement cost, model cost, |step|^2, |X, tau|^2) of this rank's owned terms /
// rows (frames [k0, k1), super-blocks [n0, n1) of the trial's norm partials)
// which = 1: the trial's measurement terms are in Fm's speculative copy (cur ^ 1, N each)
__global__ __launch_bounds__(256) void k_dist_cost_pack(FteState* __restrict__ st, int which, int N, int m0,
                                                        int m1, int q0, int q1, const double* __restrict__ Fm,
                                                        const double* __restrict__ Fq, int n0, int n1,
                                                        const double* __restrict__ normp, double* __restrict__ p3,
                                                        int t0 = 0, int t1 = 0,
                                                        const double* __restrict__ normt = nullptr) {
  if (which == 1 && st->status != 0) return;
  if (which == 1) Fm += (size_t)(st->cur ^ 1) * N;
  __shared__ double s_red[256];
  double a = 0.0, b = 0.0, nrm[2] = {0.0, 0.0};
  {
    const double* xs[1] = {Fm};
    strided_sums<1>(xs, 1, m0 + (int)threadIdx.x, m1, blockDim.x, &a);
  }
  {
    const double* xs[1] = {Fq};
    strided_sums<1>(xs, 1, q0 + (int)threadIdx.x, q1, blockDim.x, &b);
  }
  if (n1 > n0) {
    const double* xs[2] = {normp, normp + 1};
    strided_sums<2>(xs, 2, n0 + (int)threadIdx.x, n1, blockDim.x, nrm);
  }
  if (normt && t1 > t0) {  // per-frame delays of the owned frames, over every block of the chain
    const double* xs[2] = {normt, normt + 1};
    strided_sums<2>(xs, 2, t0 + (int)threadIdx.x, t1, blockDim.x, nrm);
  }
  double dn = nrm[0], xn = nrm[1];
  a = block_sum(a, s_red);
  b = block_sum(b, s_red);
  dn = block_sum(dn, s_red);
  xn = block_sum(xn, s_red);
  if (threadIdx.x == 0) {
    p3[0] = a;
    p3[1] = b;
    p3[2] = dn;
    p3[3] = xn;
    if (which == 1) st->pending = 1;  // this round took a step: its cost travels in p3
  }
}

// X[cur] rows of super-blocks [b_lo, b_hi) in the block layout of the step (BP per block);
// per-frame delays: those of the owned frames [k_lo, k_hi) after the rows
__global__ __launch_bounds__(256) void k_dist_x_out(FteDims d, const FteState* __restrict__ st, int b_lo, int b_hi,
                                                    const double* __restrict__ Xbuf, double* __restrict__ p2,
                                                    const double* __restrict__ taubuf, int k_lo, int k_hi) {
  const double* X = Xbuf + (size_t)st->cur * d.M * d.P;
  const int P = d.P, BP = d.BP;
  for (size_t e = (size_t)b_lo * BP + (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < (size_t)b_hi * BP;
       e += (size_t)gridDim.x * blockDim.x) {
    const int i = (int)(e / BP), r = (int)(e % BP), f = 3 * i + r / P;
    if (r < 3 * P && f < d.M) p2[e] = X[(size_t)f * P + r % P];
  }
  if (d.var) {
    const double* tau = taubuf + (size_t)st->cur * d.NT;
    for (size_t e = (size_t)k_lo * d.C + (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < (size_t)k_hi * d.C;
         e += (size_t)gridDim.x * blockDim.x)
      p2[(size_t)d.nblk * BP + e] = tau[e];
  }
}

// every row of X[cur] (and every per-frame delay) from the gathered layout
__global__ __launch_bounds__(256) void k_dist_x_in(FteDims d, const FteState* __restrict__ st,
                                                   const double* __restrict__ p2, double* __restrict__ Xbuf,
                                                   double* __restrict__ taubuf) {
  double* X = Xbuf + (size_t)st->cur * d.M * d.P;
  const int P = d.P, BP = d.BP;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < (size_t)d.nblk * BP;
       e += (size_t)gridDim.x * blockDim.x) {
    const int i = (int)(e / BP), r = (int)(e % BP), f = 3 * i + r / P;
    if (r < 3 * P && f < d.M) X[(size_t)f * P + r % P] = p2[e];
  }
  if (d.var) {
    double* tau = taubuf + (size_t)st->cur * d.NT;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < (size_t)d.NT; e += (size_t)gridDim.x * blockDim.x)
      tau[e] = p2[(size_t)d.nblk * BP + e];
  }
}

// Round control (one thread). On the summed payload of the previous round: the first round
// takes the initial cost; otherwise a pending step is accepted or rejected (oracle/fte.py
// solve; every rank takes the same decision). A rejection marks the round SKIP: its solve
// is stale (formed for the trial state) and the round only re-forms the reduced system.
__global__ void k_dist_decide(FteState* __restrict__ st, FteOptsDev o, const double* __restrict__ p3) {
  if (threadIdx.x != 0) return;
  const double fm = p3[0], fq = p3[1];
  if (st->first) {
    st->first = 0;
    st->F = st->F0 = fm + fq;
    st->Fmeas = fm;
    st->Fmodel = fq;
    // max_iters = 0: no step at all, as acs_fte_solve (X0 back, iters 0)
    if (o.max_iters <= 0) st->status = ACS_STATUS_MAXITER;
    return;
  }
  if (st->status != 0 || !st->pending) return;
  st->pending = 0;
  const double Fn = fm + fq, dn = p3[2], xn = p3[3];  // step / state norms summed over the owned rows
  st->iters += 1;
  st->dnorm = sqrt(dn);
  st->xnorm = sqrt(xn);
  const bool small = sqrt(dn) <= o.xtol * (o.xtol + sqrt(xn));
  if (Fn < st->F) {
    const bool fconv = (st->F - Fn) <= o.ftol * fabs(st->F);
    st->nacc += 1;
    st->F = Fn;
    st->Fmeas = fm;
    st->Fmodel = fq;
    st->cur ^= 1;
    st->lam = fmax(st->lam * 0.1, 1e-15);
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
  if (st->status == 0 && !st->relin) st->status = FTE_STATUS_SKIP;
}

// after the reduced solve of a live round: the gradient test on the summed gradient
__global__ void k_dist_gtol(FteState* __restrict__ st, FteOptsDev o) {
  if (threadIdx.x == 0 && st->status == 0 && st->gmax <= o.gtol) st->status = ACS_STATUS_GTOL;
}

// before / after the round's reduced system: a round that took a step forms it at the trial
// state (copy cur ^ 1, linearised there for the trial cost) with the damping an acceptance
// sets; the LM state is swapped for those kernels and restored after them
__global__ void k_dist_spec(FteState* __restrict__ st, int enter) {
  if (threadIdx.x != 0) return;
  if (enter) {
    if (st->status == FTE_STATUS_SKIP) st->status = 0;
    if (st->status == 0 && st->pending) {
      st->spec_on = 1;
      st->save_cur = st->cur;
      st->save_lam = st->lam;
      st->cur ^= 1;
      st->lam = fmax(st->lam * 0.1, 1e-15);
    }
  } else if (st->spec_on) {
    st->spec_on = 0;
    st->cur = st->save_cur;
    st->lam = st->save_lam;
  }
}

struct acs_fte_dist {
  acs_ctx* ctx;
  FteSetup S;
  void* own = nullptr;
  void* own_red = nullptr;
  FteDims dr;        // reduced system dims (R + 1 blocks)
  FteBuffers r;      // reduced arrays (Dc, Ec, GBc, Wc, Tau, dcv, part, gmaxp)
  DistLayout Lo;
  FteOptsDev o;
  int R, rank, span, a0, bend, klev;
  double lam0;  // the LM's initial damping (acs_fte_dist_reset restarts from it)
  int k_lo, k_hi, f_lo, f_hi, b_hi_build, c_lo, c_hi, own_lo, own_hi, out_lo, out_hi;
  // rounds captured as hipGraphs (one graph launch instead of ~60 kernel launches); key =
  // (input payload, output payload, stream): two graphs for the two payload buffers
  struct Captured {
    hipGraphExec_t exec = nullptr;
    const void* ptr = nullptr;
    const void* ptr2 = nullptr;
    hipStream_t stream = nullptr;
  } g[2];
  // status after each round: pinned ring of ACS_DIST_RING slots with completion events
  int32_t* snap = nullptr;
  hipEvent_t snap_ev[4] = {};
  int64_t rounds = 0;
};
#define ACS_DIST_RING 4

// Run `enqueue` (kernel launches on ctx->stream) through the phase's cached graph,
// capturing it when the key changed; plain launches if capture is unavailable.
template <typename F>
static int dist_run_captured(acs_fte_dist* h, const void* ptr, const void* ptr2, F enqueue) {
  acs_ctx* ctx = h->ctx;
  hipStream_t s = ctx->stream;
  int which = 0;
  for (; which < 2; ++which)
    if (h->g[which].exec && h->g[which].ptr == ptr && h->g[which].ptr2 == ptr2 && h->g[which].stream == s) break;
  if (which == 2) which = (h->g[0].exec && !h->g[1].exec) ? 1 : 0;
  auto& c = h->g[which];
  if (!c.exec || c.ptr != ptr || c.ptr2 != ptr2 || c.stream != s) {
    if (c.exec) (void)hipGraphExecDestroy(c.exec);
    c.exec = nullptr;
    hipGraph_t graph = nullptr;
    if (hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed) == hipSuccess) {
      const int rc = enqueue();
      const hipError_t e = hipStreamEndCapture(s, &graph);
      if (rc) {
        if (graph) (void)hipGraphDestroy(graph);
        return rc;
      }
      if (e == hipSuccess && graph && hipGraphInstantiate(&c.exec, graph, nullptr, nullptr, 0) == hipSuccess) {
        c.ptr = ptr;
        c.ptr2 = ptr2;
        c.stream = s;
      } else {
        c.exec = nullptr;
      }
      if (graph) (void)hipGraphDestroy(graph);
    }
    if (!c.exec) {
      (void)hipGetLastError();
      return enqueue();
    }
  }
  ACS_HIP(ctx, hipGraphLaunch(c.exec, s));
  return ACS_OK;
}

static const double* dist_local_cr(acs_fte_dist* h) {
  const FteDims& d = h->S.d;
  FteBuffers& b = h->S.b;
  const int top = std::min(h->bend, d.nblk - 1);  // last existing block of the chain
  return cr_reduce(d, h->ctx->stream, b, h->a0, std::min(h->bend, d.nblk), top, h->klev);
}

static int dist_phase1_body(acs_fte_dist* h, double* p1) {
  ACS_DEVICE_GUARD(h ? h->ctx : nullptr);
  acs_ctx* ctx = h->ctx;
  const FteDims& d = h->S.d;
  FteBuffers& b = h->S.b;
  hipStream_t s = ctx->stream;
  ACS_HIP(ctx, hipMemsetAsync(p1, 0, sizeof(double) * h->Lo.n1, s));
  if (h->a0 < d.nblk) {
    // the linearisation of X[cur] is there already (init, or the speculative one of phase 3)
    // the chain's rows assembled in LDS and its super-blocks built in one pass (the banded
    // rows never reach HBM), as the single-GPU solve; the ends' raw diagonals / gradients
    // go to Adiag / gb (row layout) for the payload
    const int top = std::min(h->bend, d.nblk - 1);
    CrChain ch;
    ch.b0 = h->a0;
    ch.nblk = top - h->a0 + 1;
    ch.lo = h->own_lo;
    ch.hi = h->own_hi;
    ch.end_l = h->a0;
    ch.end_r = h->bend;
    ch.rdiag = b.Adiag;
    ch.graw = b.graw;
    if (d.var) {
      // per-frame delays: eliminated per frame in the row assembly (damped with the LM
      // lambda), the rows' gradients before that kept for the payload, then the build
      hipLaunchKernelGGL(k_fte_assemble, dim3(h->f_hi - h->f_lo), dim3(256), 0, s, d, b.X, b.tau, b.qinv, b.st, 0,
                         h->f_lo, h->own_lo, h->own_hi, b.Hloc, b.gloc, b.Ab, b.gb, b.Bt, b.gmaxp, b.Adiag, 1, b.graw,
                         b.gmaxt);
      cr_launch_build(d, s, b, ch);
    } else {
      cr_launch_assemble_build(d, h->S.n_cu, s, b, 0, ch);
    }
    const double* Efin = dist_local_cr(h);
    hipLaunchKernelGGL(k_cr_tau_partial, dim3(CR_NCHUNK), dim3(512), 0, s, d, b.st, b.Hloc, b.gloc, b.Tau, b.part,
                       h->k_lo, h->k_hi, h->a0 + 1, std::min(h->bend, d.nblk), 1,
                       (const double*)b.Tc);
    hipLaunchKernelGGL(k_dist_pack, dim3(32, 2), dim3(256), 0, s, d, b.st, h->Lo, h->rank, h->a0, h->bend, b.Dc, Efin,
                       b.GBc, b.Adiag, b.graw, p1);
    hipLaunchKernelGGL(k_dist_pack_small, dim3(1), dim3(256), 0, s, d, b.st, h->Lo, h->rank, h->a0, h->bend, b.part,
                       b.gmaxp, p1, d.var ? (const double*)b.gmaxt : (const double*)nullptr);
  }
  ACS_HIP(ctx, hipGetLastError());
  return ACS_OK;
}

// ACS_DIST_BACK_LEVELS=1: the rank chain's back substitution as one k_cr_back launch per level
// plus k_cr_trial (the round-5 form, kept for A/B timing); default: k_cr_back_chain
static bool dist_back_levels() {
  static const bool v = acs_env_int("ACS_DIST_BACK_LEVELS", 0) == 1;
  return v;
}

static int dist_phase2_body(acs_fte_dist* h, const double* p1) {
  ACS_DEVICE_GUARD(h ? h->ctx : nullptr);
  acs_ctx* ctx = h->ctx;
  const FteDims& d = h->S.d;
  const FteDims& dr = h->dr;
  FteBuffers& b = h->S.b;
  FteBuffers& r = h->r;
  hipStream_t s = ctx->stream;
  // reduced system (identical on every rank)
  hipLaunchKernelGGL(k_red_build, dim3(dr.nblk), dim3(256), 0, s, d, b.st, h->Lo, h->R, h->span, p1, r.Dc, r.Ec,
                     r.GBc, r.gmaxp);
  const int rb = dr.nblk - 1;
  CrPending pend;
  CrReduceOpts ro;
  ro.final_apply = false;  // the top block applies what is pending
  ro.e_upper = false;      // built by k_red_build, not by the chain builds whose E are upper triangular
  ro.pend_out = &pend;
  cr_reduce(dr, s, r, 0, dr.nblk, rb, dr.nlev, ro);
  cr_launch_top(dr, s, dr.nlev, 0, dr.nblk, r, pend);
  hipLaunchKernelGGL(k_cr_tau_partial, dim3(CR_NCHUNK), dim3(512), 0, s, dr, b.st, r.Hloc, r.gloc, r.Tau, r.part, 0,
                     0, 0, dr.nblk, 0, (const double*)nullptr);
  const int nE = d.Cg * d.Cg + d.Cg + d.GR * d.GR;
  hipLaunchKernelGGL(k_red_part, dim3(1), dim3(256), 0, s, nE, h->Lo, b.st, p1, r.part);
  hipLaunchKernelGGL(k_cr_top, dim3(1), dim3(1024), 0, s, dr, b.st, (const double*)r.Wc, r.part, r.gmaxp, b.tau, r.dcv,
                     b.dtau, b.bad);
  hipLaunchKernelGGL(k_dist_gtol, dim3(1), dim3(64), 0, s, b.st, h->o);
  for (int lv = dr.nlev - 1; lv >= 0; --lv) {
    const int st = 1 << lv;
    const int ne = (dr.nblk - st + 2 * st - 1) / (2 * st);
    hipLaunchKernelGGL(k_cr_back, dim3(ne), dim3(1024), 0, s, dr, st, 0, rb, b.st, r.Wc, b.dtau, r.dcv);
  }
  // this chain: ends from the reduced solve, interior by back substitution, then the trial
  // rows of the whole chain (its end blocks are shared: both neighbours step them alike) and
  // the replicated delays; the norm partials of the owned blocks go to phase 3's payload
  if (h->a0 < d.nblk && !d.var && !dist_back_levels()) {
    hipLaunchKernelGGL(k_dist_scatter, dim3(1), dim3(128), 0, s, d, b.st, h->rank, h->a0, h->bend, r.dcv, b.dcv);
    // the chain's back substitution and trial rows in one launch (k_cr_back_chain)
    const int iend = std::min(h->bend, d.nblk);
    int nint = 0;
    for (int lv = h->klev - 1; lv >= 0; --lv) {
      const int sv = 1 << lv;
      nint += std::max(0, (iend - h->a0 - sv + 2 * sv - 1) / (2 * sv));
    }
    const int nwork = (h->bend < d.nblk ? 2 : 1) + nint;
    const int nth_back = (8 * d.BP + 63) / 64 * 64;
    const CrBackChainKernel kb = cr_back_chain_kernel(d);
    hipLaunchKernelGGL(kb, dim3(nwork), dim3(nth_back), 0, s, d, h->a0, h->bend, h->klev, h->rank == 0 ? 1 : 0,
                       (const FteState*)b.st, (const double*)b.Wc, (const double*)b.dtau, b.dcv, b.bk, b.gdcv, b.bad,
                       b.X, b.tau, b.normp);
  } else if (h->a0 < d.nblk) {
    hipLaunchKernelGGL(k_dist_scatter, dim3(1), dim3(128), 0, s, d, b.st, h->rank, h->a0, h->bend, r.dcv, b.dcv);
    for (int lv = h->klev - 1; lv >= 0; --lv) {
      const int st = 1 << lv;
      int ne = 0;
      for (int i = h->a0 + st; i < std::min(h->bend, d.nblk); i += 2 * st) ++ne;
      if (ne)
        hipLaunchKernelGGL(k_cr_back, dim3(ne), dim3(1024), 0, s, d, st, h->a0, h->bend, b.st, b.Wc, b.dtau, b.dcv);
    }
    const int top = std::min(h->bend, d.nblk - 1);
    hipLaunchKernelGGL(k_cr_trial, dim3(top - h->a0 + 1), dim3(256), 0, s, d, b.st, (const double*)b.dcv, b.dtau,
                       b.Hloc, b.gloc, b.X, b.tau, b.normp, 1, h->a0, h->rank == 0 ? 1 : 0, h->k_lo, h->k_hi,
                       b.normt);
  } else {
    // a rank past the last block still steps the replicated delays
    hipLaunchKernelGGL(k_cr_trial, dim3(1), dim3(256), 0, s, d, b.st, (const double*)b.dcv, b.dtau, b.Hloc, b.gloc,
                       b.X, b.tau, b.normp, 0, d.nblk, h->rank == 0 ? 1 : 0);
  }
  ACS_HIP(ctx, hipGetLastError());
  return ACS_OK;
}

static int dist_phase3_body(acs_fte_dist* h, double* p3) {
  ACS_DEVICE_GUARD(h ? h->ctx : nullptr);
  acs_ctx* ctx = h->ctx;
  const FteDims& d = h->S.d;
  FteBuffers& b = h->S.b;
  hipStream_t s = ctx->stream;
  // speculative linearisation of the trial rows: its measurement terms (owned frames
  // [k_lo, k_hi)) and model stencils (owned: k - 1 in [own_lo, own_hi), so frames up to k_hi
  // inclusive; the one extra frame's own terms are not counted) are the trial cost, and an
  // accepted step needs no new linearisation in phase 1
  const int l_hi = std::min(h->k_hi + 1, d.N);
  if (h->a0 < d.nblk && l_hi > h->k_lo)
    fte_launch_lin(d, s, b, 0, h->k_lo, l_hi - h->k_lo, 1);
  const int q0 = std::max(h->k_lo + 1, 1), q1 = l_hi;
  const int t_hi = std::min(h->bend, d.nblk - 1) + 1;
  hipLaunchKernelGGL(k_dist_cost_pack, dim3(1), dim3(256), 0, s, b.st, 1, d.N, h->k_lo, h->k_hi, q0,
                     std::max(q0, q1), (const double*)b.Floc, (const double*)b.Fq, h->out_lo, h->out_hi, b.normp, p3,
                     d.var ? h->a0 : 0, d.var ? t_hi : 0, (const double*)b.normt);
  ACS_HIP(ctx, hipGetLastError());
  return ACS_OK;
}

// The reduced system's own arrays (dr.nblk = R + 1 blocks) carved out of `base` (null: only the
// size is counted); the rest of r stays the rank's buffers. Returns the bytes taken.
static size_t dist_red_carve(double* base, const FteDims& dr, FteBuffers& r) {
  Arena A{base};
  const size_t nb = dr.nblk, BP = dr.BP, GR = dr.GR;
  r.Dc = A.take(nb * BP * BP);
  r.Ec = A.take(nb * BP * BP);
  r.GBc = A.take(nb * BP * GR);
  r.Wc = A.take(nb * BP * (2 * BP + GR));
  r.Tau = A.take(nb * GR * GR);
  r.dcv = A.take(nb * BP);
  r.Ec2 = A.take(nb * BP * BP);
  r.dL = A.take(nb * BP * (BP + GR));
  r.dR = A.take(nb * BP * (BP + GR));
  r.part = A.take((size_t)CR_NCHUNK * (16 * 16 + 16 + 32 * 32));
  r.gmaxp = A.take(4);
  return A.bytes();
}

// ---------------------------------------------------------------------------------------
// distributed handle API (include/acinoset_hip.h, §8(e)); payloads are device pointers
// ---------------------------------------------------------------------------------------
extern "C" {

int acs_fte_dist_create(acs_ctx* ctx, const int32_t* skel_ints, int64_t n_ints, const double* skel_reals,
                        int64_t n_reals, const double* cams, int32_t n_cams, const double* meas, const double* w,
                        int32_t n_frames, int32_t shutter_delay, double Ts, const double* qinv, int32_t sd_mode,
                        int32_t intermode, const double* X, const double* tau, const acs_fte_opts* opts, int32_t rank,
                        int32_t world, acs_fte_dist** out, int64_t* payload_sizes, uint32_t flags) {
  ACS_DEVICE_GUARD(ctx);
  ACS_FISHEYE_ONLY(ctx, flags, "acs_fte_dist_create");
  acs_fte_opts op;
  acs_fte_default_opts(&op);
  if (opts) op = *opts;
  ACS_CHECK(ctx, op.max_iters >= 0, "fte: max_iters < 0");
  ACS_CHECK(ctx, world >= 1 && world <= 1024 && rank >= 0 && rank < world, "fte_dist: rank %d / world %d", rank,
            world);
  acs_fte_dist* h = new acs_fte_dist();
  h->ctx = ctx;
  const FteProblem pb{skel_ints, n_ints, skel_reals, n_reals, cams, n_cams, meas, w, n_frames, shutter_delay, Ts, qinv,
                      sd_mode, intermode, X, tau, flags, op.redesc_a, op.redesc_b, op.redesc_c};
  int rc = fte_setup(ctx, h->S, pb, &h->own);
  if (rc) {
    if (h->own) (void)acs_dev_free(h->own);
    delete h;
    return rc;
  }
  const FteDims& d = h->S.d;
  h->R = world;
  h->rank = rank;
  h->lam0 = op.lambda0;
  h->o = FteOptsDev{op.max_iters, op.ftol, op.xtol, op.gtol};
  // chain length 2^k: smallest k >= 1 with R 2^k >= nblk - 1
  h->klev = 1;
  while ((int64_t)world * (1 << h->klev) < d.nblk - 1) h->klev++;
  h->span = 1 << h->klev;
  h->a0 = rank * h->span;
  h->bend = h->a0 + h->span;
  const int N = d.N, M = d.M;
  auto clampi = [](int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); };
  h->own_lo = 3 * h->a0;                    // owned terms: lowest row in [own_lo, own_hi)
  h->own_hi = rank == world - 1 ? INT_MAX / 2 : 3 * h->bend;  // the last rank owns the tail
  h->k_lo = clampi(h->own_lo, 0, N);        // frames to linearise
  h->k_hi = clampi(h->own_hi, 0, N);
  h->f_lo = clampi(3 * h->a0, 0, M);        // rows to assemble (chain incl. its right end)
  h->f_hi = clampi(3 * h->bend + 3, 0, M);
  h->c_lo = clampi(h->own_lo, 0, N);        // cost blocks: frames [lo, hi) and stencils up to hi
  h->c_hi = clampi(h->own_hi + 1, 0, N);
  h->out_lo = clampi(h->a0, 0, d.nblk);     // step rows this rank publishes
  h->out_hi = clampi(rank == world - 1 ? h->bend + 1 : h->bend, 0, d.nblk);
  h->Lo = dist_layout(d, world);
  // reduced system arrays
  FteDims& dr = h->dr;
  dr = d;
  dr.nblk = world + 1;
  dr.M = 1;
  dr.N = 0;
  dr.nlev = 0;
  for (int s = 1; s < dr.nblk; s <<= 1) dr.nlev++;
  h->r = h->S.b;
  void* p = nullptr;
  if (acs_dev_malloc(&p, dist_red_carve(nullptr, dr, h->r)) != hipSuccess) {
    (void)acs_dev_free(h->own);
    delete h;
    return acs_fail(ctx, ACS_E_NOMEM, "fte_dist: reduced-system allocation failed");
  }
  h->own_red = p;
  dist_red_carve((double*)p, dr, h->r);
  if ((rc = fte_upload_state(ctx, h->S, op.lambda0, 1))) return rc;
  ACS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  bool snap_ok = acs_host_malloc((void**)&h->snap, sizeof(int32_t) * ACS_DIST_RING, hipHostMallocDefault) == hipSuccess;
  for (auto& e : h->snap_ev)
    if (snap_ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
      e = nullptr;
      snap_ok = false;
    }
  if (!snap_ok) {
    acs_fte_dist_destroy(h);
    return acs_fail(ctx, ACS_E_HIP, "fte_dist: pinned status ring allocation failed");
  }
  if (payload_sizes) {
    payload_sizes[0] = (int64_t)(h->Lo.n1 + h->Lo.n3);
    payload_sizes[1] = (int64_t)h->Lo.n2;
    payload_sizes[2] = (int64_t)h->Lo.n3;
  }
  *out = h;
  return ACS_OK;
}

// A solve restarted on the same handle: X / tau from the caller (host or, with
// ACS_DEVICE_PTRS, device pointers; tau NULL = zeros), the LM state of acs_fte_dist_create
// (first round pending, lambda0), the back-substitution tickets and granules zeroed. The
// arena, the reduced-system arrays, the status ring and the captured round graphs are kept:
// no allocation, so a timed multi-GPU solve can reuse one handle per rank.
int acs_fte_dist_reset(acs_fte_dist* h, const double* X, const double* tau, uint32_t flags) {
  ACS_DEVICE_GUARD(h ? h->ctx : nullptr);
  ACS_CHECK(h ? h->ctx : nullptr, h && X, "fte_dist_reset: null handle or X");
  acs_ctx* ctx = h->ctx;
  const FteDims& d = h->S.d;
  FteBuffers& b = h->S.b;
  hipStream_t s = ctx->stream;
  // rounds of the previous solve still queued finish first (their snapshots are then stale)
  ACS_HIP(ctx, hipStreamSynchronize(s));
  if (int rc = fte_init_state(ctx, d, b, X, tau, flags)) return rc;
  hipLaunchKernelGGL(k_fte_state_reset, dim3(1), dim3(64), 0, s, b.st, h->lam0);
  ACS_HIP(ctx, hipGetLastError());
  h->rounds = 0;
  return ACS_OK;
}

int acs_fte_dist_destroy(acs_fte_dist* h) {
  ACS_DEVICE_GUARD(h ? h->ctx : nullptr);
  if (!h) return ACS_OK;
  (void)hipStreamSynchronize(h->ctx->stream);
  for (auto& c : h->g)
    if (c.exec) (void)hipGraphExecDestroy(c.exec);
  for (auto& e : h->snap_ev)
    if (e) (void)hipEventDestroy(e);
  if (h->snap) (void)acs_host_free(h->snap);
  if (h->own) (void)acs_dev_free(h->own);
  if (h->own_red) (void)acs_dev_free(h->own_red);
  delete h;
  return ACS_OK;
}

// payload of the starting state: the reduced system at X0 and the owned terms' cost
int acs_fte_dist_init(acs_fte_dist* h, double* payload) {
  ACS_DEVICE_GUARD(h ? h->ctx : nullptr);
  acs_ctx* ctx = h->ctx;
  const FteDims& d = h->S.d;
  FteBuffers& b = h->S.b;
  hipStream_t s = ctx->stream;
  double* p3 = payload + h->Lo.n1;
  if (h->c_hi > h->c_lo) fte_launch_cost(d, s, b, h->c_lo, h->c_hi - h->c_lo, h->own_lo, h->own_hi);
  hipLaunchKernelGGL(k_dist_cost_pack, dim3(1), dim3(256), 0, s, b.st, 0, d.N, h->c_lo, h->c_hi, h->c_lo, h->c_hi,
                     (const double*)b.Fm, (const double*)b.Fq, 0, 0, (const double*)nullptr, p3);
  // the linearisation of the starting state (copy 0); later ones are speculative (phase 3)
  if (h->a0 < d.nblk && h->k_hi > h->k_lo)
    fte_launch_lin(d, s, b, 1, h->k_lo, h->k_hi - h->k_lo);
  ACS_HIP(ctx, hipGetLastError());
  return dist_phase1_body(h, payload);
}

// one LM step: decide on the pending step (summed cost in `in`), solve the summed reduced
// system of `in`, step the chain, the new trial cost -> `out`, then the reduced system at the
// trial state (or, after a rejection, at the unchanged state) -> `out`
int acs_fte_dist_round(acs_fte_dist* h, const double* in, double* out) {
  ACS_DEVICE_GUARD(h ? h->ctx : nullptr);
  ACS_CHECK(h ? h->ctx : nullptr, h && in && out && in != out, "fte_dist_round: two distinct payload buffers");
  acs_ctx* ctx = h->ctx;
  FteBuffers& b = h->S.b;
  hipStream_t s = ctx->stream;
  const size_t n1 = h->Lo.n1;
  int rc = dist_run_captured(h, in, out, [&] {
    hipLaunchKernelGGL(k_dist_decide, dim3(1), dim3(64), 0, s, b.st, h->o, in + n1);
    int r2 = dist_phase2_body(h, in);
    if (r2) return r2;
    if ((r2 = dist_phase3_body(h, out + n1))) return r2;
    hipLaunchKernelGGL(k_dist_spec, dim3(1), dim3(64), 0, s, b.st, 1);
    if ((r2 = dist_phase1_body(h, out))) return r2;
    hipLaunchKernelGGL(k_dist_spec, dim3(1), dim3(64), 0, s, b.st, 0);
    ACS_HIP(ctx, hipGetLastError());
    return ACS_OK;
  });
  if (rc) return rc;
  const int slot = (int)(h->rounds % ACS_DIST_RING);
  ACS_HIP(ctx, hipMemcpyAsync(h->snap + slot, &b.st->status, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  ACS_HIP(ctx, hipEventRecord(h->snap_ev[slot], s));
  h->rounds++;
  return ACS_OK;
}

// LM status after round r (waits for that round only)
int acs_fte_dist_poll(acs_fte_dist* h, int64_t round, int32_t* status) {
  ACS_DEVICE_GUARD(h ? h->ctx : nullptr);
  ACS_CHECK(h ? h->ctx : nullptr, h && status && round >= 0 && round < h->rounds && round >= h->rounds - ACS_DIST_RING,
            "fte_dist_poll: round %lld not among the last %d enqueued", (long long)round, ACS_DIST_RING);
  const int slot = (int)(round % ACS_DIST_RING);
  ACS_HIP(h->ctx, hipEventSynchronize(h->snap_ev[slot]));
  *status = h->snap[slot];
  return ACS_OK;
}

int acs_fte_dist_gather(acs_fte_dist* h, double* p2) {
  ACS_DEVICE_GUARD(h ? h->ctx : nullptr);
  acs_ctx* ctx = h->ctx;
  const FteDims& d = h->S.d;
  FteBuffers& b = h->S.b;
  hipStream_t s = ctx->stream;
  ACS_HIP(ctx, hipMemsetAsync(p2, 0, sizeof(double) * h->Lo.n2, s));
  if (h->out_hi > h->out_lo)
    hipLaunchKernelGGL(k_dist_x_out, dim3(64), dim3(256), 0, s, d, b.st, h->out_lo, h->out_hi, (const double*)b.X, p2,
                       (const double*)b.tau, h->k_lo, h->k_hi);
  ACS_HIP(ctx, hipGetLastError());
  return ACS_OK;
}

int acs_fte_dist_scatter(acs_fte_dist* h, const double* p2) {
  ACS_DEVICE_GUARD(h ? h->ctx : nullptr);
  acs_ctx* ctx = h->ctx;
  const FteDims& d = h->S.d;
  FteBuffers& b = h->S.b;
  hipLaunchKernelGGL(k_dist_x_in, dim3(64), dim3(256), 0, ctx->stream, d, b.st, p2, b.X, b.tau);
  ACS_HIP(ctx, hipGetLastError());
  return ACS_OK;
}

int acs_fte_dist_result(acs_fte_dist* h, double* X, double* tau, acs_fte_report* report, uint32_t flags) {
  ACS_DEVICE_GUARD(h ? h->ctx : nullptr);
  acs_ctx* ctx = h->ctx;
  FteState hs;
  ACS_HIP(ctx, hipMemcpyAsync(&hs, h->S.b.st, sizeof(hs), hipMemcpyDeviceToHost, ctx->stream));
  ACS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return fte_read_result(ctx, h->S, hs, X, tau, report, flags);
}

}  // extern "C"
