// fte_host.hpp — host side of the FTE solve: the problem record, buffer layout, fte_setup, the
// cyclic-reduction launchers and the per-iteration enqueue. Included by fte.hip after the kernels.
#pragma once

struct FteBuffers {
  int* I;
  double *Rl, *cams, *meas, *w, *qinv, *X, *tau;
  double *Hloc, *gloc, *Floc, *Tc, *Ab, *gb, *Bt, *gmaxp, *Dc, *Ec, *GBc, *Wc, *Tau, *dcv, *dtau, *normp, *Fm, *Fq, *part;
  double* Adiag;
  double *Ec2, *dL, *dR;  // second coupling buffer (levels alternate), pending Schur terms
  // frame-window ranks with per-frame delays: rows' gradients before the delay elimination,
  // per-row max |delay gradient| of the frame the row starts, per-block delay step / state norms
  double *graw, *gmaxt, *normt;
  int* bad;
  int* bk;                    // k_cr_back_all: ticket counter, partials counter
  unsigned long long* gdcv;   // k_cr_back_all: the step rows, then dtau, as {stamp, word} granules
  FteState* st;
};

// k_fte_linearize over frames [k0, k0 + nk) (spec: at the trial state, with the model terms in Fq)
static void fte_launch_lin(const FteDims& d, hipStream_t s, const FteBuffers& b, int force, int k0, int nk,
                           int spec = 0) {
  const LinKernel kf = lin_kernel(nk);
  const size_t lds = lin_lds_bytes(d);
  hipLaunchKernelGGL(kf, dim3(nk), dim3(256), lds, s, d, b.I, b.Rl, b.cams, b.meas, b.w, b.X, b.tau,
                     b.st, force, k0, b.Hloc, b.gloc, b.Floc, spec, spec ? b.Fq : (double*)nullptr,
                     spec ? (const double*)b.qinv : (const double*)nullptr, b.Tc);
}

// k_fte_cost at the current state: frames [k0, k0 + nk), the terms owned by rows [lo, hi)
// (the default: every frame, every term)
static void fte_launch_cost(const FteDims& d, hipStream_t s, const FteBuffers& b, int k0 = 0, int nk = -1, int lo = 0,
                            int hi = INT_MAX) {
  hipLaunchKernelGGL(k_fte_cost, dim3(nk < 0 ? d.N : nk), dim3(64), 0, s, d, b.I, b.Rl, b.cams, b.meas, b.w, b.X,
                     b.tau, b.qinv, b.st, 0, k0, lo, hi, b.Fm, b.Fq);
}

// One FTE problem as every entry point receives it (include/acinoset_hip.h): the skeleton table
// blobs, cameras, measurements and weights, the model, the starting state and the loss constants.
struct FteProblem {
  const int32_t* skel_ints;
  int64_t n_ints;
  const double* skel_reals;
  int64_t n_reals;
  const double* cams;
  int32_t n_cams;
  const double *meas, *w;
  int32_t N, sd;
  double Ts;
  const double* qinv;
  int32_t sd_mode, intermode;
  const double *X, *tau;
  uint32_t flags;
  double la = 3.0, lb = 10.0, lc = 20.0;
};

struct FteSetup {
  FteState* snap = nullptr;  // pinned host slots the LM kernel writes its state into
  int n_cu = 256;            // the context's device (k_cr_assemble_build's instance: cr_asm_threads)
  FteDims d;
  FteBuffers b;
};

// The sizes that choose the solve's kernels and grids: the 3-frame super-blocks (nblk of BP
// rows), the tau border (Cg constant delays + the gradient column, GR wide) and the
// cyclic-reduction depth
static void fte_shape(FteDims& d, int N, int P, int n_cams, int sd, int sd_mode) {
  d.N = N;
  d.M = N + 2;
  d.P = P;
  d.C = n_cams;
  d.var = sd && sd_mode == 1;
  d.Ct = sd ? n_cams : 0;
  d.Cg = sd && !d.var ? n_cams : 0;
  d.NT = d.var ? N * n_cams : n_cams;
  d.NZ = P + 6 + d.Ct;
  d.nblk = (d.M + 2) / 3;
  d.BP = ((3 * P + 15) / 16) * 16;
  d.GR = ((d.Cg + 1 + 15) / 16) * 16;
  d.nlev = 0;
  for (int s = 1; s < d.nblk; s <<= 1) d.nlev++;
}

// The solve's buffers carved out of `base` (null: only the size is counted), then, with `inputs`
// (the owned mode), the staged inputs after them. Returns the bytes taken.
static size_t fte_carve(double* base, const FteDims& d, bool inputs, FteBuffers& b) {
  Arena A{base};
  const size_t N = d.N, M = d.M, P = d.P, C = d.C, BP = d.BP, GR = d.GR, n = d.nblk, NZ = FTE_NZP;
  const size_t Cg1 = d.Cg ? d.Cg : 1;
  // the per-frame linearisation is double-buffered: the speculative linearisation of the
  // trial state (k_fte_linearize spec = 1) writes copy cur ^ 1 (single-GPU and frame-window)
  const size_t nlin = 2;
  b.X = A.take(2 * M * P);
  b.tau = A.take(2 * (size_t)d.NT);
  b.Adiag = A.take(M * P);
  b.Hloc = A.take(nlin * N * NZ * NZ);
  b.gloc = A.take(nlin * N * NZ);
  b.Floc = A.take(nlin * N);
  b.Ab = A.take(M * 4 * P * P);
  b.gb = A.take(M * P);
  b.Bt = A.take(M * P * Cg1);
  b.gmaxp = A.take(M);
  b.Dc = A.take(n * BP * BP);
  b.Ec = A.take(n * BP * BP);
  b.GBc = A.take(n * BP * GR);
  b.Wc = A.take(n * BP * (2 * BP + GR));
  b.Tau = A.take(n * GR * GR);
  b.Ec2 = A.take(n * BP * BP);
  b.dL = A.take(n * BP * (BP + GR));
  b.dR = A.take(n * BP * (BP + GR));
  b.dcv = A.take(n * BP);
  b.dtau = A.take(GR);
  b.part = A.take((size_t)CR_NCHUNK * (32 * 32 + 32 + 32 * 32 + 1));
  b.normp = A.take(2 * n);
  b.Tc = A.take(nlin * N * std::max(tc_stride(d.Cg), 1));
  b.Fm = A.take(N);
  b.Fq = A.take(N);
  b.st = A.take<FteState>(16);
  b.bad = A.take<int>(8);
  b.graw = A.take(M * P);
  b.gmaxt = A.take(M);
  b.normt = A.take(2 * n);
  b.bk = A.take<int>(n / 2 + 2);
  b.gdcv = A.take<unsigned long long>(n * BP * 2 + 64);
  if (inputs) {
    b.I = A.take<int>(((size_t)d.nint + 1) / 2 + 1);
    b.Rl = A.take((size_t)d.nreal);
    b.cams = A.take((size_t)ACS_CAM_STRIDE * C);
    b.meas = A.take(N * C * d.L * 2);
    b.w = A.take(N * C * d.L);
    b.qinv = A.take(P);
  }
  return A.bytes();
}

// X / tau of a new solve from the caller (host or, with ACS_DEVICE_PTRS, device pointers; tau
// NULL = zeros) and the rest of the state buffers zeroed, in one launch (was six copies / fills):
// host inputs are copied into copy 0 first and the kernel then works in place
static int fte_init_state(acs_ctx* ctx, const FteDims& d, const FteBuffers& b, const double* X, const double* tau,
                          uint32_t flags) {
  hipStream_t s = ctx->stream;
  const double* Xs = X;
  const double* ts = tau;
  if (!(flags & ACS_DEVICE_PTRS)) {
    ACS_HIP(ctx, hipMemcpyAsync(b.X, X, sizeof(double) * d.M * d.P, hipMemcpyHostToDevice, s));
    if (tau) ACS_HIP(ctx, hipMemcpyAsync(b.tau, tau, sizeof(double) * d.NT, hipMemcpyHostToDevice, s));
    Xs = b.X;
    ts = tau ? b.tau : nullptr;
  }
  const int n = d.nblk;
  const size_t MP = (size_t)d.M * d.P;
  const size_t ngd = (size_t)n * d.BP * 2 + 64;
  const size_t nI = std::max(std::max(std::max(MP, (size_t)n + 1), ngd), (size_t)std::max(d.NT, d.GR));
  hipLaunchKernelGGL(k_fte_init_state, dim3(acs_grid((int64_t)nI, 256)), dim3(256), 0, s, b.X, Xs, MP, b.tau, ts,
                     d.NT, b.bad, b.dtau, d.GR, b.bk, n + 1, b.gdcv, ngd);
  return ACS_OK;
}

// The LM state of a new solve: damping lam, linearisation due; `first`: the frame-window
// rounds' first round pending (acs_fte_dist_create)
static int fte_upload_state(acs_ctx* ctx, FteSetup& S, double lam, int first = 0) {
  FteState st0;
  std::memset(&st0, 0, sizeof(st0));
  st0.lam = lam;
  st0.relin = 1;
  st0.first = first;
  ACS_HIP(ctx, hipMemcpyAsync(S.b.st, &st0, sizeof(st0), hipMemcpyHostToDevice, ctx->stream));
  return ACS_OK;
}

// Dimensions, device buffers and initial state of one FTE problem. With `owned` == NULL
// the buffers live in the context workspace (acs_fte_solve / acs_fte_eval); otherwise one
// hipMalloc block is allocated for them and returned in *owned (the distributed handles,
// several of which may share a context).
static int fte_setup(acs_ctx* ctx, FteSetup& S, const FteProblem& pb, void** owned = nullptr) {
  const int64_t n_ints = pb.n_ints, n_reals = pb.n_reals;
  const int32_t n_cams = pb.n_cams, N = pb.N, sd = pb.sd, sd_mode = pb.sd_mode, intermode = pb.intermode;
  const double Ts = pb.Ts;
  const uint32_t flags = pb.flags;
  int hdr[FK_HDR];
  if (flags & ACS_DEVICE_PTRS)
    ACS_HIP(ctx, hipMemcpy(hdr, pb.skel_ints, sizeof(hdr), hipMemcpyDeviceToHost));
  else
    std::memcpy(hdr, pb.skel_ints, sizeof(hdr));
  const int Jn = hdr[0], K = hdr[1], P = hdr[2], L = hdr[3];
  ACS_CHECK(ctx, Jn > 0 && Jn <= FK_MAXJ && K <= FK_MAXN && P >= 3 && P <= FK_MAXP && L >= 1 && L <= K,
            "fte: skeleton table out of range");
  ACS_CHECK(ctx, n_ints == FK_HDR + 9 * Jn + 4 * K + L + 4 * P + K * P && n_reals == 3 * K, "fte: blob sizes");
  ACS_CHECK(ctx, N >= 2 && n_cams >= 1 && n_cams <= FTE_MAXC && Ts > 0, "fte: N=%d C=%d Ts=%g", N, n_cams, Ts);
  ACS_CHECK(ctx, intermode >= 0 && intermode <= 2 && (sd ? intermode >= 1 : intermode == 0),
            "fte: shutter_delay=%d needs intermode %s (got %d), as src/core/fte.py:44-48", sd,
            sd ? "vel/acc" : "pos", intermode);
  ACS_CHECK(ctx, sd_mode == 0 || sd_mode == 1, "fte: shutter_delay_mode %d (0 const, 1 variable)", sd_mode);
  S.n_cu = ctx->n_cu;
  FteDims& d = S.d;
  fte_shape(d, N, P, n_cams, sd, sd_mode);
  d.L = L;
  d.nint = (int)n_ints;
  d.nreal = (int)n_reals;
  d.pad_ = 0;
  ACS_CHECK(ctx, d.NZ <= FTE_NZP, "fte: P + 6 + C = %d exceeds %d", d.NZ, FTE_NZP);
  d.im = intermode;
  d.Ts = Ts;
  d.la = pb.la;
  d.lb = pb.lb;
  d.lc = pb.lc;
  ACS_CHECK(ctx, d.BP <= CR_MAXBP, "fte: 3P = %d exceeds %d", 3 * P, CR_MAXBP);
  const int C = d.C;
  FteBuffers& b = S.b;
  hipStream_t s = ctx->stream;
  const size_t bI = sizeof(int32_t) * n_ints, bR = sizeof(double) * n_reals, bC = sizeof(double) * ACS_CAM_STRIDE * C,
               bM = sizeof(double) * (size_t)N * C * L * 2, bW = sizeof(double) * (size_t)N * C * L,
               bQ = sizeof(double) * P;
  if (owned) {
    // the staged inputs follow the buffers in the same allocation
    const hipMemcpyKind kin = (flags & ACS_DEVICE_PTRS) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    void* p = nullptr;
    ACS_HIP(ctx, acs_dev_malloc(&p, fte_carve(nullptr, d, true, b)));
    *owned = p;
    fte_carve((double*)p, d, true, b);
    ACS_HIP(ctx, hipMemcpyAsync(b.I, pb.skel_ints, bI, kin, s));
    ACS_HIP(ctx, hipMemcpyAsync(b.Rl, pb.skel_reals, bR, kin, s));
    ACS_HIP(ctx, hipMemcpyAsync(b.cams, pb.cams, bC, kin, s));
    ACS_HIP(ctx, hipMemcpyAsync(b.meas, pb.meas, bM, kin, s));
    ACS_HIP(ctx, hipMemcpyAsync(b.w, pb.w, bW, kin, s));
    ACS_HIP(ctx, hipMemcpyAsync(b.qinv, pb.qinv, bQ, kin, s));
  } else {
    // the staged inputs in workspace slots of their own (or the caller's device pointers)
    int rc;
    void* p;
    if ((rc = acs_stage_in(ctx, WS_FTE0, pb.skel_ints, bI, flags, &p))) return rc;
    b.I = (int*)p;
    if ((rc = acs_stage_in(ctx, WS_FTE1, pb.skel_reals, bR, flags, &p))) return rc;
    b.Rl = (double*)p;
    if ((rc = acs_stage_in(ctx, WS_CAMS, pb.cams, bC, flags, &p))) return rc;
    b.cams = (double*)p;
    if ((rc = acs_stage_in(ctx, WS_FTE2, pb.meas, bM, flags, &p))) return rc;
    b.meas = (double*)p;
    if ((rc = acs_stage_in(ctx, WS_FTE3, pb.w, bW, flags, &p))) return rc;
    b.w = (double*)p;
    if ((rc = acs_stage_in(ctx, WS_FTE4, pb.qinv, bQ, flags, &p))) return rc;
    b.qinv = (double*)p;
    double* arena = (double*)acs_ws(ctx, WS_FTE5, fte_carve(nullptr, d, false, b));
    if (!arena) return ACS_E_NOMEM;
    fte_carve(arena, d, false, b);
  }
  if (int rc = fte_init_state(ctx, d, b, pb.X, pb.tau, flags)) return rc;
  ACS_HIP(ctx, hipGetLastError());
  return ACS_OK;
}

// workgroups per eliminated block of a k_cr_level launch: enough column waves (16 - NB per
// workgroup), and more of them when few blocks are left (the deep levels are latency-bound):
// the widest split whose grid still fits the 256 CUs in one wave of workgroups (one
// 1024-thread workgroup per CU: the LDS is full), one column-block per workgroup when
// possible, else 6 / 4 / 3 / 2 column-blocks' worth of workgroups per block
static int cr_nsplit(const FteDims& d, int ne, int ns) {
  const int NB = d.BP >> 4, NBB = 2 * NB + d.GR / 16;
  const int need = (NBB + 16 - NB - 1) / (16 - NB);
  int want = 1;
  for (int c : {NBB, 6, 4, 3, 2})
    if (c <= NBB && ne * c + ns <= 256) {
      want = c;
      break;
    }
  int n = std::min(std::max(need, want), NBB);
  // two GB column-blocks (GR = 32) over several workgroups: each workgroup's idle column
  // waves load the GB blocks it does not own (k_cr_level), so keep GRB of them idle
  const int GRB = d.GR / 16;
  while (GRB > 1 && n > 1 && n < NBB && 16 - NB - (NBB + n - 1) / n < GRB) ++n;
  return n;
}

// Pending-term bookkeeping of one cyclic reduction (k_cr_level): the terms of the levels with
// steps lo_s .. (current step)/2 have not been applied to the surviving blocks; bit l of
// symmask: the level of step 2^l stored its D parts as upper tiles.
struct CrPending {
  int lo_s = 1;
  unsigned symmask = 0;
};

// The cyclic-reduction kernels are templates on the tile count NB = BP/16 = 1 .. 6 (CR_MAXBP):
// CALL(nb) with the literal tile count. The selectors below return the instance a launcher runs.
#define CR_NB_SWITCH(NB, CALL) \
  switch (NB) {                \
    case 1: CALL(1); break;    \
    case 2: CALL(2); break;    \
    case 3: CALL(3); break;    \
    case 4: CALL(4); break;    \
    case 5: CALL(5); break;    \
    default: CALL(6); break;   \
  }
typedef decltype(&k_cr_build<1>) CrBuildKernel;
typedef decltype(&k_cr_assemble_build<1, 1024>) CrAsmBuildKernel;
typedef decltype(&k_cr_level<1, false, false>) CrLevelKernel;
typedef decltype(&k_cr_back_all<1, 1>) CrBackAllKernel;
typedef decltype(&k_cr_back_chain<1, 1>) CrBackChainKernel;

static CrBuildKernel cr_build_kernel(const FteDims& d) {
#define CR_PICK(nb) return k_cr_build<nb>
  CR_NB_SWITCH(d.BP >> 4, CR_PICK)
#undef CR_PICK
}
// wide: the 512-thread instance (compact LDS rows, cr_asm_threads)
static CrAsmBuildKernel cr_asm_build_kernel(const FteDims& d, bool wide) {
#define CR_PICK(nb) return wide ? k_cr_assemble_build<nb, 512> : k_cr_assemble_build<nb, 1024>
  CR_NB_SWITCH(d.BP >> 4, CR_PICK)
#undef CR_PICK
}
// k_cr_level of a level or of the top block: the GB2 instance for two GB column-blocks, else the
// DUP one where D is read as upper tiles (d_up), else the plain one
static CrLevelKernel cr_level_kernel(const FteDims& d, int d_up) {
#define CR_PICK(nb)                                                          \
  return d.GR > 16 ? k_cr_level<nb, true, false> : d_up ? k_cr_level<nb, false, true> : k_cr_level<nb, false, false>
  CR_NB_SWITCH(d.BP >> 4, CR_PICK)
#undef CR_PICK
}
// the back-substitution kernels: GRB = GR / 16 column-blocks of the border
static CrBackAllKernel cr_back_all_kernel(const FteDims& d) {
#define CR_PICK(nb) return d.GR <= 16 ? k_cr_back_all<nb, 1> : k_cr_back_all<nb, 2>
  CR_NB_SWITCH(d.BP >> 4, CR_PICK)
#undef CR_PICK
}
static CrBackChainKernel cr_back_chain_kernel(const FteDims& d) {
#define CR_PICK(nb) return d.GR <= 16 ? k_cr_back_chain<nb, 1> : k_cr_back_chain<nb, 2>
  CR_NB_SWITCH(d.BP >> 4, CR_PICK)
#undef CR_PICK
}

// one k_cr_level launch (template on the tile count NB = BP/16). Returns whether this level's
// pending Schur terms are stored as upper tiles (the one-wave-per-column-block path; the deep
// path of k_cr_level writes full tiles).
static int cr_launch_level(const FteDims& d, hipStream_t s, int sl, int a0, int iend, int top, int ne, int ns,
                           int astep, FteBuffers& b, const double* Ein, double* Eout, const CrPending& pend,
                           int l0 = 0, int d_up = 0) {
  if (ne + ns == 0) return 0;
  const int NB = d.BP >> 4, NBB = 2 * NB + d.GR / 16;
  const int nsplit = cr_nsplit(d, ne, ns);
  const int nwg = ne * nsplit + ns;
  const size_t lds = sizeof(double) * cr_level_lds_doubles(d.BP, d.GR);
  const CrLevelKernel kf = cr_level_kernel(d, d_up);
  hipLaunchKernelGGL(kf, dim3(nwg), dim3(1024), lds, s, d, sl, a0, iend, top, ne, astep, nsplit, pend.symmask,
                     pend.lo_s, 0, l0, (const FteState*)b.st, b.Dc, Ein, Eout, b.GBc, b.Wc, b.Tau, b.dL, b.dR, b.bad,
                     CrTauSrc{});
  return (ne > 0 && !cr_level_deep(d.BP, NBB, nsplit)) ? 1 : 0;
}

static bool cr_defer() {
  static const bool v = acs_env_int("ACS_CR_DEFER", 0) == 1;
  return v;
}
// the single-GPU solve stores D as its upper tiles (k_cr_assemble_build) and levels 0-1 read it
// so (k_cr_level DUP): constant / no delays (the per-frame-delay mode builds through k_cr_build),
// one GB column-block (the GB2 instances have no DUP form), survivors not deferred
// (ACS_D_FULL=1: D stored whole, for A/B timing)
static bool fte_d_upper(const FteDims& d) {
  static const bool full = acs_env_int("ACS_D_FULL", 0) == 1;
  return !d.var && d.GR <= 16 && !cr_defer() && !full;
}

// blocks eliminated (ne) and survivors applying the previous level's terms (ns) at the level of
// step sl of the chain [a0, top]
static void cr_level_counts(int a0, int iend, int top, int sl, int* ne, int* ns) {
  *ne = *ns = 0;
  for (int i = a0 + sl; i < iend; i += 2 * sl) ++*ne;
  if (sl > 1)
    for (int j = a0; j <= top; j += 2 * sl) ++*ns;
}

// Block cyclic reduction of super-blocks [a0, top] (blocks < iend may be eliminated; a
// chain end at iend survives), nlev levels, then (final_apply) every pending Schur term is
// applied to the survivors. Survivor workgroups apply the previous level's terms at every
// level. ACS_CR_DEFER=1 launches them only at a level whose grid then still fits the chip in
// one wave of workgroups, and the blocks subtract the deferred terms when they are next loaded:
// at 10,000 frames that saved 26 us at level 1 and cost 30 us at levels 2-4 (each deferred
// term is one more dependent round of loads, profiles/r05/seq10k_*.log), so it is off.
// Returns the buffer holding the final couplings E; *pend_out: what is still pending (for the
// top block).
struct CrReduceOpts {
  bool final_apply = true;        // apply every pending Schur term to the survivors at the end
  bool e_upper = true;            // level 0 reads every E as upper triangular (a chain just built)
  bool d_upper = false;           // D stored as upper tiles (fte_d_upper)
  CrPending* pend_out = nullptr;  // what is still pending afterwards
};
static const double* cr_reduce(const FteDims& d, hipStream_t s, FteBuffers& b, int a0, int iend, int top, int nlev,
                               const CrReduceOpts& o = CrReduceOpts()) {
  const bool defer = cr_defer();
  const double* Ein = b.Ec;
  double* Eout = b.Ec2;
  CrPending pend;
  int sl = 1;
  for (int lv = 0; lv < nlev; ++lv, sl <<= 1) {
    int ne, ns;
    cr_level_counts(a0, iend, top, sl, &ne, &ns);
    if (ns && defer && ne * cr_nsplit(d, ne, ns) + ns > 256) ns = 0;  // defer
    // level 0 of a chain built by k_cr_assemble_build / k_cr_build: every E is upper triangular.
    // d_upper (D stored as upper tiles): levels 0 and 1 read D as assembled (the level-1
    // survivors rewrite theirs whole; every block eliminated later is one of them)
    const int sym = cr_launch_level(d, s, sl, a0, iend, top, ne, ns, 2 * sl, b, Ein, Eout, pend,
                                    lv == 0 && o.e_upper ? 1 : 0, o.d_upper && lv <= 1 ? 1 : 0);
    if (ns) pend.lo_s = sl;  // the survivors now hold every term of the levels below sl
    pend.symmask |= (unsigned)sym << lv;
    double* t = const_cast<double*>(Ein);
    Ein = Eout;
    Eout = t;
  }
  if (nlev > 0 && o.final_apply) {
    int ns = 0;
    for (int j = a0; j <= top; j += sl) ++ns;
    cr_launch_level(d, s, sl, a0, iend, top, 0, ns, sl, b, Ein, Eout, pend, 0, o.d_upper && nlev <= 1 ? 1 : 0);
    pend.lo_s = sl;
  }
  if (o.pend_out) *o.pend_out = pend;
  return Ein;
}

// The single surviving block a0 after nlev levels (step sl = 2^nlev): its pending terms,
// then W_gb = D^-1 GB and Tau = GB^T W_gb on the register-tiled Gauss-Jordan of k_cr_level
// (top_mode); k_cr_top finishes with the tau border.
// with_partials: CR_NCHUNK more workgroups form the tau border partial sums and the frames'
// |g| max (b.part) meanwhile, for k_cr_back_all (the single-GPU chain, a0 = 0)
static void cr_launch_top(const FteDims& d, hipStream_t s, int nlev, int a0, int iend, FteBuffers& b,
                          const CrPending& pend, bool with_partials = false, int d_up = 0) {
  const CrTauSrc ts = with_partials ? CrTauSrc{b.Tc, b.gmaxp, b.part} : CrTauSrc{};
  const int nwg = with_partials ? 1 + CR_NCHUNK : 1;
  const int sl = 1 << nlev;
  const size_t lds = sizeof(double) * cr_level_lds_doubles(d.BP, d.GR);
  const CrLevelKernel kf = cr_level_kernel(d, d_up);
  hipLaunchKernelGGL(kf, dim3(nwg), dim3(1024), lds, s, d, sl, a0, iend, a0, 1, sl, 1, pend.symmask, pend.lo_s, 1, 0,
                     (const FteState*)b.st, b.Dc, b.Ec, b.Ec2, b.GBc, b.Wc, b.Tau, b.dL, b.dR, b.bad, ts);
}

// threads per block of k_cr_assemble_build: the 512-thread instance (compact LDS rows) when the
// grid is more than one round of 1024-thread blocks, two per CU
static int cr_asm_threads(int nblk, int n_cu) { return nblk > 2 * n_cu ? 512 : 1024; }

// The part of the chain a build launch covers. The default is the whole chain of the single-GPU
// solve; a frame-window rank builds blocks [b0, b0 + nblk) from the terms it owns (lowest row in
// [lo, hi)), leaves the chain ends end_l / end_r undamped and keeps every row's raw diagonal and
// gradient (rdiag, graw) for the payload.
struct CrChain {
  int b0 = 0, nblk = -1;  // nblk < 0: d.nblk
  int lo = 0, hi = INT_MAX;
  int end_l = -1, end_r = -1;
  double *rdiag = nullptr, *graw = nullptr;
};

// k_cr_build from the banded rows of k_fte_assemble (per-frame delays)
static void cr_launch_build(const FteDims& d, hipStream_t s, const FteBuffers& b, const CrChain& ch = CrChain()) {
  const int nblk = ch.nblk < 0 ? d.nblk : ch.nblk;
  if (nblk <= 0) return;
  const CrBuildKernel kf = cr_build_kernel(d);
  hipLaunchKernelGGL(kf, dim3(nblk), dim3(1024), 0, s, d, (const FteState*)b.st, (const double*)b.Ab,
                     (const double*)b.gb, (const double*)b.Bt, b.Dc, b.Ec, b.GBc, ch.b0, ch.end_l, ch.end_r,
                     (const double*)b.Adiag);
}

// k_cr_assemble_build (constant / no delays); d_full: D stored whole instead of as upper tiles
static void cr_launch_assemble_build(const FteDims& d, int n_cu, hipStream_t s, const FteBuffers& b, int d_full,
                                     const CrChain& ch = CrChain()) {
  const int nblk = ch.nblk < 0 ? d.nblk : ch.nblk;
  if (nblk <= 0) return;
  const int th = cr_asm_threads(nblk, n_cu);
  const CrAsmBuildKernel kf = cr_asm_build_kernel(d, th < 1024);
  hipLaunchKernelGGL(kf, dim3(nblk), dim3(th), asm_build_lds_bytes(d, th < 1024), s, d, b.X, b.qinv, b.st, b.Hloc,
                     b.gloc, b.Dc, b.Ec, b.GBc, b.gmaxp, ch.b0, ch.lo, ch.hi, ch.end_l, ch.end_r, ch.rdiag, ch.graw,
                     d_full);
}

static void fte_enqueue_linearize(FteSetup& S, hipStream_t s, int force) {
  const FteDims& d = S.d;
  FteBuffers& b = S.b;
  fte_launch_lin(d, s, b, force, 0, d.N);
  hipLaunchKernelGGL(k_fte_assemble, dim3(d.M), dim3(256), 0, s, d, b.X, b.tau, b.qinv, b.st, force, 0, 0, INT_MAX,
                     b.Hloc, b.gloc, b.Ab, b.gb, b.Bt, b.gmaxp, b.Adiag, 1);
}

// one LM iteration: linearise (if the last step was accepted), cyclic-reduction solve,
// trial state, exact cost, accept/reject — all device-resident, no host round trip
static void fte_enqueue_iteration(FteSetup& S, hipStream_t s, const FteOptsDev& o) {
  const FteDims& d = S.d;
  FteBuffers& b = S.b;
  // D stored as upper tiles by k_cr_assemble_build (constant / no delays; the per-frame-delay
  // mode builds through k_cr_build, whole): read as assembled by levels 0-1 and by the top block
  // when no survivor ever rewrote it (nlev <= 1); off with ACS_CR_DEFER (survivors deferred)
  const bool dup = fte_d_upper(d);
  // the linearisation of X[cur] is already there (initial, or speculative at the last
  // accepted trial): assemble the banded rows and build the damped super-blocks (variable
  // delays: assembled when new or re-eliminated for a new damping, then built)
  if (d.var) {
    hipLaunchKernelGGL(k_fte_assemble, dim3(d.M), dim3(256), 0, s, d, b.X, b.tau, b.qinv, b.st, 0, 0, 0, INT_MAX,
                       b.Hloc, b.gloc, b.Ab, b.gb, b.Bt, b.gmaxp, b.Adiag, 1);
    cr_launch_build(d, s, b);
  } else {
    cr_launch_assemble_build(d, S.n_cu, s, b, dup ? 0 : 1);
  }
  const int bend = d.nblk - 1;
  CrPending pend;
  CrReduceOpts ro;
  ro.final_apply = false;  // the top block applies what is pending
  ro.d_upper = dup;
  ro.pend_out = &pend;
  cr_reduce(d, s, b, 0, d.nblk, d.nblk - 1, d.nlev, ro);
  cr_launch_top(d, s, d.nlev, 0, d.nblk, b, pend, true, dup && d.nlev <= 1 ? 1 : 0);
  // the top block and every back-substitution level in one launch, chained by
  // per-launch stamps (running the top levels' few blocks one after the other inside one
  // workgroup was tried in r03 and took 30 us: one workgroup streams a block's W at ~2 us, so
  // the W loads of every block have to be in flight at once). Constant / no delays: the
  // trial state is stepped there too; variable delays need the neighbours' rows: k_cr_trial
  double* Xt = d.var ? nullptr : b.X;
  // 8 lanes per row of a block (cr_back_block): 640 threads at BP = 80, so two workgroups
  // share a CU (91 VGPRs, 5 waves per SIMD) and one's W loads overlap the other's wait
  // (template sizes: the columns each lane of a row holds, BP / 8 and GR / 8, no padding)
  const int nth_back = (8 * d.BP + 63) / 64 * 64;
  // blocks of levels >= late_lv wait for their inputs before loading W (ACS_BACK_LATE_LV; 30: never)
  static const int late_lv = acs_env_int("ACS_BACK_LATE_LV", 30, 0, 30);  // k_cr_back_all shifts 1 << late_lv
  const CrBackAllKernel kb = cr_back_all_kernel(d);
  hipLaunchKernelGGL(kb, dim3(d.nblk), dim3(nth_back), 0, s, d, bend, b.st, (const double*)b.Wc, (const double*)b.Tau,
                     (const double*)b.part, (const double*)b.gmaxp, b.tau, b.dtau, b.dcv, b.bk, b.gdcv, b.bad, Xt,
                     b.normp, late_lv);
  if (d.var)
    hipLaunchKernelGGL(k_cr_trial, dim3(d.nblk), dim3(256), 0, s, d, b.st, b.dcv, b.dtau, b.Hloc, b.gloc, b.X, b.tau,
                       b.normp, 1, 0, 1);
  // speculative linearisation at the trial state: its measurement terms and the model terms
  // are the trial cost (no separate cost pass)
  fte_launch_lin(d, s, b, 0, 0, d.N, 1);
  hipLaunchKernelGGL(k_fte_lm, dim3(1), dim3(FTE_LM_THREADS), 0, s, d, b.st, o, 0, b.Floc, b.Fq, b.normp, 1, S.snap);
}

// The end of a solve whose final LM state is hs: X and tau of the accepted copy to the caller (host
// or, with ACS_DEVICE_PTRS, device pointers), the pivot counter and the report. tau may be null;
// acs_fte_dist_result may also pass a null X (acs_fte_solve's X was its input: fte_setup read it)
static int fte_read_result(acs_ctx* ctx, const FteSetup& S, const FteState& hs, double* X, double* tau,
                           acs_fte_report* report, uint32_t flags) {
  const FteDims& d = S.d;
  const FteBuffers& b = S.b;
  hipStream_t s = ctx->stream;
  const hipMemcpyKind kout = (flags & ACS_DEVICE_PTRS) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (X) ACS_HIP(ctx, hipMemcpyAsync(X, b.X + (size_t)hs.cur * d.M * d.P, sizeof(double) * d.M * d.P, kout, s));
  if (tau) ACS_HIP(ctx, hipMemcpyAsync(tau, b.tau + (size_t)hs.cur * d.NT, sizeof(double) * d.NT, kout, s));
  int nbad = 0;
  ACS_HIP(ctx, hipMemcpyAsync(&nbad, b.bad, sizeof(int), hipMemcpyDeviceToHost, s));
  ACS_HIP(ctx, hipStreamSynchronize(s));
  if (report) {
    report->status = hs.status == 0 ? ACS_STATUS_MAXITER : hs.status;
    report->iters = hs.iters;
    report->n_accepted = hs.nacc;
    report->n_bad_pivots = nbad;
    report->cost_before = hs.F0;
    report->cost_after = hs.F;
    report->cost_meas = hs.Fmeas;
    report->cost_model = hs.Fmodel;
    report->grad_max = hs.gmax;
    report->lambda_final = hs.lam;
  }
  return ACS_OK;
}
