// common.hpp — context, device workspace, error plumbing and the two camera models
// shared by every translation unit of libacinoset_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "acinoset_hip.h"

// ------------------------------------------------------------------------------------
// Context
// ------------------------------------------------------------------------------------
enum WsSlot {
  WS_CAMS = 0, WS_UV, WS_MASK, WS_CAMID, WS_PTS, WS_PTIDX, WS_CAMIDX, WS_OUT0, WS_OUT1,
  WS_PERPT_F0, WS_PERPT_F1, WS_PERPT_I, WS_REPORT, WS_SORT0, WS_SORT1, WS_SORT2, WS_SORT3,
  WS_TMP0, WS_TMP1, WS_TMP2, WS_TMP3, WS_TMP4, WS_TMP5, WS_TMP6, WS_TMP7,
  WS_FTE0, WS_FTE1, WS_FTE2, WS_FTE3, WS_FTE4, WS_FTE5, WS_FTE6, WS_FTE7, WS_FTE8, WS_FTE9,
  WS_FTE10, WS_FTE11, WS_FTE12, WS_FTE13, WS_FTE14, WS_FTE15,
  WS_PIPE0, WS_PIPE1, WS_PIPE2, WS_PIPE3, WS_PIPE4, WS_PIPE5, WS_PIPE6, WS_PIPE7,
  WS_NSLOTS
};
struct acs_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  std::string err;
  void* ws[WS_NSLOTS] = {};
  size_t ws_bytes[WS_NSLOTS] = {};
  int n_cu = 256;
  // pinned (coherent) host slots the kernels write device-state snapshots into (the FTE
  // solve reads the LM status of iteration n while iteration n + 1 runs)
  void* pinned = nullptr;
  size_t pinned_bytes = 0;
  // device counter of singular solves of the last EKF enqueue (acs_ekf_run / the pipeline);
  // its own allocation, so that a device-pointer call can be checked after the fact
  // (acs_ekf_singular_count) whatever the workspace slots did since
  int* ekf_bad = nullptr;
  // factors and covariance blocks of acs_fte_covariance (fte_cov.hpp), allocated on first use
  // and kept: its own allocation, so the solve's workspace slots stay as they are
  void* fte_cov = nullptr;
  size_t fte_cov_bytes = 0;
  // which k_sba_lm instance run_lm takes where both are legal (acs_sba_set_lm_layout; sba.hip)
  int sba_lm_layout = ACS_SBA_LM_AUTO;
};

// Every device / pinned-host allocation and free the library makes goes through these, and
// counts one event in a process-wide counter (acs_alloc_events): a timed region that reuses its
// buffers shows no change.
hipError_t acs_dev_malloc(void** p, size_t bytes);
hipError_t acs_dev_free(void* p);
hipError_t acs_host_malloc(void** p, size_t bytes, unsigned flags);
hipError_t acs_host_free(void* p);

// Coherent pinned host buffer of at least `bytes` (grow-only).
// Returns nullptr (and sets the error) on failure.
void* acs_pinned(acs_ctx* ctx, size_t bytes);

int acs_fail(acs_ctx* ctx, int code, const char* fmt, ...);

// Makes `device` current for the lifetime of the guard and restores the caller's current
// device afterwards. Every exported entry point that allocates or launches holds one, so two
// contexts on different devices (or a call from another host thread) allocate workspace and
// launch on the context's own device, and the caller's (e.g. torch's) current device is left
// as it was.
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int device) {
    if (device < 0) return;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != device) (void)hipSetDevice(device);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};
#define ACS_DEVICE_GUARD(ctx) DeviceGuard _acs_dev_guard((ctx) ? (ctx)->device : -1)

#define ACS_HIP(ctx, call)                                                                 \
  do {                                                                                     \
    hipError_t _e = (call);                                                                \
    if (_e != hipSuccess)                                                                  \
      return acs_fail((ctx), ACS_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), \
                      __FILE__, __LINE__);                                                 \
  } while (0)

#define ACS_CHECK(ctx, cond, ...)                                                          \
  do {                                                                                     \
    if (!(cond)) return acs_fail((ctx), ACS_E_INVALID, __VA_ARGS__);                       \
  } while (0)

// Grow-only device workspace slot. Returns nullptr (and sets the error) on failure.
void* acs_ws(acs_ctx* ctx, int slot, size_t bytes);

// Host<->device staging: with ACS_DEVICE_PTRS the pointer is used as is.
int acs_stage_in(acs_ctx* ctx, int slot, const void* src, size_t bytes, uint32_t flags, void** dev);
int acs_stage_out(acs_ctx* ctx, void* dst, const void* dev, size_t bytes, uint32_t flags);
// Output buffer: the caller's device pointer, or a workspace slot to copy back later.
void* acs_out_buf(acs_ctx* ctx, int slot, void* dst, size_t bytes, uint32_t flags);

static inline int acs_grid(int64_t n, int block) { return (int)((n + block - 1) / block); }

// Integer tuning knob from the environment: def when unset, else its value clamped to [lo, hi].
// A caller keeps the result in a function-local static, so a knob is read once per process.
// The value is read with atoi, so an on/off knob (def 0, tested == 1) is on at "1" and off at "10".
static inline int acs_env_int(const char* name, int def, int lo = INT_MIN, int hi = INT_MAX) {
  const char* e = std::getenv(name);
  const int v = e ? std::atoi(e) : def;
  return v < lo ? lo : (v > hi ? hi : v);
}

// An observation list (any order) on the device and its per-point slot tensor (n_pts, K): uvp, mask,
// camid, deterministic (stable radix sort by point id); K = max obs/pt.
struct ObsSlots {
  const double *cams = nullptr, *uv = nullptr;
  const int32_t *pt_idx = nullptr, *cam_idx = nullptr;
  double* pts = nullptr;
  double2* uvp = nullptr;
  uint8_t *mask = nullptr, *camid = nullptr;
  int K = 1;
};
// Stages (cams, uv, pt_idx, cam_idx, pts) and builds the slots (sba.hip). fn names the entry point
// in the messages; a point with more than max_K observations is refused. Without observations:
// one empty slot per point.
int acs_stage_obs(acs_ctx* ctx, const char* fn, int max_K, int cam_stride, const double* cams, int n_cams,
                  const double* uv, const int32_t* pt_idx, const int32_t* cam_idx, int64_t n_obs, const double* pts,
                  int64_t n_pts, uint32_t flags, ObsSlots* o);

// One point = one aligned group of G lanes, G = 2 .. 64: CALL(g) with the literal group size
#define ACS_G_SWITCH(G, CALL) \
  switch (G) {                \
    case 2: CALL(2); break;   \
    case 4: CALL(4); break;   \
    case 8: CALL(8); break;   \
    case 16: CALL(16); break; \
    case 32: CALL(32); break; \
    default: CALL(64); break; \
  }

// 256-byte aligned runs of doubles carved out of one allocation. With a null base only the size
// is counted: a layout function runs once for bytes() and once more with the allocation.
struct Arena {
  double* base;
  size_t off = 0;
  template <class T = double>
  T* take(size_t n_doubles) {
    const size_t o = off;
    off += ((n_doubles * sizeof(double) + 255) / 256) * 256 / sizeof(double);
    return base ? (T*)(base + o) : nullptr;
  }
  size_t bytes() const { return off * sizeof(double); }
};

// ---- device-buffer stages shared by the entry points and the fused pipeline -------------
// Dense points-only SBA (sba.hip): the fused LM over (n_pts, C) observation slots; with a
// report, waits for it (else asynchronous on the context stream).
int acs_sba_dense_enqueue(acs_ctx* ctx, const double* dcams, int C, const double2* duv, const uint8_t* dmask,
                          int64_t n_pts, const double* dpts_in, double* dpts_out, const acs_sba_opts* opts,
                          acs_report* report, int model = 0);
// Pairwise triangulation of the dense slots (tri.hip): mean over adjacent pairs.
// model (both): 0 = fisheye records (the default), 1 = standard records (ACS_MODEL_*, below).
int acs_tri_dense_enqueue(acs_ctx* ctx, const double* dcams, int C, const double* duv, const uint8_t* dmask,
                          int64_t n_pts, double* dout, int32_t* dcnt, int model = 0);
// EKF + RTS smoother (ekf.hip) on device buffers.
struct EkfIo {
  const int* I = nullptr;
  const double *R = nullptr, *cams = nullptr, *meas = nullptr, *lik = nullptr, *rstd = nullptr, *Q = nullptr,
               *P0 = nullptr, *s0 = nullptr;
  double *x_pred = nullptr, *x_est = nullptr, *x_smooth = nullptr, *P_est = nullptr, *P_smooth = nullptr;
  long long* outliers = nullptr;  // set by acs_ekf_enqueue (device, one per sequence)
  int* bad = nullptr;             // set by acs_ekf_enqueue (device): singular update / gain solves
};
int acs_ekf_enqueue(acs_ctx* ctx, int n_ints, int n_reals, const int* hdr, int n_cams, int n_seq, int n_frames,
                    double fps, double thresh, double max_pixel_err, double eps, int ref_numerics, EkfIo& io);

#include "fastmath.hpp"

// ------------------------------------------------------------------------------------
// Fisheye camera model (cv::fisheye::projectPoints with alpha = 0; src/lib/calib.py:132,
// restated by the reference itself in src/core/fte.py:80-96). Camera record layout:
// [fx fy cx cy k1 k2 k3 k4 R00..R22 t0 t1 t2] (ACS_CAM_STRIDE = 20 doubles).
// ------------------------------------------------------------------------------------
struct ProjOut {
  double u, v;
  double J[6];   // d(u,v)/dX (world point), row-major 2x3
  double JY[6];  // d(u,v)/dY (camera-frame point Y = R X + t)
  double Y[3];
};

template <bool JAC, bool FTE_FORM = false>
__device__ __forceinline__ void fisheye_project(const double* __restrict__ c, double X0, double X1,
                                                double X2, ProjOut& o) {
  const double Y0 = fma(c[8], X0, fma(c[9], X1, fma(c[10], X2, c[17])));
  const double Y1 = fma(c[11], X0, fma(c[12], X1, fma(c[13], X2, c[18])));
  const double Y2 = fma(c[14], X0, fma(c[15], X1, fma(c[16], X2, c[19])));
  const double iz = rcp_nr(Y2);
  const double a = Y0 * iz;
  const double b = Y1 * iz;
  const double r2 = a * a + b * b;
  const double k1 = c[4], k2 = c[5], k3 = c[6], k4 = c[7];
  // r and 1/r from one reciprocal square root; OpenCV's guard r > 1e-8 (the FTE form's
  // r = sqrt(r2 + 1e-12) needs none)
  const bool big = FTE_FORM ? true : (r2 > 1e-16);
  const double rr = FTE_FORM ? r2 + 1e-12 : (big ? r2 : 1.0);
  const double ir = rsq_nr(rr);
  const double r = big ? rr * ir : 0.0;
  const double th = atan_pos(r);
  const double th2 = th * th;
  const double poly = 1.0 + th2 * (k1 + th2 * (k2 + th2 * (k3 + th2 * k4)));
  const double thd = th * poly;
  const double s = big ? thd * ir : 1.0;
  o.u = c[0] * (a * s) + c[2];
  o.v = c[1] * (b * s) + c[3];
  if (JAC) {
    // s'(r)/r = (thd'(th) r / (1 + r^2) - thd) / r^3   (0 below OpenCV's guard)
    const double dthd = 1.0 + th2 * (3.0 * k1 + th2 * (5.0 * k2 + th2 * (7.0 * k3 + th2 * 9.0 * k4)));
    double spr;
    if (FTE_FORM) {
      // r = sqrt(a^2+b^2+eps): dr/da = a/r, same formula with this r
      spr = (dthd * r * rcp_nr(1.0 + r * r) - thd) * (ir * ir * ir);
    } else {
      // zero below the guard by a multiply, not a branch (there the factor is exactly 0:
      // r = 0, thd = 0, ir = 1); the 0/1 factor is opaque to the compiler so that it does
      // not turn the product back into a branch around the reciprocal
      double keep = big ? 1.0 : 0.0;
      asm volatile("" : "+v"(keep));
      spr = (dthd * r * rcp_nr(1.0 + r2) - thd) * (ir * ir * ir) * keep;
    }
    const double duda = c[0] * (s + a * a * spr);
    const double dudb = c[0] * (a * b * spr);
    const double dvda = c[1] * (a * b * spr);
    const double dvdb = c[1] * (s + b * b * spr);
    // d(u,v)/dY = J_uv_ab * [[iz, 0, -a iz], [0, iz, -b iz]]
    const double u0 = duda * iz, u1 = dudb * iz, u2 = -(duda * a + dudb * b) * iz;
    const double v0 = dvda * iz, v1 = dvdb * iz, v2 = -(dvda * a + dvdb * b) * iz;
    o.JY[0] = u0;
    o.JY[1] = u1;
    o.JY[2] = u2;
    o.JY[3] = v0;
    o.JY[4] = v1;
    o.JY[5] = v2;
    o.Y[0] = Y0;
    o.Y[1] = Y1;
    o.Y[2] = Y2;
    // times R
    o.J[0] = u0 * c[8] + u1 * c[11] + u2 * c[14];
    o.J[1] = u0 * c[9] + u1 * c[12] + u2 * c[15];
    o.J[2] = u0 * c[10] + u1 * c[13] + u2 * c[16];
    o.J[3] = v0 * c[8] + v1 * c[11] + v2 * c[14];
    o.J[4] = v0 * c[9] + v1 * c[12] + v2 * c[15];
    o.J[5] = v0 * c[10] + v1 * c[13] + v2 * c[16];
  }
}

// u, v and d(u, v)/dX of the same model (OpenCV's r > 1e-8 guard) for the points-only SBA
// LM (k_sba_lm), with the camera-frame Jacobian folded into R's rows: with A = R_0 - a R_2 and
// B = R_1 - b R_2 (shared by both image rows), J_u = iz (du/da A + du/db B) and J_v likewise:
// 22 f64 operations instead of the 28 of forming d(u,v)/dY and multiplying by R
// (fisheye_project, which also returns JY and Y for the extrinsics SBA).
__device__ __forceinline__ void fisheye_uvj(const double* __restrict__ c, double X0, double X1, double X2, double& u,
                                            double& v, double* J) {
  const double Y0 = fma(c[8], X0, fma(c[9], X1, fma(c[10], X2, c[17])));
  const double Y1 = fma(c[11], X0, fma(c[12], X1, fma(c[13], X2, c[18])));
  const double Y2 = fma(c[14], X0, fma(c[15], X1, fma(c[16], X2, c[19])));
  const double iz = rcp_nr(Y2);
  const double a = Y0 * iz;
  const double b = Y1 * iz;
  const double r2 = a * a + b * b;
  const double k1 = c[4], k2 = c[5], k3 = c[6], k4 = c[7];
  const bool big = r2 > 1e-16;
  const double rr = big ? r2 : 1.0;
  const double ir = rsq_nr(rr);
  const double r = big ? rr * ir : 0.0;
  const double th = atan_pos(r);
  const double th2 = th * th;
  const double poly = 1.0 + th2 * (k1 + th2 * (k2 + th2 * (k3 + th2 * k4)));
  const double thd = th * poly;
  const double s = big ? thd * ir : 1.0;
  u = c[0] * (a * s) + c[2];
  v = c[1] * (b * s) + c[3];
  const double dthd = 1.0 + th2 * (3.0 * k1 + th2 * (5.0 * k2 + th2 * (7.0 * k3 + th2 * 9.0 * k4)));
  // zero below the guard by two selects of the result (there the product is exactly 0, as in
  // fisheye_project); the product is opaque to the compiler so that it does not turn the
  // selects back into a branch around the reciprocal
  double sprb = (dthd * r * rcp_nr(1.0 + r2) - thd) * (ir * ir * ir);
  asm volatile("" : "+v"(sprb));
  const double spr = big ? sprb : 0.0;
  const double ab = a * b * spr;
  const double fu = c[0] * iz, fv = c[1] * iz;
  const double ua = fu * (s + a * a * spr), ub = fu * ab;  // iz du/da, iz du/db
  const double va = fv * ab, vb = fv * (s + b * b * spr);  // iz dv/da, iz dv/db
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double A = fma(-a, c[14 + j], c[8 + j]), B = fma(-b, c[14 + j], c[11 + j]);
    J[j] = fma(ua, A, ub * B);
    J[3 + j] = fma(va, A, vb * B);
  }
}

// ------------------------------------------------------------------------------------
// Standard (pinhole) camera model (cv::projectPoints with up to 8 coefficients;
// src/lib/calib.py:65-67). Camera record layout:
// [fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 R00..R22 t0 t1 t2] (ACS_CAM_STRIDE_STD = 24 doubles;
// a shorter coefficient vector is zero-padded by the packer). With a = Y0/Y2, b = Y1/Y2,
// r2 = a^2 + b^2 and cd = (1 + k1 r2 + k2 r2^2 + k3 r2^3) / (1 + k4 r2 + k5 r2^2 + k6 r2^3):
//   xd = a cd + 2 p1 a b + p2 (r2 + 2 a^2),  yd = b cd + p1 (r2 + 2 b^2) + 2 p2 a b,
//   u = fx xd + cx, v = fy yd + cy.
// No guard: a point behind the camera projects by the same formula, as OpenCV's does. The null
// record (all zeros, t2 = 1) gives u = v = 0 and a zero Jacobian exactly (fx = fy = 0).
// ------------------------------------------------------------------------------------
enum : int { ACS_MODEL_FISHEYE = 0, ACS_MODEL_STANDARD = 1 };
template <int MODEL>
struct CamRec {
  static constexpr int stride = MODEL == ACS_MODEL_STANDARD ? ACS_CAM_STRIDE_STD : ACS_CAM_STRIDE;
  static constexpr int R = stride - 12;  // first entry of the rotation; t follows it
};
static inline int acs_cam_stride(int model) { return model == ACS_MODEL_STANDARD ? ACS_CAM_STRIDE_STD : ACS_CAM_STRIDE; }
static inline int acs_flags_model(uint32_t flags) {
  return (flags & ACS_CAMS_STANDARD) ? ACS_MODEL_STANDARD : ACS_MODEL_FISHEYE;
}
// every entry point whose cameras must be fisheye records starts with this
#define ACS_FISHEYE_ONLY(ctx, flags, fn) \
  ACS_CHECK(ctx, !((flags) & ACS_CAMS_STANDARD), fn ": the standard camera model (ACS_CAMS_STANDARD) is not supported here")

// the distorted normalised point and, with JAC, its partials (xa = dxd/da, xb = dxd/db = dyd/da,
// yb = dyd/db); c' = d cd / d r2 = (num' - cd den') / den
template <bool JAC>
__device__ __forceinline__ void standard_distort(const double* __restrict__ c, double a, double b, double& xd,
                                                 double& yd, double& xa, double& xb, double& yb) {
  const double k1 = c[4], k2 = c[5], p1 = c[6], p2 = c[7], k3 = c[8], k4 = c[9], k5 = c[10], k6 = c[11];
  const double aa = a * a, bb = b * b, ab = a * b;
  const double r2 = aa + bb;
  const double num = fma(r2, fma(r2, fma(r2, k3, k2), k1), 1.0);
  const double den = fma(r2, fma(r2, fma(r2, k6, k5), k4), 1.0);
  const double id = rcp_nr(den);
  const double cd = num * id;
  xd = fma(a, cd, fma(2.0 * p1, ab, p2 * (r2 + 2.0 * aa)));
  yd = fma(b, cd, fma(p1, r2 + 2.0 * bb, 2.0 * p2 * ab));
  if (JAC) {
    const double dnum = fma(r2, fma(r2, 3.0 * k3, 2.0 * k2), k1);
    const double dden = fma(r2, fma(r2, 3.0 * k6, 2.0 * k5), k4);
    const double cp2 = 2.0 * (dnum - cd * dden) * id;  // 2 c'
    xa = fma(aa, cp2, cd) + fma(2.0 * p1, b, 6.0 * p2 * a);
    xb = fma(ab, cp2, 2.0 * fma(p1, a, p2 * b));
    yb = fma(bb, cp2, cd) + fma(6.0 * p1, b, 2.0 * p2 * a);
  }
}

// fills the same ProjOut as fisheye_project
template <bool JAC>
__device__ __forceinline__ void standard_project(const double* __restrict__ c, double X0, double X1, double X2,
                                                 ProjOut& o) {
  const double Y0 = fma(c[12], X0, fma(c[13], X1, fma(c[14], X2, c[21])));
  const double Y1 = fma(c[15], X0, fma(c[16], X1, fma(c[17], X2, c[22])));
  const double Y2 = fma(c[18], X0, fma(c[19], X1, fma(c[20], X2, c[23])));
  const double iz = rcp_nr(Y2);
  const double a = Y0 * iz;
  const double b = Y1 * iz;
  double xd, yd, xa = 0.0, xb = 0.0, yb = 0.0;
  standard_distort<JAC>(c, a, b, xd, yd, xa, xb, yb);
  o.u = c[0] * xd + c[2];
  o.v = c[1] * yd + c[3];
  if (JAC) {
    const double duda = c[0] * xa, dudb = c[0] * xb, dvda = c[1] * xb, dvdb = c[1] * yb;
    const double u0 = duda * iz, u1 = dudb * iz, u2 = -(duda * a + dudb * b) * iz;
    const double v0 = dvda * iz, v1 = dvdb * iz, v2 = -(dvda * a + dvdb * b) * iz;
    o.JY[0] = u0;
    o.JY[1] = u1;
    o.JY[2] = u2;
    o.JY[3] = v0;
    o.JY[4] = v1;
    o.JY[5] = v2;
    o.Y[0] = Y0;
    o.Y[1] = Y1;
    o.Y[2] = Y2;
    o.J[0] = u0 * c[12] + u1 * c[15] + u2 * c[18];
    o.J[1] = u0 * c[13] + u1 * c[16] + u2 * c[19];
    o.J[2] = u0 * c[14] + u1 * c[17] + u2 * c[20];
    o.J[3] = v0 * c[12] + v1 * c[15] + v2 * c[18];
    o.J[4] = v0 * c[13] + v1 * c[16] + v2 * c[19];
    o.J[5] = v0 * c[14] + v1 * c[17] + v2 * c[20];
  }
}

// u, v and d(u, v)/dX for the points-only SBA LM (k_sba_lm), the camera-frame Jacobian folded
// into R's rows exactly as in fisheye_uvj: A = R_0 - a R_2, B = R_1 - b R_2,
// J_u = iz (du/da A + du/db B). Two reciprocals (1/Y2, 1/den), no atan and no rsq.
__device__ __forceinline__ void standard_uvj(const double* __restrict__ c, double X0, double X1, double X2, double& u,
                                             double& v, double* J) {
  const double Y0 = fma(c[12], X0, fma(c[13], X1, fma(c[14], X2, c[21])));
  const double Y1 = fma(c[15], X0, fma(c[16], X1, fma(c[17], X2, c[22])));
  const double Y2 = fma(c[18], X0, fma(c[19], X1, fma(c[20], X2, c[23])));
  const double iz = rcp_nr(Y2);
  const double a = Y0 * iz;
  const double b = Y1 * iz;
  double xd, yd, xa, xb, yb;
  standard_distort<true>(c, a, b, xd, yd, xa, xb, yb);
  u = c[0] * xd + c[2];
  v = c[1] * yd + c[3];
  const double fu = c[0] * iz, fv = c[1] * iz;
  const double ua = fu * xa, ub = fu * xb;  // iz du/da, iz du/db
  const double va = fv * xb, vb = fv * yb;  // iz dv/da, iz dv/db
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double A = fma(-a, c[18 + j], c[12 + j]), B = fma(-b, c[18 + j], c[15 + j]);
    J[j] = fma(ua, A, ub * B);
    J[3 + j] = fma(va, A, vb * B);
  }
}

// the model's projection by a template argument (the elementwise kernels and k_sba_lm)
template <int MODEL, bool JAC>
__device__ __forceinline__ void model_project(const double* __restrict__ c, double X0, double X1, double X2,
                                              ProjOut& o) {
  if constexpr (MODEL == ACS_MODEL_STANDARD)
    standard_project<JAC>(c, X0, X1, X2, o);
  else
    fisheye_project<JAC>(c, X0, X1, X2, o);
}

// ------------------------------------------------------------------------------------
// Redescending loss (src/lib/misc.py:329-343): value, d/de and d2/de2.
// ------------------------------------------------------------------------------------
struct LossOut {
  double f, d1, d2;
};

__device__ __forceinline__ LossOut redescending(double err, double a, double b, double c) {
  const double E = fabs(err);
  const double sa = rcp_nr(1.0 + exp(-(E - a)));
  const double sb = rcp_nr(1.0 + exp(-(E - b)));
  const double sc = rcp_nr(1.0 + exp(-(E - c)));
  const double da = sa * (1.0 - sa), db = sb * (1.0 - sb), dc = sc * (1.0 - sc);
  const double dda = da * (1.0 - 2.0 * sa), ddb = db * (1.0 - 2.0 * sb), ddc = dc * (1.0 - 2.0 * sc);
  const double lin = a * E - 0.5 * a * a;
  const double K3 = a * b - 0.5 * a * a;
  const double cb = c - b;
  const double icb = rcp_nr(cb);
  const double w = (c - E) * icb;
  const double q = K3 + (0.5 * a * cb) * (1.0 - w * w);
  const double q1 = a * (c - E) * icb;
  const double q2 = -a * icb;
  const double K4 = K3 + 0.5 * a * cb;
  LossOut o;
  o.f = (1.0 - sa) * 0.5 * E * E + (sa - sb) * lin + (sb - sc) * q + sc * K4;
  const double dE = -0.5 * da * E * E + (1.0 - sa) * E + (da - db) * lin + (sa - sb) * a +
                    (db - dc) * q + (sb - sc) * q1 + dc * K4;
  const double ddE = -0.5 * dda * E * E - 2.0 * da * E + (1.0 - sa) + (dda - ddb) * lin +
                     2.0 * (da - db) * a + (ddb - ddc) * q + 2.0 * (db - dc) * q1 + (sb - sc) * q2 +
                     ddc * K4;
  const double sg = err > 0.0 ? 1.0 : (err < 0.0 ? -1.0 : 0.0);
  o.d1 = dE * sg;
  o.d2 = ddE;
  return o;
}

// Sum inside an aligned group of G lanes; every lane ends with the bit-identical total
// (each step adds a lane's value to its partner's, and IEEE addition is commutative).
// Within a 16-lane row the partners come from DPP lane permutes (quad xor 1, quad xor 2,
// half-row mirror, row mirror) on the VALU; wider groups finish with LDS-routed shuffles.
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}

template <int G>
__device__ __forceinline__ double group_sum(double v) {
  if (G >= 2) v += dpp_f64<0xB1>(v);   // quad_perm [1,0,3,2]
  if (G >= 4) v += dpp_f64<0x4E>(v);   // quad_perm [2,3,0,1]
  if (G >= 8) v += dpp_f64<0x141>(v);  // row_half_mirror: quad 0 <-> quad 1 (quads uniform)
  if (G >= 16) v += dpp_f64<0x140>(v); // row_mirror: half 0 <-> half 1
  if (G >= 32) v += __shfl_xor(v, 16, G);
  if (G >= 64) v += __shfl_xor(v, 32, G);
  return v;
}

// The point rule of both covariances (k_sba_cov, k_extcov_linearize). v: the point's 3x3
// Gauss-Newton matrix, packed upper [00 01 02 11 12 22]. LDL^T without pivoting: H = L D L^T,
// H^-1 = sum_k (1 / d_k) m_k^T m_k with m_k the rows of L^-1 = [1 0 0; -l10 1 0; l10 l21 - l20,
// -l21, 1], into c (packed likewise). True when every pivot passes d > 1e-9 max(H00, H11, H22),
// written so that a NaN pivot or threshold fails. rcp is the caller's reciprocal.
#define ACS_COV_PIVOT_TOL 1e-9
template <class Rcp>
__device__ __forceinline__ bool ldl3_inverse(const double* v, Rcp rcp, double c[6]) {
  const double d0 = v[0], i0 = rcp(d0);
  const double l10 = v[1] * i0, l20 = v[2] * i0;
  const double d1 = v[3] - l10 * v[1], i1 = rcp(d1);
  const double t = v[4] - l20 * v[1];
  const double l21 = t * i1;
  const double d2 = v[5] - l20 * v[2] - l21 * t, i2 = rcp(d2);
  const double thr = ACS_COV_PIVOT_TOL * fmax(v[0], fmax(v[3], v[5]));
  const bool ok = d0 > thr && d1 > thr && d2 > thr;
  const double m20 = l10 * l21 - l20;
  c[5] = i2;
  c[4] = -l21 * i2;
  c[2] = m20 * i2;
  c[3] = i1 + l21 * l21 * i2;
  c[1] = -l10 * i1 - l21 * c[2];
  c[0] = i0 + l10 * l10 * i1 + m20 * c[2];
  return ok;
}
// ACS_COV_* of a point from its number of scalar residuals and ldl3_inverse's verdict
__device__ __forceinline__ int cov_point_status(double n_res, bool pivots_ok) {
  return n_res == 0.0 ? ACS_COV_NOOBS : pivots_ok ? ACS_COV_OK : ACS_COV_DEGENERATE;
}

// Row-broadcast group sums of k_sba_lm's ROW instances (sba.hip; one point per 16-lane DPP row, slots in lanes 0..K-1, K <= 8): the sums behind
// the first (quad_perm xor 1) stage are taken with row_newbcast, the one DPP control gfx950's
// f64 VALU accepts. After stage 1 lane 2j holds the pair sum s(2j,2j+1), and for every lane
//   v_mov_b64_dpp  t, s       row_newbcast:0   t  = s01
//   v_fmac_f64_dpp t, s, 1.0  row_newbcast:2   t  = fma(s23, 1.0, t) = s01 + s23, rounded once
//   v_fmac_f64_dpp t, s, 1.0  row_newbcast:4   t += s45
// is one issue slot per term, where the butterfly pays two 32-bit DPP moves and an add per
// stage. ROW is the number of pairs, (K + 1) / 2, and the tree is the butterfly's own:
//   ROW 2  s01 + s23                  = group_sum<4>
//   ROW 3  (s01 + s23) + s45          = group_sum<8>, whose s67 is the empty lanes' +0.0
//   ROW 4  (s01 + s23) + (s45 + s67)  = group_sum<8>
// so every sum has the bits of the butterfly instance's; the only possible difference would be
// the sign of a sum that is exactly zero (x + (+0.0) turns -0.0 into +0.0), and a lane's value
// is 0.0 + products here, never -0.0.
// Hazard the assembler does not see inside an asm statement: a DPP instruction must not read a
// VGPR that either of the two instructions before it wrote. The statements below run stage by
// stage over their values, and start with instructions that are not DPP.
#define ACS_ROW_BC(n) " row_newbcast:" #n " row_mask:0xf bank_mask:0xf\n\t"
#define ACS_ROW_MOV(d, s, n) "v_mov_b64_dpp %[" #d "], %[" #s "]" ACS_ROW_BC(n)
#define ACS_ROW_FMAC(d, s, n) "v_fmac_f64_dpp %[" #d "], %[" #s "], %[one]" ACS_ROW_BC(n)
#define ACS_ROW_ADD(d, a, b) "v_add_f64 %[" #d "], %[" #a "], %[" #b "]\n\t"
#define ACS_ROW_ADDT(d, t, n) ACS_ROW_ADD(d, d, t)
#define ACS_ROW9(OP, d, s, n)                                                                             \
  OP(d##0, s##0, n) OP(d##1, s##1, n) OP(d##2, s##2, n) OP(d##3, s##3, n) OP(d##4, s##4, n) OP(d##5, s##5, n) \
      OP(d##6, s##6, n) OP(d##7, s##7, n) OP(d##8, s##8, n)
// the nine H and g sums from their pair sums s0..s8 into h0..h8 (ROW 4: temporaries t0..t8);
// the operand lists name the caller's H[6], g[3], s[9+], one and t[9]
#define ACS_ROW_SUMS2 ACS_ROW9(ACS_ROW_MOV, h, s, 0) ACS_ROW9(ACS_ROW_FMAC, h, s, 2)
#define ACS_ROW_SUMS3 ACS_ROW_SUMS2 ACS_ROW9(ACS_ROW_FMAC, h, s, 4)
#define ACS_ROW_SUMS4                                                                                \
  ACS_ROW9(ACS_ROW_MOV, h, s, 0) ACS_ROW9(ACS_ROW_MOV, t, s, 4) ACS_ROW9(ACS_ROW_FMAC, h, s, 2)      \
  ACS_ROW9(ACS_ROW_FMAC, t, s, 6) ACS_ROW9(ACS_ROW_ADDT, h, t, 0)
#define ACS_ROW_H(c)                                                                                       \
  [h0] c(H[0]), [h1] c(H[1]), [h2] c(H[2]), [h3] c(H[3]), [h4] c(H[4]), [h5] c(H[5]), [h6] c(g[0]), [h7] c(g[1]), \
      [h8] c(g[2])
#define ACS_ROW_T                                                                                              \
  [t0] "=&v"(t[0]), [t1] "=&v"(t[1]), [t2] "=&v"(t[2]), [t3] "=&v"(t[3]), [t4] "=&v"(t[4]), [t5] "=&v"(t[5]), \
      [t6] "=&v"(t[6]), [t7] "=&v"(t[7]), [t8] "=&v"(t[8])
#define ACS_ROW_S                                                                                          \
  [s0] "v"(s[0]), [s1] "v"(s[1]), [s2] "v"(s[2]), [s3] "v"(s[3]), [s4] "v"(s[4]), [s5] "v"(s[5]), [s6] "v"(s[6]), \
      [s7] "v"(s[7]), [s8] "v"(s[8]), [one] "v"(one)

// Stage 1 of the ten sums (s[i] += q[i], q the xor-1 partner's value) and the cost's sum, which
// the accept decision waits for, in one statement: the cost's DPP instructions stand between
// the additions, each two instructions behind the last write of what it reads.
template <int ROW>
__device__ __forceinline__ double row_pairs_cost(double (&s)[10], const double (&q)[10], double one) {
  double c, c2;
#define ACS_ROW_PAIR(i) "v_add_f64 %[s" #i "], %[s" #i "], %[q" #i "]\n\t"
#define ACS_ROW_PAIR_OPS                                                                                       \
  [s0] "+v"(s[0]), [s1] "+v"(s[1]), [s2] "+v"(s[2]), [s3] "+v"(s[3]), [s4] "+v"(s[4]), [s5] "+v"(s[5]),          \
      [s6] "+v"(s[6]), [s7] "+v"(s[7]), [s8] "+v"(s[8]), [s9] "+v"(s[9])
#define ACS_ROW_PAIR_IN                                                                                        \
  [q0] "v"(q[0]), [q1] "v"(q[1]), [q2] "v"(q[2]), [q3] "v"(q[3]), [q4] "v"(q[4]), [q5] "v"(q[5]), [q6] "v"(q[6]), \
      [q7] "v"(q[7]), [q8] "v"(q[8]), [q9] "v"(q[9]), [one] "v"(one)
  if constexpr (ROW == 2) {
    asm(ACS_ROW_PAIR(9) ACS_ROW_PAIR(0) ACS_ROW_PAIR(1) ACS_ROW_MOV(c, s9, 0) ACS_ROW_PAIR(2) ACS_ROW_PAIR(3)
            ACS_ROW_FMAC(c, s9, 2) ACS_ROW_PAIR(4) ACS_ROW_PAIR(5) ACS_ROW_PAIR(6) ACS_ROW_PAIR(7) ACS_ROW_PAIR(8)
        : [c] "=&v"(c), ACS_ROW_PAIR_OPS
        : ACS_ROW_PAIR_IN);
  } else if constexpr (ROW == 3) {
    asm(ACS_ROW_PAIR(9) ACS_ROW_PAIR(0) ACS_ROW_PAIR(1) ACS_ROW_MOV(c, s9, 0) ACS_ROW_PAIR(2) ACS_ROW_PAIR(3)
            ACS_ROW_FMAC(c, s9, 2) ACS_ROW_PAIR(4) ACS_ROW_PAIR(5) ACS_ROW_FMAC(c, s9, 4) ACS_ROW_PAIR(6)
                ACS_ROW_PAIR(7) ACS_ROW_PAIR(8)
        : [c] "=&v"(c), ACS_ROW_PAIR_OPS
        : ACS_ROW_PAIR_IN);
  } else {
    static_assert(ROW == 4, "row-broadcast sums are written out for 2, 3 and 4 lane pairs");
    asm(ACS_ROW_PAIR(9) ACS_ROW_PAIR(0) ACS_ROW_PAIR(1) ACS_ROW_MOV(c, s9, 0) ACS_ROW_MOV(c2, s9, 4) ACS_ROW_PAIR(2)
            ACS_ROW_FMAC(c, s9, 2) ACS_ROW_FMAC(c2, s9, 6) ACS_ROW_PAIR(3) ACS_ROW_PAIR(4) ACS_ROW_ADD(c, c, c2)
                ACS_ROW_PAIR(5) ACS_ROW_PAIR(6) ACS_ROW_PAIR(7) ACS_ROW_PAIR(8)
        : [c] "=&v"(c), [c2] "=&v"(c2), ACS_ROW_PAIR_OPS
        : ACS_ROW_PAIR_IN);
  }
#undef ACS_ROW_PAIR
#undef ACS_ROW_PAIR_OPS
#undef ACS_ROW_PAIR_IN
  return c;
}

// The nine H and g sums from the pair sums, in every lane (the first linearisation; the LM
// pass takes them under the accepting lanes' mask, inside its accept statement).
template <int ROW>
__device__ __forceinline__ void row_sums9(double (&H)[6], double (&g)[3], const double (&s)[10], double one) {
  if constexpr (ROW == 2) {
    asm(ACS_ROW_SUMS2 : ACS_ROW_H("=&v") : ACS_ROW_S);
  } else if constexpr (ROW == 3) {
    asm(ACS_ROW_SUMS3 : ACS_ROW_H("=&v") : ACS_ROW_S);
  } else {
    double t[9];
    asm(ACS_ROW_SUMS4 : ACS_ROW_H("=&v"), ACS_ROW_T : ACS_ROW_S);
  }
}
