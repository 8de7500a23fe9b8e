// The ten group sums of one k_sba_lm linearisation (6 H + 3 g + 1 F over an 8-lane group), one
// wave per SIMD (one block of 256 threads), as a chain from pass to pass like the LM loop's:
//   base  group_sum<8> of common.hpp: 3 stages x (2 DPP moves + 1 add) x 10 values = 90 slots
//   mfma  a point's lanes at {2m, 2m+1} + 16k: a ones-matrix v_mfma_f64_16x16x4 sums the four
//         rows, one quad_perm stage finishes: (1 MFMA + 2 DPP moves + 1 add) x 10
//   half  recursive halving with bank_mask: the inter-quad stage leaves five sums in quad 0 and
//         five in quad 1 (4 DPP moves + 1 add per pair), two in-quad stages on five values,
//         a masked gather back (4 DPP moves per pair): 75 slots
//   add90 calibration: 90 independent v_add_f64 per pass (what 90 issue slots cost)
//   stage the kernel's own staged butterfly, group_sum10<8> of sba.hip (stage by stage over the
//         ten values, no DPP move behind the add it reads): 90 slots, no s_nop
//   row   (c) one point per 16-lane row, 6 live lanes (the headline's 6 cameras), the code of the
//         ROW instances (row_pairs_cost<3> and row_sums9<3> of common.hpp): a quad_perm pair stage,
//         then v_mov_b64_dpp row_newbcast:0 and two v_fmac_f64_dpp (x 1.0) row_newbcast:2 / :4
//         per value: 60 slots if each of them issues in one
// Prints clock64 ticks per pass and checks every variant's sums against base (1e-14 relative)
// and that all lanes of a group hold the same bits.
// Build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -I include tools/probe/group_sum10_probe.hip -o tools/probe/group_sum10_probe
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../acinoset_amd/csrc/common.hpp"

#define CK(call)                                                     \
  do {                                                               \
    const hipError_t e_ = (call);                                    \
    if (e_ != hipSuccess) {                                          \
      printf("%s: %s\n", #call, hipGetErrorString(e_));              \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)

enum { BASE = 0, MFMA = 1, HALF = 2, ADD90 = 3, STAGE = 4, ROWB = 5 };

template <int CTRL, int BANK>
__device__ __forceinline__ double dpp_upd(double old, double src) {
  const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(src), CTRL, 0xF, BANK, false);
  const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(src), CTRL, 0xF, BANK, false);
  return __hiloint2double(hi, lo);
}

typedef double double4v __attribute__((ext_vector_type(4)));

// group_sum10<8> as sba.hip has it, completed (the kernel leaves the last stage's nine additions
// to its accept statement; they are slots of the pass all the same)
template <int K>
__device__ __forceinline__ void staged10(double* v) {
#pragma unroll
  for (int i = 0; i < 10; ++i) v[i] += dpp_f64<K == 0 ? 0xB1 : K == 1 ? 0x4E : 0x141>(v[i]);
  if constexpr (K < 2) staged10<K + 1>(v);
}

template <int MODE>
__device__ __forceinline__ void sum10(double* v) {
  if (MODE == STAGE) {
    staged10<0>(v);
  } else if (MODE == ROWB) {
    double s[10], q[10], H[6], g[3];
#pragma unroll
    for (int i = 0; i < 10; ++i) s[i] = v[i];
#pragma unroll
    for (int i = 0; i < 10; ++i) q[i] = dpp_f64<0xB1>(s[i]);
    v[9] = row_pairs_cost<3>(s, q, 1.0);
    row_sums9<3>(H, g, s, 1.0);
#pragma unroll
    for (int i = 0; i < 6; ++i) v[i] = H[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) v[6 + i] = g[i];
  } else if (MODE == BASE) {
#pragma unroll
    for (int i = 0; i < 10; ++i) v[i] = group_sum<8>(v[i]);
  } else if (MODE == MFMA) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
      const double4v z = {0.0, 0.0, 0.0, 0.0};
      const double4v d = __builtin_amdgcn_mfma_f64_16x16x4f64(1.0, v[i], z, 0, 0, 0);
      v[i] = d[0] + dpp_f64<0xB1>(d[0]);
    }
  } else if (MODE == HALF) {
    // banks (4-lane quads of a 16-lane row) 0 and 2 are the groups' quad 0, 1 and 3 their quad 1
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const double x = dpp_upd<0x141, 0x5>(v[i + 5], v[i]);  // quad 0: partner's v[i]; quad 1: own v[i+5]
      const double y = dpp_upd<0x141, 0xA>(v[i], v[i + 5]);  // quad 0: own v[i]; quad 1: partner's v[i+5]
      double w = x + y;
      w += dpp_f64<0xB1>(w);
      w += dpp_f64<0x4E>(w);
      v[i] = dpp_upd<0x141, 0xA>(w, w);      // quad 1 takes quad 0's
      v[i + 5] = dpp_upd<0x141, 0x5>(w, w);  // quad 0 takes quad 1's
    }
  }
}

// the lane of the base layout whose value this lane holds (MFMA layout: camera = (lane & 1) +
// 2 (lane >> 4) of point (lane & 15) >> 1)
template <int MODE>
__device__ __forceinline__ int base_lane(int l) {
  return MODE == MFMA ? 8 * ((l & 15) >> 1) + (l & 1) + 2 * (l >> 4) : MODE == ROWB ? 8 * (l >> 4) + (l & 7) : l;
}
// ROWB: lanes 6..15 of a row are empty slots (exact zeros, as the null camera's)
template <int MODE>
__device__ __forceinline__ bool slot_live(int l) {
  return MODE != ROWB || (l & 15) < 6;
}

template <int MODE>
__global__ __launch_bounds__(256) void k(double* out, long long* ticks, int n) {
  const int l = threadIdx.x & 63;
  double v[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) v[i] = slot_live<MODE>(l) ? 1.0 + 0.001 * base_lane<MODE>(l) + 0.01 * i : 0.0;
  double upd = slot_live<MODE>(l) ? 1e-3 * (base_lane<MODE>(l) >> 3) : 0.0;
  double scale = slot_live<MODE>(l) ? (MODE == ADD90 ? 0.1 : 0.125) : 0.0;
  asm volatile("" : "+v"(scale), "+v"(upd));  // a register in every variant: the update is one v_fma_f64 per value
  const long long t0 = clock64();
  for (int it = 0; it < n; ++it) {
    if (MODE == ADD90) {
      double a[10];
#pragma unroll
      for (int i = 0; i < 10; ++i) a[i] = v[i];
#pragma unroll
      for (int r = 0; r < 9; ++r)
#pragma unroll
        for (int i = 0; i < 10; ++i) {
          a[i] += v[(i + r) % 10];
          asm volatile("" : "+v"(a[i]));
        }
#pragma unroll
      for (int i = 0; i < 10; ++i) v[i] = a[i];
    } else {
      sum10<MODE>(v);
    }
    // the next pass depends on this one's sums, the values stay bounded and a group's lanes agree
#pragma unroll
    // (an empty slot holds the row's sum after the broadcast; its factor and offset are zero)
    for (int i = 0; i < 10; ++i) v[i] = v[i] * scale + upd;
  }
  const long long t1 = clock64();
#pragma unroll
  for (int i = 0; i < 10; ++i) out[(size_t)(MODE == ROWB ? l : base_lane<MODE>(l)) * 10 + i + (threadIdx.x >> 6) * 640] = v[i];
  if (l == 0) ticks[threadIdx.x >> 6] = t1 - t0;
}

template <int MODE>
static double run(const char* name, int n, double* host) {
  double* o;
  long long *c, h[4];
  CK(hipMalloc(&o, 4 * 640 * sizeof(double)));
  CK(hipMalloc(&c, sizeof(h)));
  for (int r = 0; r < 3; ++r) hipLaunchKernelGGL(k<MODE>, dim3(1), dim3(256), 0, 0, o, c, n);
  CK(hipMemcpy(h, c, sizeof(h), hipMemcpyDeviceToHost));
  CK(hipMemcpy(host, o, 640 * sizeof(double), hipMemcpyDeviceToHost));
  CK(hipFree(o));
  CK(hipFree(c));
  long long m = h[0];
  for (int w = 1; w < 4; ++w) m = h[w] > m ? h[w] : m;
  const double per = (double)m / n;
  if (name) printf("%-6s %8.1f ticks per pass (slowest of 4 waves, %d passes)\n", name, per, n);
  return per;
}

static void check(const char* name, const double* ref, const double* got) {
  double worst = 0.0;
  bool same = true;
  for (int l = 0; l < 64; ++l)
    for (int i = 0; i < 10; ++i) {
      worst = std::fmax(worst, std::fabs(got[l * 10 + i] - ref[l * 10 + i]) / std::fabs(ref[l * 10 + i]));
      same = same && std::memcmp(&got[l * 10 + i], &got[(l & ~7) * 10 + i], sizeof(double)) == 0;
    }
  printf("%-6s after one pass: max relative difference to base %.2e (%s), lanes of a group %s\n", name, worst,
         worst < 1e-14 ? "ok" : "WRONG", same ? "bit-identical" : "DIFFER");
}

// (c): every lane of row r must hold ((v0 + v1) + (v2 + v3)) + (v4 + v5) of its six live slots, the
// butterfly's own tree; checked against the host's evaluation of the same formula
static void check_row(const double* got) {
  double worst = 0.0;
  bool same = true;
  for (int r = 0; r < 4; ++r)
    for (int i = 0; i < 10; ++i) {
      double x[6];
      for (int k = 0; k < 6; ++k) x[k] = 1.0 + 0.001 * (8 * r + k) + 0.01 * i;
      const double want = (((x[0] + x[1]) + (x[2] + x[3])) + (x[4] + x[5])) * 0.125 + 1e-3 * r;
      for (int l = 0; l < 6; ++l) {
        const double g = got[(16 * r + l) * 10 + i];
        worst = std::fmax(worst, std::fabs(g - want) / std::fabs(want));
        same = same && std::memcmp(&g, &got[(16 * r) * 10 + i], sizeof(double)) == 0;
      }
    }
  printf("%-6s after one pass: max relative difference to the host's sums %.2e (%s), live lanes of a row %s\n", "row",
         worst, worst < 1e-14 ? "ok" : "WRONG", same ? "bit-identical" : "DIFFER");
}

int main() {
  static double ref[640], got[640];
  run<BASE>(nullptr, 1, ref);
  run<STAGE>(nullptr, 1, got);
  check("stage", ref, got);
  run<ROWB>(nullptr, 1, got);
  check_row(got);
  run<MFMA>(nullptr, 1, got);
  check("mfma", ref, got);
  run<HALF>(nullptr, 1, got);
  check("half", ref, got);
  const int n = 4096;
  for (int rep = 0; rep < 3; ++rep) {
    const double b = run<BASE>("base", n, got);
    const double m = run<MFMA>("mfma", n, got);
    const double h = run<HALF>("half", n, got);
    const double a = run<ADD90>("add90", n, got);
    const double st = run<STAGE>("stage", n, got);
    const double rw = run<ROWB>("row", n, got);
    printf("relative to base: mfma %.3f, half %.3f, add90 %.3f, stage %.3f, row %.3f; row / stage %.3f\n", m / b, h / b,
           a / b, st / b, rw / b, rw / st);
  }
  return 0;
}
