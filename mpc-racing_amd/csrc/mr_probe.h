// TEST-ONLY probe bodies for the wave primitives (mr_wave_prims.h) and pick6 (mr_wave.h).
//
// The bodies are written against Wv, as the solver is, and are compiled twice: by hipcc into
// libmpcracing_probe.so (mr_probe.hip, the product's code-generation flags) and by g++ into the host
// twin, where they run under host_wave_run.  Each applies every primitive to the lane's inputs and
// stores the lane's results, one 64-word slot per result, so a test can compare the two builds with
// each other and with a restatement of the primitives (tests/wave_prims_ref.py).
//
// Not part of the C ABI: nothing here is declared in include/mpcracing.h.
#pragma once
#include <type_traits>
#include "mr_wave.h"

namespace mr {
namespace probe {

// ---- layout of the primitive probe (words of T per workgroup) ----
// in:  [0, 64) the lane values v; [64 + 64 j, 128 + 64 j) the pick6 / wtranspose4 arguments a_j, j < 6
constexpr int PRIMS_IN_W = 7 * WL;
// out: slot s occupies [64 s, 64 s + 64)
enum PrimSlot {
  PS_SHFL_CONST = 0,  // wshfl(v, 37)
  PS_SHFL_UNI,        // wshfl(v, u), u wave-uniform at run time: (number of the workgroup * 5 + 11) & 63
  PS_SHFL_LANE,       // wshfl(v, (7 lane + 3) & 63)
  PS_SHFL_REV,        // wshfl(v, 63 - lane)
  PS_XOR,             // 32 slots: wxor(v, m), m = 1 .. 32
  PS_NEXT = PS_XOR + 32,
  PS_PREV,
  PS_ROW_NEXT,
  PS_BCAST,           // 6 slots: wbcast(v, s), s = 0, 15, 16, 31, 32, 63
  PS_GATHER = PS_BCAST + 6,  // 6 slots: wgather<T, 6>
  PS_SUM = PS_GATHER + 6,
  PS_MAX,
  PS_MIN,
  PS_ANY_NEG,         // wany(v < 0)
  PS_ALL_NEG,         // wall(v < 0)
  PS_ALL_ORD,         // wall(v == v)
  PS_ANY_BIG,         // wany(v > a_0)
  PS_UNI,             // wuni(wshfl(v, 3) > 0)
  PS_WU,              // wu(wshfl(v, 9))
  PS_TRANSPOSE,       // 4 slots: wtranspose4 of (a_0 .. a_3)
  PS_BUF_LD = PS_TRANSPOSE + 4,  // WBuf::ld at a non-zero uniform offset and lane offset (5 lane + 2) & 63
  PS_BUF_ST,          // v stored through WBuf::st at lane offset (11 lane + 7) & 63
  PS_PICK6,           // pick6(lane, a_0 .. a_5)
  PS_PICK6_MOD,       // pick6(lane & 7, a_0 .. a_5)
  PS_COUNT
};
constexpr int PRIMS_OUT_W = PS_COUNT * WL;

// ---- layout of the MFMA probe (words of T per workgroup) ----
// A: [0, 64) the lane's a of the first product; [64 + 64 s, 128 + 64 s) the lane's a of k-block s of the second
// B: [0, 64) the lane's b;  C: register v of the lane at [64 v, 64 v + 64)
// D: [0, 256) registers of C + A B; [256, 512) registers of A2 (A B), accumulated from zero over the four
//    k-blocks with the first product's registers (f32: after wtranspose4) as B fragments, as the Riccati sweep does
constexpr int MFMA_A_W = 5 * WL, MFMA_B_W = WL, MFMA_C_W = 4 * WL, MFMA_D_W = 8 * WL;

template <typename T>
MR_HD T from_bool(bool b) { return b ? T(1) : T(0); }

template <typename T>
#if MR_DEVICE_BUILD
__device__ __forceinline__
#else
inline
#endif
void prims_body(const Wv& w, int wg, int n_wg, MR_GLOBAL T* in_all, MR_GLOBAL T* out_all) {
  const int l = w.lane;
  MR_GLOBAL const T* in = in_all + (int64_t)wg * PRIMS_IN_W;
  MR_GLOBAL T* out = out_all + (int64_t)wg * PRIMS_OUT_W;
  const T v = in[l];
  T a[6];
  for (int j = 0; j < 6; ++j) a[j] = in[WL + WL * j + l];
  auto put = [&](int slot, T x) { out[slot * WL + l] = x; };

  put(PS_SHFL_CONST, wshfl(w, v, 37));
  put(PS_SHFL_UNI, wshfl(w, v, (wg * 5 + 11) & 63));
  put(PS_SHFL_LANE, wshfl(w, v, (7 * l + 3) & 63));
  put(PS_SHFL_REV, wshfl(w, v, 63 - l));
#if MR_DEVICE_BUILD
#pragma unroll
#endif
  for (int m = 1; m <= 32; ++m) put(PS_XOR + m - 1, wxor(w, v, m));
  put(PS_BCAST + 0, wbcast(w, v, 0));
  put(PS_BCAST + 1, wbcast(w, v, 15));
  put(PS_BCAST + 2, wbcast(w, v, 16));
  put(PS_BCAST + 3, wbcast(w, v, 31));
  put(PS_BCAST + 4, wbcast(w, v, 32));
  put(PS_BCAST + 5, wbcast(w, v, 63));
  T g[6];
  wgather<T, 6>(w, v, g);
  for (int j = 0; j < 6; ++j) put(PS_GATHER + j, g[j]);
  put(PS_SUM, wsum(w, v));
  put(PS_MAX, wmax(w, v));
  put(PS_MIN, wmin(w, v));
  put(PS_ANY_NEG, from_bool<T>(wany(w, v < T(0))));
  put(PS_ALL_NEG, from_bool<T>(wall(w, v < T(0))));
  put(PS_ALL_ORD, from_bool<T>(wall(w, v == v)));
  put(PS_ANY_BIG, from_bool<T>(wany(w, v > a[0])));
  put(PS_UNI, from_bool<T>(wuni(w, wshfl(w, v, 3) > T(0))));
  put(PS_WU, wu(w, wshfl(w, v, 9)));
  put(PS_PICK6, pick6(l, a[0], a[1], a[2], a[3], a[4], a[5]));
  put(PS_PICK6_MOD, pick6(l & 7, a[0], a[1], a[2], a[3], a[4], a[5]));
  if constexpr (!std::is_same<T, int>::value) {  // the DPP rotates and the buffer accessors carry floating types only
    put(PS_NEXT, wnext(w, v));
    put(PS_PREV, wprev(w, v));
    put(PS_ROW_NEXT, wrow_next(w, v));
    const WBuf<T> bi((MR_GLOBAL T*)in_all, (unsigned)n_wg * PRIMS_IN_W), bo(out_all, (unsigned)n_wg * PRIMS_OUT_W);
    put(PS_BUF_LD, bi.ld((unsigned)wg * PRIMS_IN_W + 2 * WL, (unsigned)((5 * l + 2) & 63)));
    bo.st(v, (unsigned)wg * PRIMS_OUT_W + PS_BUF_ST * WL, (unsigned)((11 * l + 7) & 63));
  }
  if constexpr (std::is_same<T, float>::value) {  // the device has wtranspose4 for f32 only (f64 needs none)
    T d[4] = {a[0], a[1], a[2], a[3]};
    wtranspose4(w, d);
    for (int s = 0; s < 4; ++s) put(PS_TRANSPOSE + s, d[s]);
  }
}

template <typename T>
#if MR_DEVICE_BUILD
__device__ __forceinline__
#else
inline
#endif
void mfma_body(const Wv& w, int wg, MR_GLOBAL const T* A, MR_GLOBAL const T* B, MR_GLOBAL const T* C, MR_GLOBAL T* D) {
  const int l = w.lane;
  A += (int64_t)wg * MFMA_A_W; B += (int64_t)wg * MFMA_B_W; C += (int64_t)wg * MFMA_C_W; D += (int64_t)wg * MFMA_D_W;
  T d[4], z[4] = {T(0), T(0), T(0), T(0)};
  for (int v = 0; v < 4; ++v) d[v] = C[WL * v + l];
  wmfma(w, A[l], B[l], d);
  for (int v = 0; v < 4; ++v) D[WL * v + l] = d[v];
  for (int v = 0; v < 4; ++v) d[v] = z[v];
  wmfma(w, A[l], B[l], d);  // A B alone: the B fragments of the second product
  if constexpr (sizeof(T) == 4) wtranspose4(w, d);
  T q[4] = {T(0), T(0), T(0), T(0)};
  for (int s = 0; s < 4; ++s) wmfma(w, A[WL + WL * s + l], d[s], q);
  for (int v = 0; v < 4; ++v) D[4 * WL + WL * v + l] = q[v];
}

}  // namespace probe
}  // namespace mr
