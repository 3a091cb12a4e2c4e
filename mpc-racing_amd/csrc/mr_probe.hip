// libmpcracing_probe.so -- TEST-ONLY entry points to the device-only code of the fp32 solve.
//
// The fp32 scalar functions of mr_common.h, Dyn<float, MODEL>, the 3 x 3 pivots and the wave
// primitives exist in this form only in the gfx950 build.  This library calls them from small kernels
// of its own, compiled with exactly the code-generation flags of libmpcracing.so (mpcracing/build.py
// keeps one flag list for both), so that tests can compare each piece with a plain reference
// (tests/test_gpu_f32_math.py, test_gpu_f32_dynamics.py, test_gpu_wave_prims.py).
//
// What this pins: the functions as the compiler builds them with the product's flags.  Inlined into
// mr_wave_kernel the compiler may contract or schedule the same source differently; the fp32 solve
// tests (tests/test_gpu.py) remain the check of the kernel as a whole.
//
// The product's headers are included unchanged.  Nothing here belongs to the C ABI
// (include/mpcracing.h); the symbols are mrp_*, bound by mpcracing.abi.load_probe().
// Every kernel guards its index, and every entry point checks on the host that each pointer lies in
// a device allocation large enough for what the kernel will touch, before anything is launched.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string>

#include "mr_probe.h"

using namespace mr;
using namespace mr::probe;

static thread_local std::string g_err;

static int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

// ptr .. ptr + bytes lies inside one device allocation (bytes == 0: ptr only needs to be non-null)
static bool in_device_range(const void* ptr, size_t bytes) {
  if (!ptr) return false;
  if (bytes == 0) return true;
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)ptr) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  const char* b = (const char*)base;
  const char* p = (const char*)ptr;
  return p >= b && bytes <= size && (size_t)(p - b) <= size - bytes;
}
#define MRP_RANGE(ptr, bytes)                                                                              \
  do {                                                                                                     \
    if (!in_device_range((ptr), (size_t)(bytes)))                                                          \
      return fail(MR_ERR_ARG, std::string(#ptr) + ": not a device buffer of at least " + std::to_string((size_t)(bytes)) + " bytes"); \
  } while (0)
#define MRP_LAUNCHED()                                                                     \
  do {                                                                                     \
    hipError_t e_ = hipGetLastError();                                                     \
    if (e_ != hipSuccess) return fail(MR_ERR_HIP, std::string("launch: ") + hipGetErrorString(e_)); \
  } while (0)

constexpr int kMaxN = 1 << 24;   // elements of a per-lane probe
constexpr int kMaxWG = 1 << 12;  // workgroups of a wave probe

// ---- fp32 scalar functions: one lane per element ----
enum MathOp { OP_SIN = 0, OP_COS, OP_TAN, OP_ATAN, OP_ATAN2, OP_SQRT, OP_EXP, OP_LOG, OP_RSQRT, OP_DIV, OP_RCP, OP_COUNT };

__global__ __launch_bounds__(256) void mrp_math_kernel(int op, int n, const float* a, const float* b, float* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float x = a[i];
  const float y = b ? b[i] : 0.0f;
  float r;
  switch (op) {
    case OP_SIN: r = mr_sin(x); break;
    case OP_COS: r = mr_cos(x); break;
    case OP_TAN: r = mr_tan(x); break;
    case OP_ATAN: r = mr_atan(x); break;
    case OP_ATAN2: r = mr_atan2(x, y); break;
    case OP_SQRT: r = mr_sqrt(x); break;
    case OP_EXP: r = mr_exp(x); break;
    case OP_LOG: r = mr_log(x); break;
    case OP_RSQRT: r = mr_rsqrt(x); break;
    case OP_DIV: r = x / y; break;
    default: r = 1.0f / x; break;
  }
  out[i] = r;
}

// ---- Dyn<float, MODEL> ----
template <int MODEL>
__global__ __launch_bounds__(64) void mrp_dyn_kernel(ProbParams<float> P, int n, const float* x, const float* u,
                                                     const float* nu, float* f, float* J, float* H) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  if (J == nullptr)
    Dyn<float, MODEL>::f(P, x + 6 * i, u + 2 * i, f + 6 * i);
  else
    Dyn<float, MODEL>::fjh(P, x + 6 * i, u + 2 * i, nu + 6 * i, f + 6 * i, J + 48 * i, H + 36 * i);
}

// ---- chol3r + lsolve3r + ltsolve3r ----
__global__ __launch_bounds__(64) void mrp_chol3_kernel(int n, const float* R, const float* b, int32_t* ok, float* L,
                                                       float* iv, float* x) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  float Rl[6], Ll[6], ivl[3], xl[3];
  for (int j = 0; j < 6; ++j) Rl[j] = R[6 * i + j];
  for (int j = 0; j < 3; ++j) xl[j] = b[3 * i + j];
  const bool good = chol3r(Rl, Ll, ivl);
  lsolve3r(Ll, ivl, xl);
  ltsolve3r(Ll, ivl, xl);
  ok[i] = good ? 1 : 0;
  for (int j = 0; j < 6; ++j) L[6 * i + j] = Ll[j];
  for (int j = 0; j < 3; ++j) { iv[3 * i + j] = ivl[j]; x[3 * i + j] = xl[j]; }
}

// ---- wave primitives: one 64-lane workgroup per block, as mr_wave_kernel is launched ----
template <typename T>
__global__ __launch_bounds__(WL) void mrp_prims_kernel(int n_wg, T* in, T* out) {
  const int wg = (int)blockIdx.x;
  if (wg >= n_wg) return;  // block-uniform
  Wv w{(int)threadIdx.x};
  prims_body<T>(w, wg, n_wg, (MR_GLOBAL T*)in, (MR_GLOBAL T*)out);
}
template <typename T>
__global__ __launch_bounds__(WL) void mrp_mfma_kernel(int n_wg, const T* A, const T* B, const T* C, T* D) {
  const int wg = (int)blockIdx.x;
  if (wg >= n_wg) return;  // block-uniform
  Wv w{(int)threadIdx.x};
  mfma_body<T>(w, wg, (MR_GLOBAL const T*)A, (MR_GLOBAL const T*)B, (MR_GLOBAL const T*)C, (MR_GLOBAL T*)D);
}

template <typename T>
static int run_prims(int n_wg, T* in, T* out, void* hip_stream) {
  if (n_wg < 1 || n_wg > kMaxWG) return fail(MR_ERR_ARG, "n_wg out of range");
  MRP_RANGE(in, sizeof(T) * (size_t)n_wg * PRIMS_IN_W);
  MRP_RANGE(out, sizeof(T) * (size_t)n_wg * PRIMS_OUT_W);
  hipLaunchKernelGGL(mrp_prims_kernel<T>, dim3(n_wg), dim3(WL), 0, (hipStream_t)hip_stream, n_wg, in, out);
  MRP_LAUNCHED();
  return MR_OK;
}
template <typename T>
static int run_mfma(int n_wg, const T* A, const T* B, const T* C, T* D, void* hip_stream) {
  if (n_wg < 1 || n_wg > kMaxWG) return fail(MR_ERR_ARG, "n_wg out of range");
  MRP_RANGE(A, sizeof(T) * (size_t)n_wg * MFMA_A_W);
  MRP_RANGE(B, sizeof(T) * (size_t)n_wg * MFMA_B_W);
  MRP_RANGE(C, sizeof(T) * (size_t)n_wg * MFMA_C_W);
  MRP_RANGE(D, sizeof(T) * (size_t)n_wg * MFMA_D_W);
  hipLaunchKernelGGL(mrp_mfma_kernel<T>, dim3(n_wg), dim3(WL), 0, (hipStream_t)hip_stream, n_wg, A, B, C, D);
  MRP_LAUNCHED();
  return MR_OK;
}

extern "C" {

const char* mrp_last_error(void) { return g_err.c_str(); }

// the word counts per workgroup of the wave probes (mr_probe.h), for the binding to size its buffers
void mrp_layout(int32_t* out8) {
  out8[0] = PRIMS_IN_W; out8[1] = PRIMS_OUT_W; out8[2] = MFMA_A_W; out8[3] = MFMA_B_W; out8[4] = MFMA_C_W;
  out8[5] = MFMA_D_W; out8[6] = PS_COUNT; out8[7] = OP_COUNT;
}

int mrp_math_f32(int32_t op, int32_t n, const float* a, const float* b, float* out, void* hip_stream) {
  if (op < 0 || op >= OP_COUNT) return fail(MR_ERR_ARG, "unknown op");
  if (n < 1 || n > kMaxN) return fail(MR_ERR_ARG, "n out of range");
  const bool two = op == OP_ATAN2 || op == OP_DIV;
  MRP_RANGE(a, sizeof(float) * (size_t)n);
  if (two) MRP_RANGE(b, sizeof(float) * (size_t)n);
  MRP_RANGE(out, sizeof(float) * (size_t)n);
  hipLaunchKernelGGL(mrp_math_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)hip_stream, op, n, a,
                     two ? b : nullptr, out);
  MRP_LAUNCHED();
  return MR_OK;
}

// ProbParams<float> as mr_create / mr_set_tyres build them: fill_params<float> of the configuration and the fp64
// pacejka_coef constants (a_front / a_back NULL: no tyres set, zero coefficients as in a fresh handle)
int mrp_eval_dynamics_f32(const mr_config* cfg, const double* a_front, double Fz_front, const double* a_back,
                          double Fz_back, int32_t n, const float* x, const float* u, const float* nu, float* f,
                          float* J, float* H, void* hip_stream) {
  if (!cfg) return fail(MR_ERR_ARG, "null config");
  if (n < 1 || n > kMaxN) return fail(MR_ERR_ARG, "n out of range");
  if ((J == nullptr) != (H == nullptr)) return fail(MR_ERR_ARG, "J and H go together");
  MRP_RANGE(x, sizeof(float) * 6 * (size_t)n);
  MRP_RANGE(u, sizeof(float) * 2 * (size_t)n);
  MRP_RANGE(f, sizeof(float) * 6 * (size_t)n);
  if (J) {
    MRP_RANGE(nu, sizeof(float) * 6 * (size_t)n);
    MRP_RANGE(J, sizeof(float) * 48 * (size_t)n);
    MRP_RANGE(H, sizeof(float) * 36 * (size_t)n);
  }
  TyreCoef<double> tf{}, tr{};
  if (a_front) tf = pacejka_coef(a_front, Fz_front);
  if (a_back) tr = pacejka_coef(a_back, Fz_back);
  ProbParams<float> P;
  fill_params<float>(*cfg, tf, tr, P);
  hipStream_t st = (hipStream_t)hip_stream;
  dim3 grid((n + 63) / 64), block(64);
  switch (cfg->model) {
    case MR_MODEL_KINEMATIC: hipLaunchKernelGGL(mrp_dyn_kernel<MODEL_KIN>, grid, block, 0, st, P, n, x, u, nu, f, J, H); break;
    case MR_MODEL_DYNAMIC: hipLaunchKernelGGL(mrp_dyn_kernel<MODEL_DYN>, grid, block, 0, st, P, n, x, u, nu, f, J, H); break;
    case MR_MODEL_BLENDED: hipLaunchKernelGGL(mrp_dyn_kernel<MODEL_BLEND>, grid, block, 0, st, P, n, x, u, nu, f, J, H); break;
    case MR_MODEL_BLENDED_PACEJKA: hipLaunchKernelGGL(mrp_dyn_kernel<MODEL_BLEND_PACEJKA>, grid, block, 0, st, P, n, x, u, nu, f, J, H); break;
    case MR_MODEL_DYNAMIC_PACEJKA: hipLaunchKernelGGL(mrp_dyn_kernel<MODEL_DYN_PACEJKA>, grid, block, 0, st, P, n, x, u, nu, f, J, H); break;
    default: return fail(MR_ERR_ARG, "unknown model");
  }
  MRP_LAUNCHED();
  return MR_OK;
}

int mrp_chol3_f32(int32_t n, const float* R, const float* b, int32_t* ok, float* L, float* iv, float* x,
                  void* hip_stream) {
  if (n < 1 || n > kMaxN) return fail(MR_ERR_ARG, "n out of range");
  MRP_RANGE(R, sizeof(float) * 6 * (size_t)n);
  MRP_RANGE(b, sizeof(float) * 3 * (size_t)n);
  MRP_RANGE(ok, sizeof(int32_t) * (size_t)n);
  MRP_RANGE(L, sizeof(float) * 6 * (size_t)n);
  MRP_RANGE(iv, sizeof(float) * 3 * (size_t)n);
  MRP_RANGE(x, sizeof(float) * 3 * (size_t)n);
  hipLaunchKernelGGL(mrp_chol3_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)hip_stream, n, R, b, ok, L, iv, x);
  MRP_LAUNCHED();
  return MR_OK;
}

int mrp_wave_prims_f32(int32_t n_wg, float* in, float* out, void* s) { return run_prims<float>(n_wg, in, out, s); }
int mrp_wave_prims_f64(int32_t n_wg, double* in, double* out, void* s) { return run_prims<double>(n_wg, in, out, s); }
int mrp_wave_prims_i32(int32_t n_wg, int32_t* in, int32_t* out, void* s) { return run_prims<int>(n_wg, in, out, s); }
int mrp_wave_mfma_f32(int32_t n_wg, const float* A, const float* B, const float* C, float* D, void* s) {
  return run_mfma<float>(n_wg, A, B, C, D, s);
}
int mrp_wave_mfma_f64(int32_t n_wg, const double* A, const double* B, const double* C, double* D, void* s) {
  return run_mfma<double>(n_wg, A, B, C, D, s);
}

}  // extern "C"
