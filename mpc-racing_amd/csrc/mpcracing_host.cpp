// Host (g++) build of the solver core -- TEST HARNESS ONLY.
//
// libmpcracing_host.so runs the very same per-instance solver source as the
// gfx950 kernel (mr_wave.h), each instance as an emulated 64-lane wavefront, so that the solver logic can be checked
// against the oracle in the CPU test suite (no GPU in the build container).
// The product path (mpc-racing_amd/control/MPC.py, mpcracing.batch) never
// loads this library; it requires libmpcracing.so and a GPU.
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "mr_wave.h"
#include "mr_track.h"
#include "mr_agent.h"
#include "mr_plant.h"
#include "mr_tyrefit.h"
#include "mr_rollout.h"
#include "mr_plantroll.h"
#include "mr_pid.h"
#include "mr_ga.h"
#include "mr_probe.h"
#include "mr_warm.h"
#include "mr_mpcseg.h"

using namespace mr;

// Each instance runs as one emulated wavefront (64 fibers, mr_wave_prims.h host_wave_call) on one CPU thread.
template <typename T, int MODEL>
static void run(const mr_config& c, const TyreCoef<double>& tf, const TyreCoef<double>& tr, int B,
                const mr_inputs& in, const mr_outputs& out, const int32_t* horizon, const mr_warm* warm, int nthreads) {
  ProbParams<T> P;
  fill_params<T>(c, tf, tr, P);
  const mr_warm wm = warm ? *warm : mr_warm{nullptr, nullptr, nullptr, nullptr};
#pragma omp parallel for schedule(dynamic, 1) num_threads(nthreads > 0 ? nthreads : 1)
  for (int i = 0; i < B; ++i) {
    // the instance's horizon (mr_wave_kernel): out of range = not solved
    const int Ni = instance_horizon(horizon, i, P.N);
    if (!horizon_ok(Ni, P.N)) {
      nan_unreached(out, B, i, P.N, -1, 0, 1);
      if (wm.used) wm.used[i] = 0;
      continue;
    }
    // poisoned workspace / LDS: any read-before-write shows up as NaN (device memory is not zeroed)
    std::vector<T> ws((size_t)ws_words<T>(), (T)NAN), lds((size_t)LDS_WORDS, (T)NAN);
    host_wave_call([&](const Wv& w) {
      solve_instance_wave<T, MODEL>(P, in, out, (int64_t)B, (int64_t)i, ws.data(), lds.data(), w, nullptr, nullptr,
                                    nullptr, nullptr, Ni, wm);
    });
    if (Ni != P.N) nan_unreached(out, B, i, P.N, Ni, 0, 1);  // (the kernel's lanes share the rows)
  }
}

// The scalar C++ solver (mr_solver.h Solver: the same IPM, one instance per CPU thread, no wave
// emulation) over a batch with OpenMP -- the CPU baseline that bench.py times beside the GPU
// (SURVEY §8(d) "C++ fp64 CPU SQP twin").  Per-thread workspace of (N+1) stage records.
template <typename T, int MODEL>
static void run_scalar(const mr_config& c, const TyreCoef<double>& tf, const TyreCoef<double>& tr, int B,
                       const mr_inputs& in, const mr_outputs& out, const int32_t* horizon, const mr_warm* warm,
                       int nthreads) {
  ProbParams<T> P;
  fill_params<T>(c, tf, tr, P);
#pragma omp parallel num_threads(nthreads > 0 ? nthreads : 1)
  {
    std::vector<T> ws((size_t)(c.N + 1) * WF::NF, (T)NAN);
#pragma omp for schedule(dynamic, 1)
    for (int i = 0; i < B; ++i) {
      const int Ni = instance_horizon(horizon, i, P.N);
      if (horizon_ok(Ni, P.N)) solve_instance<T, MODEL>(P, in, out, (int64_t)B, (int64_t)i, WS<T>{ws.data(), 1}, Ni, warm);
      else {
        nan_unreached(out, B, i, P.N, -1, 0, 1);
        if (warm && warm->used) warm->used[i] = 0;
      }
    }
  }
}

// The host side of every rollout (mr_rollout.h): the test of the starts' range, and the driver -- one emulated
// wavefront per (set, chunk) running chunk(A, p, chunk, lds, w), the partials added in chunk order.
static const char* rollout_starts_check(const RoArgs& A) {
  for (int k = 0; k < A.n_start; ++k)
    if (A.start[k] < 0 || A.start[k] > A.T - 1 - A.H) return "start entry out of range [0, T - 1 - H]";
  return nullptr;
}
template <class Chunk>
static void rollout_host(RoArgs A, int P, double* stats, int32_t* count, int nthreads, Chunk&& chunk) {
  std::vector<double> partials((size_t)P * A.n_chunk * A.H * RO_NPART, NAN);
  A.partials = partials.data();
  const int64_t jobs = (int64_t)P * A.n_chunk;
#pragma omp parallel for schedule(dynamic, 1) num_threads(nthreads > 0 ? nthreads : 1)
  for (int64_t b = 0; b < jobs; ++b) {
    std::vector<double> lds((size_t)RO_LDS_WORDS, NAN);
    host_wave_call([&](const Wv& w) { chunk(A, (int)(b / A.n_chunk), (int)(b % A.n_chunk), lds.data(), w); });
  }
  for (int p = 0; p < P; ++p)
    for (int k = 0; k < A.H; ++k) ro_finish(A.H, A.n_chunk, partials.data(), p, p, k, stats, count);
}

extern "C" {

int mrh_config_default(mr_config* c) {
  fill_default_config(c);
  return 0;
}

// horizon: host int32 [B] or NULL; warm: host arrays or NULL (include/mpcracing.h mr_solve_batch_warm)
int mrh_solve_batch_warm(const mr_config* c, const double* a_front, double Fz_front, const double* a_back,
                         double Fz_back, int B, const mr_inputs* in, mr_outputs* out, const int32_t* horizon,
                         const mr_warm* warm, int nthreads) {
  if (warm && (!warm->x_init || !warm->s_init)) return -1;
  TyreCoef<double> tf{}, tr{};
  if (a_front) tf = pacejka_coef(a_front, Fz_front);
  if (a_back) tr = pacejka_coef(a_back, Fz_back);
  if (c->max_iter < 0 || c->max_iter > FCAP - 2) return -1;  // the line-search filter's capacity (mr_create)
#define MR_CASE(T, M) run<T, M>(*c, tf, tr, B, *in, *out, horizon, warm, nthreads)
#define MR_MODELS(T)                                                       \
  switch (c->model) {                                                      \
    case MR_MODEL_KINEMATIC: MR_CASE(T, MODEL_KIN); break;                 \
    case MR_MODEL_DYNAMIC: MR_CASE(T, MODEL_DYN); break;                   \
    case MR_MODEL_BLENDED: MR_CASE(T, MODEL_BLEND); break;                 \
    case MR_MODEL_BLENDED_PACEJKA: MR_CASE(T, MODEL_BLEND_PACEJKA); break; \
    case MR_MODEL_DYNAMIC_PACEJKA: MR_CASE(T, MODEL_DYN_PACEJKA); break;   \
    default: return -1;                                                    \
  }
  if (c->precision == MR_PREC_FP64) { MR_MODELS(double) } else { MR_MODELS(float) }
#undef MR_CASE
  return 0;
}
int mrh_solve_batch_horizons(const mr_config* c, const double* a_front, double Fz_front, const double* a_back,
                             double Fz_back, int B, const mr_inputs* in, mr_outputs* out, const int32_t* horizon,
                             int nthreads) {
  return mrh_solve_batch_warm(c, a_front, Fz_front, a_back, Fz_back, B, in, out, horizon, nullptr, nthreads);
}
int mrh_solve_batch(const mr_config* c, const double* a_front, double Fz_front, const double* a_back,
                    double Fz_back, int B, const mr_inputs* in, mr_outputs* out, int nthreads) {
  return mrh_solve_batch_horizons(c, a_front, Fz_front, a_back, Fz_back, B, in, out, nullptr, nthreads);
}

int mrh_solve_batch_scalar_warm(const mr_config* c, const double* a_front, double Fz_front, const double* a_back,
                                double Fz_back, int B, const mr_inputs* in, mr_outputs* out, const int32_t* horizon,
                                const mr_warm* warm, int nthreads) {
  if (warm && (!warm->x_init || !warm->s_init)) return -1;
  TyreCoef<double> tf{}, tr{};
  if (a_front) tf = pacejka_coef(a_front, Fz_front);
  if (a_back) tr = pacejka_coef(a_back, Fz_back);
  if (c->N < 1 || c->N > 63) return -1;
  if (c->max_iter < 0 || c->max_iter > FCAP - 2) return -1;
#define MR_CASE(T, M) run_scalar<T, M>(*c, tf, tr, B, *in, *out, horizon, warm, nthreads)
  if (c->precision == MR_PREC_FP64) { MR_MODELS(double) } else { MR_MODELS(float) }
#undef MR_CASE
  return 0;
}
int mrh_solve_batch_scalar_horizons(const mr_config* c, const double* a_front, double Fz_front, const double* a_back,
                                    double Fz_back, int B, const mr_inputs* in, mr_outputs* out,
                                    const int32_t* horizon, int nthreads) {
  return mrh_solve_batch_scalar_warm(c, a_front, Fz_front, a_back, Fz_back, B, in, out, horizon, nullptr, nthreads);
}
// mr_warm_shift on host arrays (mr_warm.h): the kernel's function, one instance after the other
int mrh_warm_shift(const mr_config* c, const double* a_front, double Fz_front, const double* a_back, double Fz_back,
                   int B, const double* X_prev, const double* U_prev, const double* S_prev, const int32_t* status_prev,
                   const int32_t* horizon_prev, const double* state0_new, const double* s0_new,
                   const int32_t* horizon_new, double* u_init, double* x_init, double* s_init, int32_t* use) {
  if (!c || c->model < 0 || c->model > 4 || c->N < 1 || c->N > 63 || B < 0) return -1;
  if (!X_prev || !U_prev || !S_prev || !status_prev || !state0_new || !s0_new || !u_init || !x_init || !s_init || !use)
    return -1;
  TyreCoef<double> tf{}, tr{};
  if (a_front) tf = pacejka_coef(a_front, Fz_front);
  if (a_back) tr = pacejka_coef(a_back, Fz_back);
  ProbParams<double> P;
  fill_params<double>(*c, tf, tr, P);
  const WarmShiftArgs A{B, c->N, X_prev, U_prev, S_prev, status_prev, horizon_prev, state0_new, s0_new, horizon_new,
                        u_init, x_init, s_init, use};
  for (int i = 0; i < B; ++i) warm_shift_dispatch(c->model, P, A, i);
  return 0;
}
int mrh_solve_batch_scalar(const mr_config* c, const double* a_front, double Fz_front, const double* a_back,
                           double Fz_back, int B, const mr_inputs* in, mr_outputs* out, int nthreads) {
  return mrh_solve_batch_scalar_horizons(c, a_front, Fz_front, a_back, Fz_back, B, in, out, nullptr, nthreads);
}

// Generated dynamics (value, Jacobian, nu-weighted Hessian) at one point, fp64.
int mrh_eval_dynamics(const mr_config* c, const double* a_front, double Fz_front, const double* a_back,
                      double Fz_back, const double* x, const double* u, const double* nu, double* f, double* J,
                      double* H) {
  TyreCoef<double> tf{}, tr{};
  if (a_front) tf = pacejka_coef(a_front, Fz_front);
  if (a_back) tr = pacejka_coef(a_back, Fz_back);
  ProbParams<double> P;
  fill_params<double>(*c, tf, tr, P);
  switch (c->model) {
    case MR_MODEL_KINEMATIC: Dyn<double, MODEL_KIN>::fjh(P, x, u, nu, f, J, H); break;
    case MR_MODEL_DYNAMIC: Dyn<double, MODEL_DYN>::fjh(P, x, u, nu, f, J, H); break;
    case MR_MODEL_BLENDED: Dyn<double, MODEL_BLEND>::fjh(P, x, u, nu, f, J, H); break;
    case MR_MODEL_BLENDED_PACEJKA: Dyn<double, MODEL_BLEND_PACEJKA>::fjh(P, x, u, nu, f, J, H); break;
    case MR_MODEL_DYNAMIC_PACEJKA: Dyn<double, MODEL_DYN_PACEJKA>::fjh(P, x, u, nu, f, J, H); break;
    default: return -1;
  }
  return 0;
}

// ---- centerline geometry (mr_track.h) on host arrays: the same functions as the gfx950 kernels ----
int mrh_track_blob_size(int nt, int n_rows) { return track_layout(nt, n_rows).total; }
int mrh_track_build(const double* t, int nt, const double* cx, const double* cy, int nc, const double* el,
                    const double* er, int n_rows, double* blob) {
  track_tables(t, nt, cx, cy, nc, el, er, n_rows, blob);
  return 0;
}
int mrh_track_eval(const double* blob, int nt, double L, int n_rows, int n, const double* s, double* out, int* span) {
  TrackView T = track_view(blob, nt, L, n_rows);
  for (int i = 0; i < n; ++i) {
    double g[6];
    int sp;
    track_eval(T, s[i], g, &sp);
    for (int c = 0; c < 6; ++c) out[(int64_t)c * n + i] = g[c];
    if (span) span[i] = sp;
  }
  return 0;
}
int mrh_track_frame(const double* blob, int nt, double L, int n_rows, int n, const double* s, double* yaw,
                    double* kappa, double* nx, double* ny, double mcla, double* meank) {
  TrackView T = track_view(blob, nt, L, n_rows);
  for (int i = 0; i < n; ++i) {
    track_frame(T, s[i], yaw + i, kappa + i, nx + i, ny + i);
    if (meank) meank[i] = track_mean_curvature(T, s[i], mcla);
  }
  return 0;
}
int mrh_track_sign(const double* blob, int nt, double L, int n_rows, int n, const double* X, const double* Y,
                   const double* s, int* sign) {
  TrackView T = track_view(blob, nt, L, n_rows);
  for (int i = 0; i < n; ++i) sign[i] = track_error_sign(T, X[i], Y[i], s[i]);
  return 0;
}
int mrh_track_polyfit(const double* blob, int nt, double L, int n_rows, int n, const double* s, const double* la,
                      double* cx, double* cy) {
  TrackView T = track_view(blob, nt, L, n_rows);
  for (int i = 0; i < n; ++i) {
    double a[5], b[5];
    track_polyfit(T, s[i], la[i], a, b);
    for (int j = 0; j < 5; ++j) { cx[(int64_t)j * n + i] = a[j]; cy[(int64_t)j * n + i] = b[j]; }
  }
  return 0;
}
int mrh_track_polyfit_deg(const double* blob, int nt, double L, int n_rows, int n, const double* s, const double* la,
                          int deg, double* cx, double* cy) {
  TrackView T = track_view(blob, nt, L, n_rows);
  for (int i = 0; i < n; ++i) {
    double a[MR_POLY_DEG_MAX + 1], b[MR_POLY_DEG_MAX + 1];
    if (!track_polyfit_deg(T, s[i], la[i], deg, a, b)) return -1;
    for (int j = 0; j <= deg; ++j) { cx[(int64_t)j * n + i] = a[j]; cy[(int64_t)j * n + i] = b[j]; }
  }
  return 0;
}
int mrh_track_lookup(const double* blob, int nt, double L, int n_rows, int n, const double* s, const double* la,
                     double* err, int* lo, int* hi, int* arg) {
  TrackView T = track_view(blob, nt, L, n_rows);
  for (int i = 0; i < n; ++i) err[i] = lane_lookup(T, s[i], la[i], lo + i, hi + i, arg + i);
  return 0;
}
int mrh_track_projection(const double* blob, int nt, double L, int n_rows, int n, const double* X, const double* Y,
                         const double* lo, const double* hi, double* s, double* dist, int* nfev) {
  TrackView T = track_view(blob, nt, L, n_rows);
  for (int i = 0; i < n; ++i) {
    s[i] = brent_projection(T, X[i], Y[i], lo[i], hi[i], nfev + i);
    dist[i] = track_dist(T, s[i], X[i], Y[i]);
  }
  return 0;
}

int mrh_spline_from_waypoints(const double* x, const double* y, int n, int close_loop, double* t, double* cx,
                              double* cy, int* n_t, double* length) {
  const int np = spline_from_waypoints(x, y, n, close_loop, t, cx, cy, length);
  if (np < 0) return np;
  *n_t = np + 4;
  return 0;
}

// lane-width table build: the serial scan of mr_track.h lane_distance (the kernel's wave scan
// visits the same samples and breaks ties the same way)
int mrh_lane_table(const double* cblob, int cnt, double cL, int c_rows, const double* lblob, int lnt, double lL,
                   int n, const double* s, double* dist, double* s_lane) {
  TrackView C = track_view(cblob, cnt, cL, c_rows), Ln = track_view(lblob, lnt, lL, 0);
#pragma omp parallel for schedule(dynamic, 16)
  for (int i = 0; i < n; ++i) dist[i] = lane_distance(C, Ln, s[i], s_lane ? s_lane + i : nullptr);
  return 0;
}

int mrh_agent_sense(const double* blob, int nt, double L, int n_rows, int n, const double* X, const double* Y,
                    const double* prev, double lookback, double lookahead, double err_offset, double* progress,
                    double* error, double* cx, double* cy, double* merr) {
  TrackView T = track_view(blob, nt, L, n_rows);
  for (int i = 0; i < n; ++i) {
    AgentSense o;
    agent_sense(T, X[i], Y[i], prev ? prev[i] : NAN, lookback, lookahead, err_offset, o);
    progress[i] = o.progress;
    error[i] = o.error;
    for (int j = 0; j < 5; ++j) { cx[(int64_t)j * n + i] = o.cx[j]; cy[(int64_t)j * n + i] = o.cy[j]; }
    merr[i] = o.max_error;
  }
  return 0;
}
int mrh_plant_step(int model, int n, const double* state, const double* cmd, double dt, double* out) {
  for (int i = 0; i < n; ++i) {
    double x[6], o[6];
    for (int j = 0; j < 6; ++j) x[j] = state[(int64_t)j * n + i];
    plant_step(model, x, cmd[i], cmd[n + i], dt, o);
    for (int j = 0; j < 6; ++j) out[(int64_t)j * n + i] = o[j];
  }
  return 0;
}

// Pacejka jet (value, d/dalpha, d2/dalpha2) in fp64 and fp32.
int mrh_pacejka(const double* a, double Fz, double alpha, int fp32, double* out3) {
  TyreCoef<double> c = pacejka_coef(a, Fz);
  if (fp32) {
    TyreCoef<float> cf{(float)c.B, (float)c.C, (float)c.E, (float)c.BCD, (float)c.K2};
    TyreJet<float> j = pacejka_jet(cf, (float)alpha);
    out3[0] = j.v; out3[1] = j.d; out3[2] = j.dd;
  } else {
    TyreJet<double> j = pacejka_jet(c, alpha);
    out3[0] = j.v; out3[1] = j.d; out3[2] = j.dd;
  }
  return 0;
}

// ---- tyre-model fitting (mr_tyrefit.h): the kernels' wave functions as emulated wavefronts ----
static thread_local const char* g_tyrefit_err = "";
static int tyrefit_fail(const char* msg) {
  g_tyrefit_err = msg;
  return -1;
}
// reason of the last -1 returned by mrh_tyre_loss_grad / mrh_tyre_fit on this thread
const char* mrh_tyrefit_last_error(void) { return g_tyrefit_err; }
int mrh_tyrefit_config_default(mr_tyrefit_config* c) {
  fill_default_tyrefit_config(c);
  return 0;
}

int mrh_tyre_loss_grad(const mr_tyrefit_config* cfg, int n, const double* rows, int P, const double* params,
                       const double* Fz, double* loss, double* grad) {
  if (const char* e = tyrefit_check_config(cfg)) return tyrefit_fail(e);
  if (!rows || !params || !Fz || !loss || !grad) return tyrefit_fail("null argument");
  if (n < 1) return tyrefit_fail("n < 1");
  if (P < 1) return tyrefit_fail("P < 1");
  const int n_chunk = (n + WL - 1) / WL;
  std::vector<double> partials((size_t)P * n_chunk * TF_NSUM, NAN);
  for (int p = 0; p < P; ++p)
    for (int k = 0; k < n_chunk; ++k)
      host_wave_call([&](const Wv& w) {
        tf_lossgrad_chunk(w, *cfg, n, rows, p, k, n_chunk, params, Fz, partials.data());
      });
  for (int p = 0; p < P; ++p) tf_lossgrad_finish(*cfg, n, p, n_chunk, partials.data(), params, Fz, loss, grad);
  return 0;
}

int mrh_tyre_fit(const mr_tyrefit_config* cfg, int n_train, const double* train, int n_val, const double* val, int R,
                 const double* init, const double* Fz, const double* hyper, const int32_t* perm,
                 int64_t perm_stride_run, double* p_final, double* p_best, double* train_loss, double* val_loss,
                 double* lr_hist, int32_t* flag, double* p_steps, int nthreads) {
  if (const char* e = tyrefit_check_fit(cfg, n_train, n_val, R, perm_stride_run)) return tyrefit_fail(e);
  if (!train || !val || !init || !Fz || !hyper || !perm || !p_final || !p_best || !train_loss || !val_loss ||
      !lr_hist || !flag)
    return tyrefit_fail("null argument");
  const int64_t per_run = (int64_t)cfg->epochs * n_train;
  for (int r = 0; r < (perm_stride_run ? R : 1); ++r)
    for (int64_t k = 0; k < per_run; ++k) {
      const int32_t v = perm[r * perm_stride_run + k];
      if (v < 0 || v >= n_train) return tyrefit_fail("perm entry out of range [0, n_train)");
    }
  const TfFitArgs A = make_tf_fit_args(*cfg, n_train, train, n_val, val, R, init, Fz, hyper, perm, perm_stride_run,
                                       p_final, p_best, train_loss, val_loss, lr_hist, flag, p_steps);
#pragma omp parallel for schedule(dynamic, 1) num_threads(nthreads > 0 ? nthreads : 1)
  for (int r = 0; r < R; ++r)
    host_wave_call([&](const Wv& w) {
      if (A.cfg.kind == MR_TYRE_PACEJKA) tf_fit_run<MR_TYRE_PACEJKA>(A, r, w);
      else tf_fit_run<MR_TYRE_LINEAR>(A, r, w);
    });
  return 0;
}

// ---- open-loop rollouts and the model as a plant (mr_rollout.h) ----
int mrh_vehicle_step(const mr_tyrefit_config* cfg, int n, const double* state, const double* cmd, double dt, int P,
                     const double* params, const double* Fz, double* out) {
  if (const char* e = vehicle_step_check(cfg, n, P)) return tyrefit_fail(e);
  if (!state || !cmd || !params || !Fz || !out) return tyrefit_fail("null argument");
  for (int i = 0; i < n; ++i) {
    if (cfg->kind == MR_TYRE_PACEJKA) ro_vehicle_step<MR_TYRE_PACEJKA>(*cfg, n, i, state, cmd, dt, P, params, Fz, out);
    else ro_vehicle_step<MR_TYRE_LINEAR>(*cfg, n, i, state, cmd, dt, P, params, Fz, out);
  }
  return 0;
}

int mrh_tyre_rollout(const mr_tyrefit_config* cfg, int T, const double* log, int n_start, const int32_t* start, int H,
                     int P, const double* params, const double* Fz, double* stats, int32_t* count, double* pred,
                     int nthreads) {
  if (const char* e = tyre_rollout_check(cfg, T, n_start, H, P)) return tyrefit_fail(e);
  if (!log || !start || !params || !Fz || !stats || !count) return tyrefit_fail("null argument");
  const RoArgs A = make_ro_args(T, log, n_start, start, H, params, Fz, pred);
  if (const char* e = rollout_starts_check(A)) return tyrefit_fail(e);
  rollout_host(A, P, stats, count, nthreads, [&](const RoArgs& Ap, int p, int chunk, double* lds, const Wv& w) {
    ro_chunk_kind(*cfg, Ap, p, p, chunk, lds, w);
  });
  return 0;
}

// ---- the plant with run-time parameters and its rollouts (mr_plantroll.h) ----
int mrh_plant_params_default(double* params) {
  plant_params_default(params);
  return 0;
}
int mrh_plant_step_params(int model, int n, const double* state, const double* cmd, double dt, int P,
                          const double* params, double* out) {
  if (const char* e = plant_step_params_check(model, n, P)) return tyrefit_fail(e);
  if (!state || !cmd || !params || !out) return tyrefit_fail("null argument");
  for (int i = 0; i < n; ++i) pr_vehicle_step(model, n, i, state, cmd, dt, P, params, out);
  return 0;
}

int mrh_plant_rollout(int model, int T, const double* log, int n_start, const int32_t* start, int H, int P,
                      const double* params, const double* dt, double* stats, int32_t* count, double* pred,
                      int nthreads) {
  if (const char* e = plant_rollout_check(model, T, n_start, H, P)) return tyrefit_fail(e);
  if (!log || !start || !params || !stats || !count) return tyrefit_fail("null argument");
  const RoArgs A = make_ro_args(T, log, n_start, start, H, params, dt, pred);
  if (const char* e = rollout_starts_check(A)) return tyrefit_fail(e);
  for (int p = 0; dt && p < P; ++p)
    if (!plant_dt_ok(dt[p])) return tyrefit_fail("dt entry not a positive finite number");
  plant_dispatch(model, [&](auto model_c) {
    rollout_host(A, P, stats, count, nthreads, [&](const RoArgs& Ap, int p, int chunk, double* lds, const Wv& w) {
      ro_chunk(Ap, RoPlantModel<decltype(model_c)::value>(Ap, p), p, p, chunk, lds, w);
    });
  });
  return 0;
}

// Pacejka force and its parameter gradient dFy/da[0..8] at a slip angle (mr_tyrefit.h), fp64
int mrh_pacejka_dparams(const double* a, double Fz, double alpha, double* Fy, double* dFy_da) {
  TfCoef t = tf_coef(a, Fz);
  double d[4];
  *Fy = pacejka_partials(t.c, alpha, d);
  pacejka_chain(t, a, Fz, d, dFy_da);
  return 0;
}

// ---- the PID agent (mr_pid.h): the blob arguments of mrh_agent_sense ----
int mrh_pid_gains_default(double* gains) {
  pid_gains_default(gains);
  return 0;
}
int mrh_pid_control(const double* blob, int nt, double L, int n_rows, int n, const double* state, double* mem, int G,
                    const double* gains, double dt, double* out) {
  if (const char* e = pid_control_check(n, G, dt)) return tyrefit_fail(e);
  if (!blob || !state || !mem || !gains || !out) return tyrefit_fail("null argument");
  TrackView T = track_view(blob, nt, L, n_rows);
  for (int i = 0; i < n; ++i) pid_control_vehicle(T, n, i, state, mem, G, gains, dt, out);
  return 0;
}
int mrh_pid_drive(const double* blob, int nt, double L, int n_rows, int model, int n, int T, double dt, double* state,
                  double* mem, int G, const double* gains, int P, const double* params, uint32_t log_mask,
                  double* log, int32_t* ticks_done, int nthreads) {
  if (const char* e = pid_drive_check(model, n, T, dt, G, P, log_mask, log)) return tyrefit_fail(e);
  if (!blob || !state || !mem || !gains || !params || !ticks_done) return tyrefit_fail("null argument");
  const TrackView Tr = track_view(blob, nt, L, n_rows);
  const PidDriveArgs A = make_pid_drive_args(n, T, dt, state, mem, G, gains, P, params, log_mask, log, ticks_done);
  plant_dispatch(model, [&](auto model_c) {
#pragma omp parallel for schedule(dynamic, 1) num_threads(nthreads > 0 ? nthreads : 1)
    for (int i = 0; i < n; ++i)
      pid_drive_vehicle<decltype(model_c)::value>(Tr, A, i, true, params + (int64_t)(P == 1 ? 0 : i) * MR_PLANT_NPAR,
                                                  PidVoteLane());
  });
  return 0;
}

// ---- the GA (mr_ga.h, mr_pid.h pid_segment_vehicle): one lane at a time for the drive, an emulated wave per island ----
int mrh_pid_segment_times(const double* blob, int nt, double L, int n_rows, int model, int n, int K, int T, double dt,
                          const double* start, const double* s_start, const double* s_end, const double* gains, int P,
                          const double* params, double* times, int32_t* ticks_done, int nthreads) {
  if (const char* e = pid_segment_check(model, n, K, T, dt, P)) return tyrefit_fail(e);
  if (!blob || !start || !s_start || !s_end || !gains || !params || !times || !ticks_done)
    return tyrefit_fail("null argument");
  const TrackView Tr = track_view(blob, nt, L, n_rows);
  const PidSegArgs A = make_pid_seg_args(n, K, T, dt, start, s_start, s_end, gains, P, params, times, ticks_done);
  plant_dispatch(model, [&](auto model_c) {
#pragma omp parallel for schedule(dynamic, 1) num_threads(nthreads > 0 ? nthreads : 1)
    for (int i = 0; i < n; ++i)
      pid_segment_vehicle<decltype(model_c)::value>(Tr, A, i, true, params + (int64_t)(P == 1 ? 0 : i) * MR_PLANT_NPAR,
                                                    PidVoteLane());
  });
  return 0;
}
int mrh_ga_random(uint64_t seed, uint64_t island, uint64_t generation, uint64_t first, int64_t count, uint64_t* out) {
  if (count < 0) return tyrefit_fail("count < 0");
  if (count > 0 && !out) return tyrefit_fail("null argument");
  GaStream rs(seed, island, generation);
  for (int64_t j = 0; j < count; ++j) out[j] = rs.raw(first + (uint64_t)j);
  return 0;
}
int mrh_ga_breed(int n_island, int P, int K, int D, int pairs, double* genes, int ld, const int32_t* col,
                 const double* times, double* avg,
                 const double* lo, const double* hi, double kT, double lambda_T, double mutation_rate, uint64_t seed,
                 uint64_t island0, uint64_t generation, double* r, double* best_r, int32_t* best_idx,
                 double* best_genes) {
  if (const char* e = ga_breed_check(n_island, P, K, D, pairs, ld, col, kT, lambda_T, mutation_rate)) return tyrefit_fail(e);
  if (!genes || !times || !avg || !r || !best_r || !best_idx || !best_genes) return tyrefit_fail("null argument");
  const GaBreedArgs A = make_ga_breed_args(n_island, P, K, D, pairs, genes, ld, col, times, avg, lo, hi, kT, lambda_T,
                                           mutation_rate, seed, island0, generation, r, best_r, best_idx, best_genes);
  for (int i = 0; i < n_island; ++i) {
    GaShared* sh = new GaShared();
    host_wave_call([&](const Wv& w) { ga_breed_island(w, A, i, sh); });
    delete sh;
  }
  return 0;
}

// ---- the glue of the MPC's segment drives (mr_mpcseg.h): one lane at a time ----
int mrh_mpcseg_runtime(int n_ind, int K, const double* genes, const double* lo, const double* hi, double d_max,
                       double* runtime) {
  if (const char* e = mpcseg_runtime_check(n_ind, K)) return tyrefit_fail(e);
  if (!genes || !lo || !hi || !runtime) return tyrefit_fail("null argument");
  for (int j = 0; j < n_ind * K; ++j) mpcseg_runtime_vehicle(n_ind, K, j, genes, lo, hi, d_max, runtime);
  return 0;
}
int mrh_mpcseg_inputs(int n, int K, int N, int tick, double dt, double L, const double* state, const double* progress,
                      const double* mem, const double* s_start, const double* s_end, const double* U_prev,
                      const int32_t* horizon_prev, const int32_t* horizon_in, double hz_lookahead, double Ts,
                      int hz_min, double* state0, double* u_init, int32_t* horizon_out, int32_t* done, double* times,
                      int32_t* ticks_done) {
  if (const char* e = mpcseg_inputs_check(n, K, N, tick, dt, L, hz_lookahead, Ts, hz_min, horizon_in, U_prev, u_init))
    return tyrefit_fail(e);
  if (!state || !progress || !mem || !s_start || !s_end || !state0 || !horizon_out || !done || !times || !ticks_done)
    return tyrefit_fail("null argument");
  const MpcSegInputsArgs A{n, K, N, tick, hz_min, dt, L, hz_lookahead, Ts, state, progress, mem, s_start, s_end,
                           U_prev, horizon_prev, horizon_in, state0, u_init, horizon_out, done, times, ticks_done};
  for (int i = 0; i < n; ++i) mpcseg_inputs_vehicle(A, i);
  return 0;
}
int mrh_mpcseg_apply(int model, int n, int K, int N, double dt, double L, double* state, double* mem,
                     const double* progress, const double* s_start, const int32_t* done, const double* U, int P,
                     const double* params) {
  if (const char* e = mpcseg_apply_check(model, n, K, N, dt, L, P, params)) return tyrefit_fail(e);
  if (!state || !mem || !progress || !s_start || !done) return tyrefit_fail("null argument");
  const MpcSegApplyArgs A{model, n, K, N, P, dt, L, state, mem, progress, s_start, done, U, params};
  for (int i = 0; i < n; ++i) mpcseg_apply_vehicle(A, i);
  return 0;
}

}  // extern "C"

// ---- probes of the wave primitives and the fp32 pieces (mr_probe.h): the bodies that
// libmpcracing_probe.so runs on gfx950, here under the fibre emulation / with libm ----
template <typename T>
static int run_prims_host(int n_wg, T* in, T* out) {
  if (n_wg < 1 || !in || !out) return -1;
  for (int g = 0; g < n_wg; ++g) host_wave_call([&](const Wv& w) { probe::prims_body<T>(w, g, n_wg, in, out); });
  return 0;
}
template <typename T>
static int run_mfma_host(int n_wg, const T* A, const T* B, const T* C, T* D) {
  if (n_wg < 1 || !A || !B || !C || !D) return -1;
  for (int g = 0; g < n_wg; ++g) host_wave_call([&](const Wv& w) { probe::mfma_body<T>(w, g, A, B, C, D); });
  return 0;
}

extern "C" {

void mrh_probe_layout(int32_t* out8) {
  out8[0] = probe::PRIMS_IN_W; out8[1] = probe::PRIMS_OUT_W; out8[2] = probe::MFMA_A_W; out8[3] = probe::MFMA_B_W;
  out8[4] = probe::MFMA_C_W; out8[5] = probe::MFMA_D_W; out8[6] = probe::PS_COUNT; out8[7] = 0;
}
int mrh_wave_prims_f32(int n_wg, float* in, float* out) { return run_prims_host<float>(n_wg, in, out); }
int mrh_wave_prims_f64(int n_wg, double* in, double* out) { return run_prims_host<double>(n_wg, in, out); }
int mrh_wave_prims_i32(int n_wg, int32_t* in, int32_t* out) { return run_prims_host<int>(n_wg, in, out); }
int mrh_wave_mfma_f32(int n_wg, const float* A, const float* B, const float* C, float* D) {
  return run_mfma_host<float>(n_wg, A, B, C, D);
}
int mrh_wave_mfma_f64(int n_wg, const double* A, const double* B, const double* C, double* D) {
  return run_mfma_host<double>(n_wg, A, B, C, D);
}

// Dyn<float, MODEL> with libm (the host's fp32 build of the model), n points; J == NULL: value only
int mrh_eval_dynamics_f32(const mr_config* c, const double* a_front, double Fz_front, const double* a_back,
                          double Fz_back, int n, const float* x, const float* u, const float* nu, float* f, float* J,
                          float* H) {
  if (!c || n < 0 || !x || !u || !f || ((J != nullptr) != (H != nullptr)) || (J && !nu)) return -1;
  TyreCoef<double> tf{}, tr{};
  if (a_front) tf = pacejka_coef(a_front, Fz_front);
  if (a_back) tr = pacejka_coef(a_back, Fz_back);
  ProbParams<float> P;
  fill_params<float>(*c, tf, tr, P);
#define MR_CASE(M)                                                                                            \
  for (int i = 0; i < n; ++i) {                                                                               \
    if (J) Dyn<float, M>::fjh(P, x + 6 * i, u + 2 * i, nu + 6 * i, f + 6 * i, J + 48 * i, H + 36 * i);          \
    else Dyn<float, M>::f(P, x + 6 * i, u + 2 * i, f + 6 * i);                                                \
  }
  switch (c->model) {
    case MR_MODEL_KINEMATIC: MR_CASE(MODEL_KIN) break;
    case MR_MODEL_DYNAMIC: MR_CASE(MODEL_DYN) break;
    case MR_MODEL_BLENDED: MR_CASE(MODEL_BLEND) break;
    case MR_MODEL_BLENDED_PACEJKA: MR_CASE(MODEL_BLEND_PACEJKA) break;
    case MR_MODEL_DYNAMIC_PACEJKA: MR_CASE(MODEL_DYN_PACEJKA) break;
    default: return -1;
  }
#undef MR_CASE
  return 0;
}

// chol3r + lsolve3r + ltsolve3r in float with libm, n systems (R packed r00 r10 r20 r11 r21 r22)
int mrh_chol3_f32(int n, const float* R, const float* b, int32_t* ok, float* L, float* iv, float* x) {
  if (n < 0 || !R || !b || !ok || !L || !iv || !x) return -1;
  for (int i = 0; i < n; ++i) {
    float xl[3] = {b[3 * i], b[3 * i + 1], b[3 * i + 2]};
    ok[i] = chol3r(R + 6 * i, L + 6 * i, iv + 3 * i) ? 1 : 0;
    lsolve3r(L + 6 * i, iv + 3 * i, xl);
    ltsolve3r(L + 6 * i, iv + 3 * i, xl);
    for (int j = 0; j < 3; ++j) x[3 * i + j] = xl[j];
  }
  return 0;
}

}  // extern "C"
