/*
 * mpcracing.h -- C ABI of the MI355X batched racing-MPC solver (libmpcracing.so).
 *
 * Drop-in boundary for the reference's hot path: the reference has no FFI; its
 * boundary is the Python class control.MPC.MPC (AlexGisi/mpc-racing
 * control/MPC.py:10-22 constructor, :183-184 solution()).  Each entry point
 * below replaces a piece of that class:
 *
 *   mr_config_default / mr_create   <- FixedControllerParameters (control/ControllerParameters.py:3-23),
 *                                      VehicleParameters (models/VehicleParameters.py:3-41),
 *                                      the IPOPT options dict (control/MPC.py:151-161)
 *   mr_set_tyres                    <- learned Pacejka tyres substituted into f_vehicle
 *                                      (learning/vehicle.py:79-92, :155-160)
 *   mr_solve_batch                  <- MPC.__init__ build + opti.solve() + the ret tuple
 *                                      (control/MPC.py:30-181) for B independent instances
 *   mr_last_error                   <- the RuntimeError text printed at control/MPC.py:173
 *
 * Conventions: every function returns 0 on success and a negative code on error
 * (message via mr_last_error(), thread-local).  All batch arrays are caller-owned
 * DEVICE pointers (e.g. torch tensors' data_ptr()) in structure-of-arrays layout
 * with the instance index fastest: element [c][i] of a [C][B] array is at
 * ptr[c*B + i].  All I/O is float64 regardless of the handle's compute precision.
 * Calls are ordered on the given HIP stream; a handle is bound to one device and is
 * not thread-safe.
 */
#ifndef MPCRACING_H
#define MPCRACING_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version (mr_version()): bumped whenever a struct layout or an entry point's meaning changes, so
   a caller built against another header can refuse to run (101: mr_config.dispatch_order,
   mr_outputs.lam_g / timeline, mr_config without lane_penalty (hard lane rows), status 4 = infeasible;
   102: mr_inputs.order_hint, dispatch_order 2; 103: mr_tyrefit_config, mr_tyre_loss_grad, mr_tyre_fit; still 103, additions only:
   mr_vehicle_step, mr_tyre_rollout, mr_plant_params_default, mr_plant_step_params, mr_plant_rollout,
   mr_pid_gains_default, mr_pid_control, mr_pid_drive, mr_pid_segment_times, mr_ga_random, mr_ga_breed,
   mr_solve_batch_horizons, mr_warm, mr_solve_batch_warm, mr_warm_shift,
   mr_mpcseg_runtime, mr_mpcseg_inputs, mr_mpcseg_apply) */
#define MR_ABI_VERSION 103

#define MR_OK 0
#define MR_ERR_ARG (-1)
#define MR_ERR_HIP (-2)
#define MR_ERR_STATE (-3)

/* dynamics models of the NLP */
#define MR_MODEL_KINEMATIC 0       /* control/MPC.py:231-260 (f_vehicle_kinematic)          */
#define MR_MODEL_DYNAMIC 1         /* control/MPC.py:186-229 (f_vehicle, the reference NLP)  */
#define MR_MODEL_BLENDED 2         /* lambda*dyn + (1-lambda)*kin, models/BlendedBicycleModel.py:22-46 */
#define MR_MODEL_BLENDED_PACEJKA 3 /* blended with learned Pacejka lateral forces            */
#define MR_MODEL_DYNAMIC_PACEJKA 4 /* dynamic with learned Pacejka lateral forces            */

/* plant models of the closed loop (the numpy simulator-side models) */
#define MR_PLANT_KINEMATIC 0 /* models/KinematicBicycleModel.py:11-48 */
#define MR_PLANT_DYNAMIC 1   /* models/DynamicBicycleModel.py:16-78   */
#define MR_PLANT_BLENDED 2   /* models/BlendedBicycleModel.py:18-58   */

#define MR_PREC_FP64 0
#define MR_PREC_FP32 1

/* per-instance solver status (replaces the try/except + breakpoint() of control/MPC.py:164-181) */
#define MR_STATUS_SOLVED 0
#define MR_STATUS_ACCEPTABLE 1
#define MR_STATUS_MAX_ITER 2
#define MR_STATUS_FAILED 3 /* non-finite values, no inertia-correct factorisation, or the restoration
                              phase's line search failed (IPOPT: Restoration_Failed) */
#define MR_STATUS_INFEASIBLE 4 /* the restoration phase converged to a minimiser of the constraint
                                  violation the original problem does not accept (IPOPT:
                                  Infeasible_Problem_Detected, "local infeasibility") */

typedef struct mr_config {
  int32_t N;           /* horizon (FixedControllerParameters.N = 30 unless the caller passes N) */
  int32_t model;       /* MR_MODEL_* */
  int32_t precision;   /* MR_PREC_* : arithmetic type of the solve */
  int32_t lane_bounds; /* 1 enables |e_C(S_i, X_i)| <= max_error, i = 1..N (the commented MPC.py:135) */
  int32_t max_batch;   /* workspace capacity (instances) */
  int32_t device;      /* HIP device ordinal */
  int32_t max_iter;    /* FixedControllerParameters.max_iter = 500 */
  int32_t acceptable_iter; /* IPOPT acceptable_iter (15); 0 disables acceptable termination */
  double Ts;           /* sampling time */
  double tol;          /* KKT tolerance of the scaled NLP (IPOPT tol) */
  double acceptable_tol;
  /* FixedControllerParameters (control/ControllerParameters.py:3-23) */
  double lambda_s, alpha_L, min_steer, max_steer, min_throttle, max_steer_delta, min_steer_delta,
      max_throttle_delta, min_throttle_delta, q_v_max, v_max, min_s_delta;
  /* VehicleParameters (models/VehicleParameters.py:3-41); max_steer_deg = VehicleParameters.max_steer */
  double m, Iz, lf, lr, Cf, Cr, T_max, r_wheel, C_wheel, R, rho, C_d, A_f, C_roll, g, max_steer_deg,
      Vblendmin, Vblendmax;
  /* workgroup dispatch order of a batch (results do not depend on it: instances are independent):
     0 = instance order; 1 = (default) a stable three-tier partition so the likely long solves start
     first: tier 0 = v >= 40 m/s, or throttle <= -0.5 at v <= 20 m/s (hard braking through a blend
     corner of the model); tier 1 = the rest outside 16.5 < v < 39; tier 2 = the others (a cold-start
     guess from the model's nonsmooth / stiff regions, for batches without history);
     2 = longest-expected-first by mr_inputs.order_hint (e.g. the previous MPC tick's iters of the same
     vehicles: LPT scheduling with a distribution-agnostic estimate); without a hint, the handle's own
     previous solve of the same batch size (its iters, kept on the device and read in stream order: calls
     on different streams must be ordered by the caller), else instance order; a uniform hint (all equal)
     gives instance order */
  int32_t dispatch_order;
} mr_config;

typedef struct mr_inputs {
  const double* state0;  /* [8][B]: x, y, yaw, v_x, v_y, yaw_dot, throttle, steer (NaN = None) */
  const double* s0;      /* [B] initial progress */
  const double* cx;      /* [5][B] centerline x polynomial, highest order first, global s */
  const double* cy;      /* [5][B] */
  const double* max_error; /* [B] lane half width (used when lane_bounds) */
  const double* runtime; /* [5][B] RuntimeControllerParameters: alpha_c, d_max, q_v_y, n, beta_delta.
                            NOTE control/MPC.py:50 reads the CLASS attribute d_max; the Python
                            drop-in passes that value here to keep the quirk. */
  const double* u_init;  /* optional [2][N][B] initial controls (already shifted last_controls,
                            control/MPC.py:120-125); NULL -> (throttle0, steer0) repeated */
  const int32_t* order_hint; /* optional [B] expected cost of each instance (larger = dispatched earlier),
                            read only with mr_config.dispatch_order = 2, before the solve starts (so the
                            previous call's mr_outputs.iters may be passed in place) */
} mr_inputs;

typedef struct mr_outputs {
  double* X;      /* [6][N+1][B] States (control/MPC.py:166) */
  double* U;      /* [2][N][B] */
  double* S;      /* [N+1][B] S_hat */
  double* eC;     /* [N][B] e_hat_C(S_hat[i], States[:, i]), i = 0..N-1 */
  double* eL;     /* [N][B] e_hat_L */
  int32_t* status; /* [B] MR_STATUS_* */
  int32_t* iters;  /* [B] interior-point iterations */
  double* obj;     /* optional [B] objective value (NULL to skip) */
  double* kkt;     /* optional [B] final scaled KKT error (NULL to skip) */
  double* trace;   /* optional [trace_cap][8] per-iteration record of instance trace_instance:
                      kkt, mu, alpha_primal, alpha_dual, delta (inertia), theta, phi, line-search trials */
  int32_t trace_instance;
  int32_t trace_cap;
  double* lam_g;   /* optional [13N+9][B]: the reference's dual = sol.value(opti.lam_g) (control/MPC.py:171)
                      in Opti row order (MPC.py:101-149): S_0, X_{:,0} (6), per i = 1..N the 6 dynamics rows and
                      the Delta-S row, per i = 0..N-1 thr < d_max, thr > min, steer < max, steer > min, the
                      throttle and steer rate rows (i = 0: against U[:, N-1]), then the state0 throttle and
                      steer rows (NaN when state0 has no throttle / steer).  CasADi convention: Lagrangian
                      f + lam_g . g, canonical row = the non-constant side (positive at an active upper
                      bound); unscaled objective.  NULL to skip. */
  int64_t* timeline; /* optional [2][B] diagnostics: device clock (s_memrealtime, 100 MHz) when instance i's
                        workgroup started and finished; NULL to skip */
  double* constr_viol; /* optional [B]: IPOPT's unscaled constraint violation of the returned point (max-norm
                          of the dynamics / initial-state rows and of the rows' bound violations; the
                          "Constraint violation" IPOPT prints on exit).  Measured, as IPOPT measures it, against
                          the bounds relaxed by bound_relax_factor: each finite bound b moved outwards by
                          1e-8 max(1, |b|), so a point up to that far outside a stated bound reports 0 for the
                          row (the lane rows included, with lane_bounds).  Tells a status-3 stop at an
                          almost-feasible point from a restoration failure.  NULL to skip */
} mr_outputs;
/* What obj, kkt, constr_viol and lam_g refer to, by how the solve ended.  X, U, S, eC, eL are always the last
   iterate the solver holds; obj, constr_viol, eC and eL are that point's (tests/test_gpu_certificate.py re-derives
   them from X, U, S at every exit) with the exceptions named here:
     status 0, and status 1 after acceptable_iter acceptable iterations or when the line search fails at an
       acceptable point: the current iterate of the original problem, its scaled KKT error in kkt, its
       multipliers in lam_g.
     status 1 otherwise (the line search failed at an almost feasible point, or the fp32 stall exit at the mu
       floor): the stored acceptable point restored whole -- X, U, S, every multiplier, and the obj, kkt and
       constr_viol saved with it; lam_g is that point's, not the abandoned iterate's.
     status 2 (max_iter): the last evaluated iterate; obj, kkt and constr_viol are its own, lam_g holds its
       multipliers, which satisfy no tolerance.  If the limit falls inside the restoration phase, see below.
     status 3 from the original problem (mu floor with a tiny step, no inertia-correct factorisation, or an almost
       feasible line-search failure without a stored point): the current iterate and its measures; where
       kkt <= tol only one of IPOPT's unscaled tests (dual_inf_tol, constr_viol_tol, compl_inf_tol) kept it from
       status 0, and lam_g is as accurate as at status 0.
     status 3 / 4 / 2 inside the restoration phase: X, U, S are the restoration iterate; obj is the original
       objective there and constr_viol the original problem's violation there; kkt is the last value the
       original problem had before the phase; lam_g holds the
       restoration NLP's multipliers (of the order of |grad f| away from a KKT multiplier, signs not those of the
       original rows): diagnostic only.
     status 3 after a non-finite evaluation: X, U, S are the iterate whose evaluation failed; obj, kkt and
       constr_viol are stale (the previous iterate's; 0 if the first evaluation failed), lam_g unspecified. */

typedef struct mr_handle mr_handle;

int mr_version(void);
const char* mr_last_error(void);
int mr_config_default(mr_config* cfg);
int mr_create(mr_handle** h, const mr_config* cfg);
int mr_destroy(mr_handle* h);
/* Pacejka coefficients a[0..8] and vertical load Fz for the front and back tyre
   (state dict keys front_tire.a / front_tire.Fz / back_tire.a / back_tire.Fz).  Synchronises the
   handle's device before it replaces the constants the kernels read (solves in flight on any stream
   finish first). */
int mr_set_tyres(mr_handle* h, const double* a_front, double Fz_front, const double* a_back, double Fz_back);
int mr_solve_batch(mr_handle* h, int32_t B, const mr_inputs* in, mr_outputs* out, void* hip_stream);
/* mr_solve_batch with one horizon per instance (the reference chooses N per call from the car's speed,
   script/test_mpc.py:32-33).  horizon: device int32 [B], or NULL (= mr_solve_batch, the same code path).
     horizon[i] = N_i, 1 <= N_i <= cfg.N.  cfg.N stays the LAYOUT horizon: every array keeps the strides
   documented above (X [6][cfg.N+1][B], U [2][cfg.N][B], S, eC, eL, u_init [2][cfg.N][B],
   lam_g [13*cfg.N+9][B]).  Instance i is solved exactly as a handle created with N = N_i solves it: it reads
   u_init[r][k][i] for k < N_i only, writes X / S rows k <= N_i and U / eC / eL rows k < N_i, and its lam_g
   column holds, in its first 13*N_i+9 rows, the Opti row order of horizon N_i (what the reference's call with
   that N returns).  Every other row of the instance's columns is NaN.
     An instance whose horizon[i] is outside [1, cfg.N] is not solved: status MR_STATUS_FAILED, iters 0, NaN in
   every float output of its columns (obj / kkt / constr_viol / lam_g included where given), nothing written
   outside its columns; timeline, where given, holds the short span of its workgroup.  The array is read by the kernel only: no host read, no synchronisation. */
int mr_solve_batch_horizons(mr_handle* h, int32_t B, const mr_inputs* in, mr_outputs* out, const int32_t* horizon,
                            void* hip_stream);
/* A caller's primal guess (what opti.set_initial(States, ...) / set_initial(S_hat, ...) give a CasADi user; the
   reference itself ignores its sol0, control/MPC.py:22).  Device arrays in the layout of mr_outputs.X / S. */
typedef struct mr_warm {
  const double* x_init;  /* [6][cfg.N+1][B]  States guess, global coordinates; row k = 0 is never read */
  const double* s_init;  /* [cfg.N+1][B]     S_hat guess, global progress;    row k = 0 is never read */
  const int32_t* use;    /* optional [B]: 0 = this instance starts cold; NULL = all warm */
  int32_t* used;         /* optional [B] out: 1 if the instance started from the guess, else 0 */
} mr_warm;
/* mr_solve_batch_horizons from a primal guess.  warm == NULL is mr_solve_batch_horizons (the same code path, the
   same bits); otherwise x_init and s_init are required.
     Warm instance: instance i with horizon N_i starts from w0 = (U = u_init rows k < N_i, or (throttle0, steer0)
   repeated when u_init is NULL; X_0 = state0, S_0 = s0; X_k = x_init[:, k, i] and S_k = s_init[k, i] for
   k = 1..N_i) instead of the rollout of the controls and S_k = s0 + k Ts v_max (control/MPC.py:120-131).
   Everything after that is IPOPT's treatment of a user-given x0, as at a cold start: the objective scaling is
   taken at w0, the slacks are pushed inside their bounds, bound multipliers 1, the least-squares multiplier
   estimate, mu = 0.1; the dynamics defects of w0 count in the initial constraint violation (the filter's
   theta_max / theta_min).  No duals, no mu warm start.  The guess is made relative to (state0.x, state0.y, s0) in
   fp64 before an fp32 handle rounds it.
     Cold instance: use[i] == 0, or a non-finite value in rows 1..N_i of the instance's x_init / s_init columns
   (decided by the instance's wavefront on the device).  It has the bits of mr_solve_batch_horizons, and
   used[i] = 0.  Rows beyond N_i and row 0 of the guess are never read.  use, x_init and s_init are read by the
   kernel only: no host read, no synchronisation. */
int mr_solve_batch_warm(mr_handle* h, int32_t B, const mr_inputs* in, mr_outputs* out, const int32_t* horizon,
                        const mr_warm* warm, void* hip_stream);
/* The next tick's guess from the previous tick's outputs, on the device, one lane per instance (the shift of
   last_controls, control/MPC.py:120-125, extended to the States and S_hat the reference throws away).  Arrays in
   the handle's layout (NL = cfg.N): X_prev [6][NL+1][B], U_prev [2][NL][B], S_prev [NL+1][B], status_prev [B],
   horizon_prev / horizon_new int32 [B] or NULL (= NL), state0_new [8][B] (rows 0..5 read), s0_new [B]; outputs
   u_init [2][NL][B], x_init [6][NL+1][B], s_init [NL+1][B], use int32 [B].  Per instance, Np = previous and
   Nn = new horizon:
     u_init[:, k] = U_prev[:, min(k + 1, Np - 1)], k = 0..NL-1 (every row: also the cold start's shifted controls);
     k = 1..Nn, k + 1 <= Np: x_init[:, k] = X_prev[:, k + 1], s_init[k] = s0_new + (S_prev[k + 1] - S_prev[1])
       (differences: a progress that wrapped at the lap end between the ticks needs no special case);
     otherwise: x_init[:, k] = f(x_init[:, k - 1], u_init[:, k - 1]), one step of the handle's MPC model in fp64
       with its tyres (the value path of mr_eval_dynamics; for k = 1, from state0_new), and
       s_init[k] = s_init[k - 1] + (S_prev[Np] - S_prev[Np - 1]) (s_init[0] = s0_new);
     row 0 and rows beyond Nn of x_init / s_init are NaN;
     use = 1 iff status_prev is 0 or 1, Np >= 2 and every value written to u_init rows k < Nn and x_init / s_init
       rows 1..Nn is finite (a non-finite value read shows in one written); else 0.
   A horizon outside [1, NL]: use = 0, x_init / s_init NaN, u_init from Np clamped into [1, NL].  The outputs
   must not overlap the inputs.  No host read, no synchronisation. */
int mr_warm_shift(mr_handle* h, int32_t B, const double* X_prev, const double* U_prev, const double* S_prev,
                  const int32_t* status_prev, const int32_t* horizon_prev, const double* state0_new,
                  const double* s0_new, const int32_t* horizon_new, double* u_init, double* x_init, double* s_init,
                  int32_t* use, void* hip_stream);
/* Diagnostics: the handle's vehicle dynamics (fp64) at n points, device arrays x [n][6], u [n][2],
   nu [n][6] -> f [n][6], J [n][6*8] (d f / d(x, u)), H [n][36] (packed upper triangle of
   sum_i nu_i d2 f_i / d(x, u)^2); J == NULL evaluates the value-only variant into f.
   Replaces CasADi's evaluation of f_vehicle (control/MPC.py:186-229). */
int mr_eval_dynamics(mr_handle* h, int32_t n, const double* x, const double* u, const double* nu, double* f,
                     double* J, double* H, void* hip_stream);
/* workspace bytes used per instance for the handle's configuration */
int64_t mr_workspace_bytes_per_instance(const mr_handle* h);

/* ---- Centerline geometry: the per-tick MPC inputs, batched (csrc/mr_track.h) --------------------
 * Replaces the host geometry the reference agent runs before every solve (agent.py:156-168,
 * 271-274): splines/ParameterizedLine.py (Gx..ddGy :19-41, x_as_coeffs/y_as_coeffs :43-64,
 * projection_local :80-97, unit_tangent/curvature/mean_curvature/unit_principal_normal :107-149)
 * and splines/ParameterizedCenterline.py (lookup_error :61-80, error_sign :82-91).
 * The track is built once on the host, as ParameterizedLine.from_waypoints (:162-178) does: knots
 * t[n_t] and B-spline coefficients cx, cy[n_c] (scipy layout, k = 3), the length L, and the lane
 * table err_left/err_right[n_rows] whose row i is s = 0.5 * i (lanes/<track>_max_error.csv;
 * n_rows = 0 with NULL tables for a lane boundary, see mr_track_lane_table).
 * All query arrays are caller-owned DEVICE pointers of length n (outputs [m][n] component-major);
 * calls are ordered on hip_stream.  One lane per query. */
typedef struct mr_track mr_track;
int mr_track_create(mr_track** tr, int32_t device, const double* t, int32_t n_t, const double* cx,
                    const double* cy, int32_t n_c, double length, const double* err_left,
                    const double* err_right, int32_t n_rows);
int mr_track_destroy(mr_track* tr);
/* out [6][n] = Gx, Gy, dGx, dGy, ddGx, ddGy at s mod L; span [n] = knot interval of G (may be NULL) */
int mr_track_eval(const mr_track* tr, int32_t n, const double* s, double* out, int32_t* span, void* hip_stream);
/* unit_tangent yaw, curvature, unit_principal_normal (nx, ny); mean_curvature over [s, s + mc_lookahead]
   (N = 10) when mean_kappa != NULL; any output may be NULL */
int mr_track_frame(const mr_track* tr, int32_t n, const double* s, double* yaw, double* kappa, double* nx,
                   double* ny, double mc_lookahead, double* mean_kappa, void* hip_stream);
/* error_sign(X, Y, s) -> +1 / -1 */
int mr_track_error_sign(const mr_track* tr, int32_t n, const double* X, const double* Y, const double* s,
                        int32_t* sign, void* hip_stream);
/* x_as_coeffs / y_as_coeffs(s, lookahead, deg = 4): cx, cy [5][n], highest order first, global s */
int mr_track_polyfit(const mr_track* tr, int32_t n, const double* s, const double* lookahead, double* cx,
                     double* cy, void* hip_stream);
/* x_as_coeffs / y_as_coeffs with the reference's deg argument (splines/ParameterizedLine.py:43-64):
   0 <= deg <= 10, cx, cy [deg + 1][n], highest order first, global s (deg 4 = mr_track_polyfit) */
int mr_track_polyfit_deg(const mr_track* tr, int32_t n, const double* s, const double* lookahead, int32_t deg,
                         double* cx, double* cy, void* hip_stream);
/* lookup_error(s, lookahead) -> err [n] (NaN where the reference raises KeyError); row_lo / row_hi /
   row_arg [n]: first / last / arg-min lane-table row (-1 on KeyError; each may be NULL) */
int mr_track_lookup_error(const mr_track* tr, int32_t n, const double* s, const double* lookahead, double* err,
                          int32_t* row_lo, int32_t* row_hi, int32_t* row_arg, void* hip_stream);
/* projection_local(X, Y, bounds = (lo, hi)) -> s [n], dist [n]; nfev [n] may be NULL */
int mr_track_projection(const mr_track* tr, int32_t n, const double* X, const double* Y, const double* lo,
                        const double* hi, double* s, double* dist, int32_t* nfev, void* hip_stream);
/* The agent's tick prep fused (agent.py:156-168 after the projection of :271-274): progress
   s = projection_local(X, Y, (lo, hi)), cx, cy = x/y_as_coeffs(s - lookback, lookahead),
   max_error = lookup_error(s, lookahead) - err_offset (agent.py: car_width / 2).  Outputs s, dist [n],
   cx, cy [5][n], max_error [n]; s0 may then feed mr_solve_batch's inputs directly. */
int mr_track_prep(const mr_track* tr, int32_t n, const double* X, const double* Y, const double* lo,
                  const double* hi, double lookback, double lookahead, double err_offset, double* s,
                  double* dist, double* cx, double* cy, double* max_error, void* hip_stream);

/* Track construction (host arrays, no device work): ParameterizedLine.from_waypoints
 * (splines/ParameterizedLine.py:162-178) -- chord-length progress, not-a-knot cubic interpolation
 * (scipy make_interp_spline, k = 3) -- with ParameterizedCenterline.from_file's closing point
 * (ParameterizedCenterline.py:93-105) when close_loop.  x, y [n]; outputs t [n + 5] (capacity),
 * cx, cy [n + 1] (capacity), *n_t = knots written (coefficients: *n_t - 4), *length = L.  The
 * result feeds mr_track_create. */
int mr_spline_from_waypoints(const double* x, const double* y, int32_t n, int32_t close_loop, double* t, double* cx,
                             double* cy, int32_t* n_t, double* length);

/* ---- lane-width table build -------------------------------------------------
 * Replaces script/make_lane_width_lookup_table.py:12-16 (Pool(14) over
 * ParameterizedCenterline.get_errors(lane, s, 0), ParameterizedCenterline.py:41-58, whose
 * lane.projection with bounds None is projection_global, ParameterizedLine.py:99-105).
 * `lane` is a lane boundary built like a track (mr_track_create with its own spline from
 * lanes/<track>_{left,right}.csv, n_rows = 0, err_* NULL).  For each centerline progress s[i]:
 * dist[i] = min over u in [0, L_lane] of |lane(u) - G(s[i])|, s_lane[i] = that u (may be NULL).
 * Deterministic global search (mr_track.h lane_distance), one wavefront per query. */
int mr_track_lane_table(const mr_track* centerline, const mr_track* lane, int32_t n, const double* s, double* dist,
                        double* s_lane, void* hip_stream);

/* ---- closed loop (agent.py:138-314 with a models/ plant in place of CARLA) ---- */

/* One tick of the agent's sensing and MPC-input preparation, per vehicle:
   progress = projection(X, Y, bounds = progress_bound(prev_progress))   agent.py:80-92, 271-273,
              ParameterizedLine.py:66-105 (NaN prev_progress or bounds wider than 5 m -> global search;
              the reference's unseeded dual_annealing is replaced by the best of the bounded Brent over
              every 5 m window, first minimum wins),
   error    = dist * error_sign(X, Y, progress)                           agent.py:274,
   cx, cy   = x/y_as_coeffs(progress - lookback, lookahead)               agent.py:156-165,
   max_error = lookup_error(progress, lookahead) - err_offset             agent.py:166-168.
   Arrays [n] (cx, cy [5][n]); prev_progress may be NULL (all global). */
int mr_agent_sense(const mr_track* tr, int32_t n, const double* X, const double* Y, const double* prev_progress,
                   double lookback, double lookahead, double err_offset, double* progress, double* error, double* cx,
                   double* cy, double* max_error, void* hip_stream);
/* One plant step per vehicle: state [6][n] = (x, y, yaw, v_x, v_y, yaw_dot), cmd [2][n] = (throttle - brake,
   steer) -> out [6][n] (may alias state).  Model.step(throttle_cmd, steer_cmd, dt) of the models/ package.
   Runs on the device that owns `state` (MR_ERR_ARG if it is not a HIP device pointer). */
int mr_plant_step(int32_t model, int32_t n, const double* state, const double* cmd, double dt, double* out,
                  void* hip_stream);

/* ---- tyre-model fitting (learning/train.py:78-192 driving learning/vehicle.py:136-205) ---------------
 * Fits the lateral tyre law of the reference's one-step torch vehicle model to logged rows by minibatch
 * gradient descent: minibatches of 64 rows (train.py BATCH_SIZE), one 64-lane wavefront per training
 * run, all epochs in one launch (csrc/mr_tyrefit.h).  Rows are structure-of-arrays [15][n]:
 * X, Y, yaw, vx, vy, yawdot, throttle, steer, dt, then the six next-state targets (train.py:32-37
 * FEATURES + TARGETS).  Parameters per set / run: linear [2] = front, back stiffness; Pacejka [18] =
 * a[0..8] front, a[0..8] back, with the vertical loads Fz [2] = front, back beside them.  The loss is
 * torch's nn.MSELoss(): the mean over rows x 6 of (prediction - target)^2; gradients are analytic in
 * the cancellation-free form.  All arrays are caller-owned DEVICE pointers; results are bitwise
 * repeatable and do not depend on how many sets / runs share a launch. */
#define MR_TYRE_LINEAR 0  /* Fy = stiffness * alpha (learning/vehicle.py:61-67)  */
#define MR_TYRE_PACEJKA 1 /* magic formula, a[0..8] (learning/vehicle.py:70-92)  */
#define MR_OPT_SGD 0      /* torch.optim.SGD                                      */
#define MR_OPT_ADAM 1     /* torch.optim.Adam (train.py's default)                */
#define MR_OPT_ADAMW 2    /* torch.optim.AdamW (decoupled weight decay)           */

typedef struct mr_tyrefit_config {
  int32_t kind;      /* MR_TYRE_* */
  int32_t optimizer; /* MR_OPT_*  */
  int32_t epochs;    /* train.py EPOCHS = 25 */
  int32_t patience;  /* ReduceLROnPlateau patience (train.py PATIENCE = 2) */
  double factor;     /* ReduceLROnPlateau factor (train.py FACTOR = 1/2)   */
  /* VehicleParameters (models/VehicleParameters.py:3-41) read by Vehicle.forward */
  double m, Iz, lf, lr, T_max, r_wheel, C_wheel, R, rho, C_d, A_f, C_roll, g, max_steer_deg;
} mr_tyrefit_config;

int mr_tyrefit_config_default(mr_tyrefit_config* cfg);
/* loss [P] and grad [P][n_par] of P parameter sets params [P][n_par], Fz [P][2] over rows [15][n].
   One wavefront per (set, chunk of 64 rows); the chunks' partial sums are added in chunk order by a second
   kernel.  The call owns the partials buffer and synchronises the stream before it returns. */
int mr_tyre_loss_grad(const mr_tyrefit_config* cfg, int32_t n, const double* rows, int32_t P, const double* params,
                      const double* Fz, double* loss, double* grad, void* hip_stream);
/* R independent training runs over train [15][n_train], validated each epoch on val [15][n_val].
   init [R][n_par], Fz [R][2], hyper [R][5] = lr, beta1, beta2, eps, weight_decay (torch's meanings; SGD
   reads lr and weight_decay).  perm: int32 [epochs][n_train], row order of every epoch (minibatch b of
   epoch e is perm[e][64 b .. 64 b + 63], the last one partial); shared by all runs when
   perm_stride_run == 0, else run r reads perm + r * perm_stride_run.  Entries are checked on the device
   before the fit starts (MR_ERR_ARG if any is outside [0, n_train); the call synchronises the stream for
   that).  End of epoch: the validation loss is the mean over minibatches of 64 of each batch's MSE, then
   ReduceLROnPlateau(mode min, factor, patience, relative threshold 1e-4, cooldown 0, eps 1e-8).
   Outputs: p_final, p_best [R][n_par] (parameters at the lowest validation loss), train_loss, val_loss,
   lr_hist [R][epochs] (lr after the scheduler's step), flag [R] = 1 when a non-finite value appeared:
   that run stopped updating, kept its last finite parameters, and its unfinished epochs are NaN.
   p_steps: optional [R][epochs * ceil(n_train / 64)][n_par], the parameters after every optimiser step
   (NaN for steps a stopped run never took); NULL to skip. */
int mr_tyre_fit(const mr_tyrefit_config* cfg, int32_t n_train, const double* train, int32_t n_val, const double* val,
                int32_t R, const double* init, const double* Fz, const double* hyper, const int32_t* perm,
                int64_t perm_stride_run, double* p_final, double* p_best, double* train_loss, double* val_loss,
                double* lr_hist, int32_t* flag, double* p_steps, void* hip_stream);

/* ---- open-loop rollouts and the fitted model as a plant (csrc/mr_rollout.h) ----------------------------
 * Which fit is good: the reference rolls a model forward along a logged drive and compares it with what
 * the car did (learning/compare.py:60, script/verify_dynamic.py, script/test_model_error.py).  The model is
 * the one-step model of the fit (learning/vehicle.py:136-205) with the tyres of mr_tyrefit_config.kind; the
 * config's optimiser fields are not read.  All arrays are caller-owned DEVICE pointers. */

/* One model step per vehicle: state [6][n], cmd [2][n] = (throttle - brake, steer) -> out [6][n] (may alias
   state).  Tyres params [P][n_par], Fz [P][2]: shared (P == 1) or one set per vehicle (P == n).  The
   model-matched plant of an MPC that carries the same tyres (control/MPC.py:186-229 with the tyre law
   swapped).  Runs on the device that owns `state`. */
int mr_vehicle_step(const mr_tyrefit_config* cfg, int32_t n, const double* state, const double* cmd, double dt,
                    int32_t P, const double* params, const double* Fz, double* out, void* hip_stream);
/* Rollouts of P parameter sets from n_start start rows over H steps along log [9][T] = X, Y, yaw, vx, vy,
   yawdot, throttle (cmd_throttle - cmd_brake), steer, ts; ts[i] is last_ts of row i, and the step from row i
   to row i + 1 uses ts[i + 1] (learning/generate_train_val_datasets.py:41-59).  Start s: x_0 = log[0..5][s],
   x_k = f(x_{k-1}, throttle[s+k-1], steer[s+k-1], ts[s+k]), error e = log[0..5][s+k] - x_k (truth minus
   prediction; yaw: the raw difference), k = 1..H.  A rollout whose x_0 or x_k is not finite stops: that step
   and its later ones contribute nothing.  stats [P][H][6][4] = sum e, sum e^2, min e, max e over the
   contributing rollouts, count [P][H] their number (count 0: sums 0, min and max NaN); pred: optional
   [P][H][6][n_start], the predictions (NaN for steps not taken), NULL to skip.  One wavefront per (set, chunk
   of 64 starts), partial sums added in chunk order: bitwise repeatable, independent of P.  start entries are
   checked on the device first (MR_ERR_ARG if any is outside [0, T - 1 - H]); the call synchronises the
   stream before it returns. */
int mr_tyre_rollout(const mr_tyrefit_config* cfg, int32_t T, const double* log, int32_t n_start, const int32_t* start,
                    int32_t H, int32_t P, const double* params, const double* Fz, double* stats, int32_t* count,
                    double* pred, void* hip_stream);

/* ---- the models/ plant with run-time parameters and its rollouts (csrc/mr_plant.h, mr_plantroll.h) ------
 * How well does the plant of the closed loop reproduce a logged drive, and which constants would do better:
 * script/verify_kinematic.py:24-41, verify_dynamic.py:26-43 and verify_blend.py:24-41 (a models/ plant rolled
 * along a drive), script/test_model_error.py (per-component error statistics) and script/optimize_coeffs.py
 * (a search over dt or (Cf, Cr) by serial rollouts).  A parameter set is MR_PLANT_NPAR doubles: the fields of
 * models/VehicleParameters.py:8-38 that the plant reads, in the order m, max_steer, T_max, r_wheel, C_wheel, R,
 * rho, C_d, A_f, C_roll, regen_brake_accel, Iz, lf, lr, Cf, Cr, g, Vblendmin, Vblendmax, then the penalty term
 * of Model.Fx (models/Model.py:50): amplitude factor (1), location (0.5), width (0.0775).  All arrays but
 * mr_plant_params_default's are caller-owned DEVICE pointers. */
#define MR_PLANT_NPAR 22

/* The class defaults of models/VehicleParameters.py:8-38 and of models/Model.py:50 (host pointer).  With
   this vector the two entries below compute bitwise what mr_plant_step computes. */
int mr_plant_params_default(double* params /* [MR_PLANT_NPAR] */);
/* mr_plant_step with parameters params [P][MR_PLANT_NPAR]: shared (P == 1) or one vector per vehicle (P == n).
   Model.step(throttle_cmd, steer_cmd, dt) with model.params set (models/Model.py:83-88; the Cf / Cr arguments of
   models/DynamicBicycleModel.py:16-28).  out may alias state.  Runs on the device that owns `state`. */
int mr_plant_step_params(int32_t model, int32_t n, const double* state, const double* cmd, double dt, int32_t P,
                         const double* params, double* out, void* hip_stream); /* P == 1 or P == n */
/* Rollouts of P parameter sets of plant `model` (MR_PLANT_*) along log [9][T] (the layout of mr_tyre_rollout),
   replacing the loops of script/verify_kinematic.py:39-41, verify_dynamic.py:41-43, verify_blend.py:39-41 and
   the objective of script/optimize_coeffs.py:34-48: x_0 = log[0..5][s], x_k = step(x_{k-1}, throttle[s+k-1],
   steer[s+k-1], dt_k), dt_k = ts[s+k], or dt[p] for every step of set p when dt is not NULL (MR_ERR_ARG if an
   entry is not a positive finite number).  Error e = log[0..5][s+k] - x_k; the yaw error is the wrapped
   difference atan2(sin d, cos d) (the plant wraps its yaw, the log's is continuous).  stats, count, pred, the
   stopping of non-finite rollouts, the start check and the synchronisation are those of mr_tyre_rollout. */
int mr_plant_rollout(int32_t model, int32_t T, const double* log, int32_t n_start, const int32_t* start, int32_t H,
                     int32_t P, const double* params, const double* dt /* [P] or NULL */, double* stats,
                     int32_t* count, double* pred, void* hip_stream);

/* ---- the PID agent and whole drives of it against the models/ plant (csrc/mr_pid.h) ---------------------
 * agent_pid.py, the controller that produced the logs the reference learns from: pure pursuit plus PD on the
 * centerline error (get_alpha / pp_delta :95-124, :211-215), a curvature-based speed target (get_target_vel
 * :126-131) with PD throttle and a brake floor of 0.5 (:217-226).  All arrays but mr_pid_gains_default's are
 * caller-owned DEVICE pointers on the track's device. */
#define MR_PID_NGAIN 8
#define MR_PID_NMEM 4
#define MR_PID_NOUT 8
#define MR_PID_NLOG 14 /* X, Y, yaw, vx, vy, yawdot (plant state), yawdot_fd, progress, error,
                          cmd_throttle, cmd_steer, cmd_brake, target_vel, kappa */
/* The tunable parameters of agent_pid.py:47-58 (host pointer): k, zeta, kP_steer, kD_steer, kP_throttle,
   kD_throttle, lookahead, vel_lookahead_factor = 1.1, 15, 0.1, 0.1, 0.82954, 1.21341, 3.0, 40. */
int mr_pid_gains_default(double* gains /* host, [MR_PID_NGAIN] */);
/* One Agent.run_step (agent_pid.py:157-237) for n vehicles: state [6][n] = (X, Y, yaw, vx, vy, yawdot) with
   body-frame velocities; mem [4][n] in/out = (prev_progress, last_error, last_throttle_error, old_yaw), NaN for
   the reference's None (first tick: global projection, yawdot_fd NaN); gains [G][8] (G == 1 or n);
   out [8][n] = (progress, error, cmd_throttle, cmd_steer, cmd_brake, target_vel, kappa, yawdot_fd), yawdot_fd
   the finite difference of :163-172 over dt.  One addition to the reference: cmd_steer is clamped to [-1, 1]
   (the range of carla.VehicleControl.steer); last_error takes the unclamped law's error.  Tracks without lane
   tables are fine. */
int mr_pid_control(const mr_track* tr, int32_t n, const double* state, double* mem, int32_t G,
                   const double* gains, double dt, double* out, void* hip_stream);
/* T ticks of agent + plant in one launch, replacing the CARLA loop around agent_pid.Agent.run_step with
   Model.step(cmd_throttle - cmd_brake, cmd_steer, dt) of plant `model` (MR_PLANT_*).  state [6][n] and mem [4][n]
   are in/out (a second call continues the drive); params [P][MR_PLANT_NPAR] (P == 1 or n); log: rows of
   MR_PID_NLOG selected by log_mask (bit r = row r), packed in row order, [popcount(log_mask)][T][n], NULL with
   log_mask 0 for none; ticks_done [n].  A vehicle whose state or command is not finite at a tick, or whose
   plant step is not, stops before that tick: its rows from there on are NaN, state and mem keep the values
   the tick started from, ticks_done is the number of ticks before it; the other vehicles do not change.
   1 <= T <= 4096 (longer drives are several calls); dt positive and finite. */
int mr_pid_drive(const mr_track* tr, int32_t model, int32_t n, int32_t T, double dt, double* state, double* mem,
                 int32_t G, const double* gains, int32_t P, const double* params, uint32_t log_mask, double* log,
                 int32_t* ticks_done, void* hip_stream);
/* The fitness of the gain-tuning GA (GA/pdGA.py:48-55) in one launch without a log: vehicle i of n (a multiple
   of K) drives segment i % K with gains row i / K of gains [n / K][8], from start [6][K] with s_start [K] as its
   first previous progress, against plant `model` with params [P][MR_PLANT_NPAR] (P == 1 or n); start, s_start
   and s_end [K] are read-only.  Every tick takes from the sensed progress what the host loop over the progress
   row took: travelled = mod(progress - s_start, L), minus L above L / 2; at the first tick k with travelled >=
   mod(s_end - s_start, L) =: need, times[i] = dt ((k - 1) + (need - a) / (c - a)), a and c the previous and the
   current travelled; inf when k is 0, when the vehicle stops first (mr_pid_drive's rule) or when T ticks do not
   reach it.  A vehicle with its time drives no further, and a wavefront ends when all its vehicles have:
   ticks_done [n] is the number of ticks driven, the crossing tick included.  1 <= T <= 4096. */
int mr_pid_segment_times(const mr_track* tr, int32_t model, int32_t n, int32_t K, int32_t T, double dt,
                         const double* start, const double* s_start, const double* s_end, const double* gains,
                         int32_t P, const double* params, double* times, int32_t* ticks_done, void* hip_stream);

/* ---- the GA's step on the device (csrc/mr_ga.h) -----------------------------------------------------------
 * GA/pdGA.py:57-91 with the rewards of GA/mpcGA.py:40-56.  The random stream is counter-based: draw j of
 * (seed, island, generation) is numpy.random.Philox(key=[seed, island], counter=[0, 0, generation,
 * 0]).random_raw()[j] (Philox4x64-10), its double (raw >> 11) * 2^-53 as numpy's Generator.random(); a draw
 * depends on nothing else. */
/* out[j] = raw draw first + j, j < count (HOST pointer; needs no GPU). */
int mr_ga_random(uint64_t seed, uint64_t island, uint64_t generation, uint64_t first, int64_t count, uint64_t* out);
/* One generation of n_island islands, one wavefront each (DEVICE pointers on the device that owns `genes`).
   Gene d of individual i of island j is genes[(j P + i) ld + col[d]] (in/out): ld the row stride in doubles,
   col the genes' distinct columns in [0, ld), NULL for 0 .. D-1 -- so the genes may be columns of wider rows,
   such as the PID gains [.][8] that mr_pid_segment_times reads, and a packed population is ld = D, col = NULL.
   times [n_island][P][K] (a non-finite time: segment not finished), avg
   [n_island][K] in/out, 2 <= P <= 64, 1 <= K <= 64, 1 <= D <= 16, 1 <= pairs, 2 pairs <= P; lo, hi [D] or NULL,
   a NaN entry for no bound.  In this order:
   1. rewards (mpcGA.py:40-56), i ascending and k ascending within i: a = avg[k]; a finite t[i][k] sets
      avg[k] = lambda_T t + (1 - lambda_T) a and adds exp(-kT (t - a)) to r[i]; an unfinished segment adds
      nothing and leaves the average (an addition: the reference's average would turn inf);
   2. roulette selection (pdGA.py:57-62): parent = the first j with u cdf[P-1] < cdf[j] (P - 1 if none), cdf the
      cumulative sum of r in index order; floor(u P) when cdf[P-1] is 0 or not finite; parents are read from the
      population as it was on entry;
   3. pair m takes draws m (3 + 4 D) + ...: parent a, parent b, crossover point 1 + floor(u (D - 1)), then the D
      mutation flags and the D mutation values of child 0 = a[:pt] ++ b[pt:], then those of child 1 = b[:pt] ++
      a[pt:] (:64-69); where flag < mutation_rate, gene += value - 0.5 (:71-76); then the clip to lo, hi;
   4. the 2 pairs lowest rewards in ascending order, ties to the lower index (NaN last), take child 0 and
      child 1 of pairs 0, 1, ... (:87);
   5. r [n_island][P]; best_r, best_idx [n_island] and best_genes [n_island][D]: the first maximum of r and
      its genes as they were on entry (:89-91).
   The island of the stream is island0 + the island's index in the call.  The reference's constants are kT = 4,
   lambda_T = 0.3, mutation_rate = 0.4 (pdGA.py:9-13). */
int mr_ga_breed(int32_t n_island, int32_t P, int32_t K, int32_t D, int32_t pairs, double* genes, int32_t ld,
                const int32_t* col /* HOST, [D] or NULL */, const double* times, double* avg, const double* lo, const double* hi, double kT, double lambda_T, double mutation_rate,
                uint64_t seed, uint64_t island0, uint64_t generation, double* r, double* best_r, int32_t* best_idx,
                double* best_genes, void* hip_stream);

/* ---- segment drives of the MPC: the fitness of the weight-tuning GA (csrc/mr_mpcseg.h) --------------------
 * GA/mpcGA.py tunes the five RuntimeControllerParameters over segments of the lap; its segment time is a random
 * placeholder (mpcGA.py:43).  Here vehicle i of n = n_ind K drives segment i % K with the runtime vector of
 * individual i / K, one tick being mr_agent_sense, mr_mpcseg_inputs, mr_solve_batch_horizons (or _warm) and
 * mr_mpcseg_apply on one stream.  A vehicle whose drive is over (done[i] != 0) gets horizon 0, which the solve
 * skips, and is not stepped.  All arrays are caller-owned DEVICE pointers; nothing synchronises.
 * mem [MR_MPCSEG_NMEM][n] = old_yaw, prev_progress (NaN: none yet, as the agent's None), cmd_throttle, cmd_steer,
 * cmd_brake, travelled_prev; row 1 is the prev_progress argument of mr_agent_sense. */
#define MR_MPCSEG_NMEM 6
/* Once per generation: runtime[d][ind K + k] = lo[d] + genes[ind][d] (hi[d] - lo[d]), genes [n_ind][5] in
   normalised units, lo, hi [5]; d_max not NaN: row 1 is d_max instead (the class attribute that the reference's
   NLP reads, control/MPC.py:50).  runtime [5][n_ind K] is mr_inputs.runtime. */
int mr_mpcseg_runtime(int32_t n_ind, int32_t K, const double* genes, const double* lo, const double* hi, double d_max,
                      double* runtime, void* hip_stream);
/* Every tick (tick = 0, 1, ...) after mr_agent_sense wrote progress [n] from state [6][n].  Vehicle i with
   done[i] != 0: horizon_out[i] = 0, nothing else written.  Otherwise, with travelled = mod(progress - s_start, L),
   minus L above L / 2, and need = mod(s_end - s_start, L) of segment i % K (s_start, s_end [K]): when travelled >=
   need, times[i] = dt ((tick - 1) + (need - a) / (travelled - a)), a = mem's travelled_prev, inf at tick 0; a
   non-finite progress gives inf; either way done[i] = 1, ticks_done[i] = tick + 1, horizon_out[i] = 0 and nothing
   else is written (times and ticks_done of a vehicle that never finishes keep the caller's values).  A vehicle
   that drives on gets state0 [8][n] = X, Y, yaw, vx, vy, the yaw rate as the wrapped difference of yaw and
   old_yaw times (1 / dt) (agent.py:240-249 as torch divides by a host scalar on the device; NaN old_yaw: NaN), cmd_brake == 0 ? cmd_throttle : -cmd_brake
   (agent.py:149), cmd_steer; with U_prev [2][N][n] (and horizon_prev [n] or NULL = N, its horizons Np),
   u_init[:, k, i] = U_prev[:, min(k + 1, Np - 1), i] (control/MPC.py:120-121; u_init and U_prev both or neither);
   horizon_out[i] = horizon_in[i], or without horizon_in N, or with hz_lookahead > 0 the reference's speed rule
   ceil((1 / (Ts max(vx, 1e-3))) hz_lookahead) clamped to [hz_min, N] (script/test_mpc.py:32-33 in the operations
   of torch's scalar / tensor; NaN speed: 0). */
int mr_mpcseg_inputs(int32_t n, int32_t K, int32_t N, int32_t tick, double dt, double L, const double* state,
                     const double* progress, const double* mem, const double* s_start, const double* s_end,
                     const double* U_prev, const int32_t* horizon_prev, const int32_t* horizon_in,
                     double hz_lookahead, double Ts, int32_t hz_min, double* state0, double* u_init,
                     int32_t* horizon_out, int32_t* done, double* times, int32_t* ticks_done, void* hip_stream);
/* Every tick after the solve.  Vehicle i with done[i] != 0 is left alone (state and mem bitwise).  Otherwise
   (throttle, steer) = U[:, 0, i] of U [2][N][n], or (0.5, 0.0) with U NULL (agent.py:283); cmd_brake = -throttle
   and cmd_throttle = 0 for a negative throttle, else 0 and throttle (agent.py:289-306); state [6][n] takes one
   step of plant `model` (MR_PLANT_*) with the command cmd_throttle - cmd_brake and the parameters params
   [P][MR_PLANT_NPAR] (P == 1 or n; NULL with P = 0: the defaults) as mr_plant_step_params computes it; mem takes
   the yaw before the step, this tick's progress, the three commands and this tick's travelled. */
int mr_mpcseg_apply(int32_t model, int32_t n, int32_t K, int32_t N, double dt, double L, double* state, double* mem,
                    const double* progress, const double* s_start, const int32_t* done, const double* U, int32_t P,
                    const double* params, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* MPCRACING_H */
