// The reference's second controller (agent_pid.py): pure pursuit plus PD on the centerline error for the
// steering, a curvature-based speed target with PD throttle, and a brake floor of 0.5 -- the agent that drove
// every log the reference learns from.  One tick (agent_pid.Agent.run_step, :157-237, without the CARLA
// plumbing) and a whole drive of that tick against the models/ plant (mr_plant.h, run-time parameters), fp64,
// host + gfx950, one lane per vehicle.  Expressions keep the order of the Python source; sensing is
// mr_agent.h / mr_track.h, bit for bit between the two builds (no FP contraction).
#pragma once
#include "mr_agent.h"
#include "mr_plantroll.h"

namespace mr {

#ifndef MR_PID_NGAIN
#define MR_PID_NGAIN 8
#define MR_PID_NMEM 4
#define MR_PID_NOUT 8
#define MR_PID_NLOG 14
#endif
#define MR_PID_T_MAX 4096

// gains: k, zeta, kP_steer, kD_steer, kP_throttle, kD_throttle, lookahead, vel_lookahead_factor (agent_pid.py:47-58)
MR_HD void pid_gains_default(double* g) {
  g[0] = 1.1; g[1] = 15; g[2] = 0.1; g[3] = 0.1; g[4] = 0.82954; g[5] = 1.21341; g[6] = 3.0; g[7] = 40;
}

// numpy.clip(v, lo, hi) = minimum(maximum(v, lo), hi); a NaN v stays NaN
MR_HD double pid_clip(double v, double lo, double hi) {
  v = v < lo ? lo : v;
  return v > hi ? hi : v;
}

// One run_step.  x = (X, Y, yaw, vx, vy, yawdot) with the body-frame velocities the agent derives (:185-186);
// mem = (prev_progress (NaN = None), last_error, last_throttle_error, old_yaw (NaN = None)), updated in place;
// out = (progress, error, cmd_throttle, cmd_steer, cmd_brake, target_vel, kappa, yawdot_fd).
// The one addition to the reference: cmd_steer is clamped to [-1, 1], the range of carla.VehicleControl.steer
// (the plant has no clamp of its own); last_error takes the error of the unclamped law, as in the reference.
MR_HD void pid_control(const TrackView& T, const double* x, double* mem, const double* g, double dt, double* out) {
  const double X = x[0], Y = x[1], yaw = x[2];
  // :163-172, old_yaw None -> yawdot None: every comparison with NaN is false and NaN / dt is NaN
  const double old_yaw = mem[3];
  double yawdot;
  if (yaw - old_yaw > 3) yawdot = (yaw - (old_yaw + 3.141592653589793 * 2)) / dt;
  else if (yaw - old_yaw < -3) yawdot = (yaw - (old_yaw - 3.141592653589793 * 2)) / dt;
  else yawdot = (yaw - old_yaw) / dt;
  const double vel = sqrt(x[3] * x[3] + x[4] * x[4]);  // :187
  // :204-205
  const double progress = agent_projection(T, X, Y, mem[0]);
  const double error = track_dist(T, progress, X, Y) * (double)track_error_sign(T, X, Y, progress);
  // get_alpha / pp_delta (:95-124)
  const double lookahead = g[6];
  const double ml = py_mod(progress + lookahead, T.L), mp = py_mod(progress, T.L);
  const double tx = spline_eval(T.x[0], ml) - spline_eval(T.x[0], mp);
  const double ty = spline_eval(T.y[0], ml) - spline_eval(T.y[0], mp);
  const double c = cos(-yaw), s = sin(-yaw);
  const double lx = tx * c - ty * s;
  const double ly = tx * s + ty * c;
  const double alpha = atan2(ly, lx);
  const double delta = atan2(2 * 2.87 * sin(alpha), lookahead);
  const double steer = delta + error * g[2] + (mem[1] - error) * g[3];  // :211-215
  // :217-226; get_target_vel (:126-131) keeps the reference's quirk: the lower clip bound is the look-ahead
  const double vel_lookahead = vel * vel / g[7];
  const double lower = pid_clip(progress + g[1], vel_lookahead, 10000);
  const double kappa = track_mean_curvature(T, lower, vel_lookahead);
  const double target_vel = pid_clip(g[0] * sqrt(9.81 / kappa), 10, 100);  // kappa == 0: inf -> 100
  const double te = target_vel - vel;
  double throttle = pid_clip(te * g[4] + (te - mem[2]) * g[5], -1, 1);
  double brake = 0;
  if (throttle < 0) {
    brake = pid_clip(-throttle, 0.5, 1);
    throttle = 0;
  }
  mem[0] = progress; mem[1] = error; mem[2] = te; mem[3] = yaw;
  out[0] = progress; out[1] = error; out[2] = throttle; out[3] = pid_clip(steer, -1, 1); out[4] = brake;
  out[5] = target_vel; out[6] = kappa; out[7] = yawdot;
}

// One tick of vehicle i of n: state [6][n], mem [4][n] in/out, gains [G][8] (G == 1 or n), out [8][n]
MR_HD void pid_control_vehicle(const TrackView& T, int n, int i, const double* state, double* mem, int G,
                               const double* gains, double dt, double* out) {
  const double* gp = gains + (int64_t)(G == 1 ? 0 : i) * MR_PID_NGAIN;
  double x[6], m[MR_PID_NMEM], g[MR_PID_NGAIN], o[MR_PID_NOUT];
  for (int c = 0; c < 6; ++c) x[c] = state[(int64_t)c * n + i];
  for (int c = 0; c < MR_PID_NMEM; ++c) m[c] = mem[(int64_t)c * n + i];
  for (int c = 0; c < MR_PID_NGAIN; ++c) g[c] = gp[c];
  pid_control(T, x, m, g, dt, o);
  for (int c = 0; c < MR_PID_NMEM; ++c) mem[(int64_t)c * n + i] = m[c];
  for (int c = 0; c < MR_PID_NOUT; ++c) out[(int64_t)c * n + i] = o[c];
}

struct PidDriveArgs {
  int n, T, G, P;
  double dt;
  double* state;         // [6][n] in/out
  double* mem;           // [4][n] in/out
  const double* gains;   // [G][8]
  const double* params;  // [P][MR_PLANT_NPAR]
  uint32_t log_mask;     // bit r: row r of MR_PID_NLOG is kept
  double* log;           // [popcount(log_mask)][T][n]
  int32_t* ticks_done;   // [n]
};
inline PidDriveArgs make_pid_drive_args(int n, int T, double dt, double* state, double* mem, int G,
                                        const double* gains, int P, const double* params, uint32_t log_mask,
                                        double* log, int32_t* ticks_done) {
  return PidDriveArgs{n, T, G, P, dt, state, mem, gains, params, log_mask, log, ticks_done};
}

// the tests a drive and a segment timing share, in the order both make them
inline const char* pid_vehicles_check(int64_t model, int64_t n) {
  if (model < PLANT_KIN || model > PLANT_BLEND) return "unknown plant model";
  if (n < 0) return "n < 0";
  if (n > (int64_t)0x7fffffff / MR_PID_NLOG) return "too many vehicles";
  return nullptr;
}
inline const char* pid_ticks_check(int64_t T, double dt, const char* too_many) {
  if (T < 1) return "T < 1";
  if (T > MR_PID_T_MAX) return too_many;
  if (!plant_dt_ok(dt)) return "dt must be a positive finite number";
  return nullptr;
}

inline const char* pid_control_check(int64_t n, int64_t G, double dt) {
  if (n < 0) return "n < 0";
  if (n > (int64_t)0x7fffffff / MR_PID_NOUT) return "too many vehicles";
  if (G != 1 && G != n) return "G must be 1 (shared gains) or n (one vector per vehicle)";
  if (!plant_dt_ok(dt)) return "dt must be a positive finite number";
  return nullptr;
}
inline const char* pid_drive_check(int64_t model, int64_t n, int64_t T, double dt, int64_t G, int64_t P,
                                   uint32_t log_mask, const void* log) {
  if (const char* e = pid_vehicles_check(model, n)) return e;
  if (const char* e = pid_ticks_check(T, dt, "T > 4096 (a longer drive is several calls)")) return e;
  if (G != 1 && G != n) return "G must be 1 (shared gains) or n (one vector per vehicle)";
  if (P != 1 && P != n) return "P must be 1 (shared parameters) or n (one vector per vehicle)";
  if (log_mask >> MR_PID_NLOG) return "log_mask has bits at or above MR_PID_NLOG";
  if ((log_mask != 0) != (log != nullptr)) return "log and log_mask must both be given or both be empty";
  return nullptr;
}

// The vote that ends a drive's loop: the host build runs one lane at a time
struct PidVoteLane {
  MR_HD bool operator()(bool alive) const { return alive; }
};

// The loop of every drive: up to T ticks of pid_control -> plant_step<MODEL>(q, x, cmd_throttle - cmd_brake,
// cmd_steer, dt) from state x and memory m, which stay in registers across the ticks, as do the gains g; q points
// at the vehicle's parameters (the caller's registers when they are shared).  A vehicle whose state, command or
// next state is not finite stops before that tick: x and m keep the values the tick started from.  Per tick,
// after that test and before x and m take the tick's result, hook(t, alive, x, o) sees the state the tick
// started from and the agent's outputs; when it returns true the vehicle is finished after this tick (which
// still counts).  any_alive(alive) is true while some lane of the wave still drives (the only cross-lane step).
// Returns the number of ticks driven; *t_end (when given) is the tick at which the loop ended.
template <int MODEL, class Vote, class Hook>
MR_HD int pid_loop(const TrackView& Tr, const double* q, const double* g, double dt, int T, bool active, double* x,
                   double* m, const Vote& any_alive, Hook&& hook, int* t_end) {
  bool alive = active;
  int done = 0;
  int t = 0;
  for (; t < T; ++t) {
    if (!any_alive(alive)) break;
    double mn[MR_PID_NMEM], o[MR_PID_NOUT], xn[6];
    for (int c = 0; c < MR_PID_NMEM; ++c) mn[c] = m[c];
    pid_control(Tr, x, mn, g, dt, o);
    plant_step<MODEL>(q, x, o[2] - o[4], o[3], dt, xn);
    bool ok = tf_finite(o[2]) && tf_finite(o[3]) && tf_finite(o[4]);
    for (int c = 0; c < 6; ++c) ok = ok && tf_finite(x[c]) && tf_finite(xn[c]);
    alive = alive && ok;
    const bool finished = hook(t, alive, x, o);
    for (int c = 0; c < 6; ++c) x[c] = alive ? xn[c] : x[c];
    for (int c = 0; c < MR_PID_NMEM; ++c) m[c] = alive ? mn[c] : m[c];
    done += alive ? 1 : 0;
    alive = alive && !finished;
  }
  if (t_end) *t_end = t;
  return done;
}

// T ticks of vehicle i with the tick's rows stored as log[row][t][i]: the rows of a stopped vehicle are NaN from
// the tick at which it stopped, ticks_done is the number of ticks before it; idle lanes (active false) store
// nothing.
template <int MODEL, class Vote>
MR_HD void pid_drive_vehicle(const TrackView& Tr, const PidDriveArgs& A, int i, bool active, const double* q,
                             const Vote& any_alive) {
  const int n = A.n;
  const int iv = active ? i : 0;  // idle lanes of the last wave follow vehicle 0 and never store
  const double* gp = A.gains + (int64_t)(A.G == 1 ? 0 : iv) * MR_PID_NGAIN;
  double x[6], m[MR_PID_NMEM], g[MR_PID_NGAIN];
  for (int c = 0; c < 6; ++c) x[c] = A.state[(int64_t)c * n + iv];
  for (int c = 0; c < MR_PID_NMEM; ++c) m[c] = A.mem[(int64_t)c * n + iv];
  for (int c = 0; c < MR_PID_NGAIN; ++c) g[c] = gp[c];
  int t;
  const int done = pid_loop<MODEL>(
      Tr, q, g, A.dt, A.T, active, x, m, any_alive,
      [&](int tick, bool live, const double* xs, const double* o) {
        if (active && A.log_mask) {
          double* lp = A.log + (int64_t)tick * n + i;
          const int64_t row = (int64_t)A.T * n;
#pragma unroll
          for (int r = 0; r < MR_PID_NLOG; ++r) {  // the mask is wave-uniform
            if (!((A.log_mask >> r) & 1u)) continue;
            const double v = r < 6 ? xs[r] : (r == 6 ? o[7] : o[r - 7]);
            *lp = live ? v : NAN;
            lp += row;
          }
        }
        return false;
      },
      &t);
  if (!active) return;
  for (; t < A.T && A.log_mask; ++t) {  // the loop ended early: every lane of the wave had stopped
    double* lp = A.log + (int64_t)t * n + i;
    for (int r = 0; r < MR_PID_NLOG; ++r) {
      if (!((A.log_mask >> r) & 1u)) continue;
      *lp = NAN;
      lp += (int64_t)A.T * n;
    }
  }
  for (int c = 0; c < 6; ++c) A.state[(int64_t)c * n + i] = x[c];
  for (int c = 0; c < MR_PID_NMEM; ++c) A.mem[(int64_t)c * n + i] = m[c];
  A.ticks_done[i] = done;
}

// ---- segment times fused into the drive: the fitness of the gain-tuning GA (GA/pdGA.py:48-55) ----
struct PidSegArgs {
  int n, T, K, P;
  double dt;
  const double* start;    // [6][K] start state of every segment (read-only: every generation reuses it)
  const double* s_start;  // [K] the first previous progress
  const double* s_end;    // [K]
  const double* gains;    // [n / K][8]
  const double* params;   // [P][MR_PLANT_NPAR]
  double* times;          // [n]
  int32_t* ticks_done;    // [n]
};
inline PidSegArgs make_pid_seg_args(int n, int K, int T, double dt, const double* start, const double* s_start,
                                    const double* s_end, const double* gains, int P, const double* params,
                                    double* times, int32_t* ticks_done) {
  return PidSegArgs{n, T, K, P, dt, start, s_start, s_end, gains, params, times, ticks_done};
}

inline const char* pid_segment_check(int64_t model, int64_t n, int64_t K, int64_t T, double dt, int64_t P) {
  if (const char* e = pid_vehicles_check(model, n)) return e;
  if (K < 1) return "K < 1";
  if (n % K != 0) return "n must be a multiple of K (vehicle i drives segment i % K with gains row i / K)";
  if (const char* e = pid_ticks_check(T, dt, "T > 4096")) return e;
  if (P != 1 && P != n) return "P must be 1 (shared parameters) or n (one vector per vehicle)";
  return nullptr;
}

// The drive of pid_loop without a log: vehicle i starts segment i % K with gains row i / K, and every tick
// takes from its sensed progress what ga.crossing_times takes from the progress row: travelled =
// py_mod(progress - s_start, L), minus L above L / 2; at the first tick k with travelled >= need =
// py_mod(s_end - s_start, L) the time is dt ((k - 1) + (need - a) / (c - a)), a and c the previous and the
// current travelled; inf when k is 0; a NaN progress never hits.  A vehicle that has its time or has stopped (the
// drive's rule) is finished; the loop ends when every lane of the wave is.  ticks_done: the ticks driven, the
// crossing tick included.
template <int MODEL, class Vote>
MR_HD void pid_segment_vehicle(const TrackView& Tr, const PidSegArgs& A, int i, bool active, const double* q,
                               const Vote& any_alive) {
  const int iv = active ? i : 0;  // idle lanes of the last wave follow vehicle 0 and never store
  const int K = A.K, seg = iv % K;
  const double* gp = A.gains + (int64_t)(iv / K) * MR_PID_NGAIN;
  double x[6], m[MR_PID_NMEM], g[MR_PID_NGAIN];
  for (int c = 0; c < 6; ++c) x[c] = A.start[(int64_t)c * K + seg];
  const double s_start = A.s_start[seg];
  m[0] = s_start; m[1] = 0; m[2] = 0; m[3] = NAN;
  for (int c = 0; c < MR_PID_NGAIN; ++c) g[c] = gp[c];
  const double L = Tr.L, need = py_mod(A.s_end[seg] - s_start, L);
  double tm = INFINITY, prev = 0;
  const int done = pid_loop<MODEL>(
      Tr, q, g, A.dt, A.T, active, x, m, any_alive,
      [&](int tick, bool live, const double*, const double* o) {
        double tr = py_mod(o[0] - s_start, L);
        tr = tr > 0.5 * L ? tr - L : tr;
        const bool hit = live && tr >= need;
        if (hit && tick > 0) tm = A.dt * ((double)(tick - 1) + (need - prev) / (tr - prev));
        prev = tr;
        return hit;
      },
      nullptr);
  if (!active) return;
  A.times[i] = tm;
  A.ticks_done[i] = done;
}

}  // namespace mr
