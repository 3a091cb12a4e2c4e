// The glue of the MPC's segment drives (mpcracing/mpc.py): what the batched closed loop of the weight-tuning GA
// (GA/mpcGA.py) does per vehicle around the library's sensing and solve launches, as three kernels -- the
// population's runtime vectors once per generation, the solve's inputs and the segment's crossing test every
// tick after mr_agent_sense, the applied command and one plant step every tick after the solve.  fp64,
// host + gfx950, one lane per vehicle, no cross-lane step.  Expressions keep the order of the torch glue in
// mpcracing/closed_loop.py (_tick) and of ga.crossing_times, bit for bit (no FP contraction).
//
// A vehicle whose drive is over (done[i] != 0: it crossed its segment's end, or its progress is not finite)
// leaves mr_mpcseg_inputs with horizon 0 -- the value that mr_solve_batch_horizons does not solve -- and is
// not touched by mr_mpcseg_apply: its state and memory stay those of the tick at which it finished.
#pragma once
#include "mr_track.h"
#include "mr_plantroll.h"

namespace mr {

#ifndef MR_MPCSEG_NMEM
#define MR_MPCSEG_NMEM 6
#endif
// rows of mem [MR_MPCSEG_NMEM][n]
#define MR_MS_OLD_YAW 0
#define MR_MS_PREV_PROGRESS 1
#define MR_MS_CMD_THROTTLE 2
#define MR_MS_CMD_STEER 3
#define MR_MS_CMD_BRAKE 4
#define MR_MS_TRAVELLED_PREV 5

// ---- runtime vectors of a population: runtime[d][ind K + k] = lo[d] + genes[ind][d] (hi[d] - lo[d]) ----
inline const char* mpcseg_runtime_check(int64_t n_ind, int64_t K) {
  if (n_ind < 0) return "n_ind < 0";
  if (K < 1) return "K < 1";
  if (n_ind * K > (int64_t)0x7fffffff / 8) return "too many vehicles";
  return nullptr;
}
// vehicle j of n_ind K; d_max NaN: row 1 is mapped like the others
MR_HD void mpcseg_runtime_vehicle(int n_ind, int K, int j, const double* genes, const double* lo, const double* hi,
                                  double d_max, double* runtime) {
  const int64_t n = (int64_t)n_ind * K;
  const double* g = genes + (int64_t)(j / K) * 5;
  for (int d = 0; d < 5; ++d) runtime[d * n + j] = lo[d] + g[d] * (hi[d] - lo[d]);
  if (d_max == d_max) runtime[n + j] = d_max;
}

// travelled of ga.crossing_times: the distance along the lap from the segment's start, negative just behind it
MR_HD double mpcseg_travelled(double progress, double s_start, double L) {
  const double tr = py_mod(progress - s_start, L);
  return tr > 0.5 * L ? tr - L : tr;
}

// ---- every tick after mr_agent_sense ----
struct MpcSegInputsArgs {
  int n, K, N, tick, hz_min;
  double dt, L, hz_lookahead, Ts;
  const double* state;        // [6][n]
  const double* progress;     // [n] this tick's sensed progress
  const double* mem;          // [MR_MPCSEG_NMEM][n], read only
  const double* s_start;      // [K]
  const double* s_end;        // [K]
  const double* U_prev;       // [2][N][n] or null
  const int32_t* horizon_prev;  // [n] the horizons of U_prev, or null (N)
  const int32_t* horizon_in;  // [n] or null (N, or the speed rule when hz_lookahead > 0)
  double* state0;             // [8][n]
  double* u_init;             // [2][N][n], with U_prev
  int32_t* horizon_out;       // [n]
  int32_t* done;              // [n] in/out
  double* times;              // [n]
  int32_t* ticks_done;        // [n]
};
inline const char* mpcseg_inputs_check(int64_t n, int64_t K, int64_t N, int64_t tick, double dt, double L,
                                       double hz_lookahead, double Ts, int64_t hz_min, const void* horizon_in,
                                       const void* U_prev, const void* u_init) {
  if (n < 0) return "n < 0";
  if (K < 1) return "K < 1";
  if (N < 1 || N > 4096) return "N out of range (1..4096)";
  if (n > (int64_t)0x7fffffff / (2 * N) || n > (int64_t)0x7fffffff / 8) return "too many vehicles";
  if (tick < 0) return "tick < 0";
  if (!plant_dt_ok(dt)) return "dt must be a positive finite number";
  if (!(L > 0.0 && L < INFINITY)) return "L must be a positive finite number";
  if (hz_lookahead > 0.0) {
    if (horizon_in) return "horizon_in and the speed rule (hz_lookahead > 0) exclude each other";
    if (!(Ts > 0.0 && Ts < INFINITY)) return "Ts must be a positive finite number";
    if (hz_min < 1 || hz_min > N) return "hz_min must be in 1..N";
  }
  if ((U_prev != nullptr) != (u_init != nullptr)) return "U_prev and u_init must both be given or both be null";
  return nullptr;
}

MR_HD void mpcseg_inputs_vehicle(const MpcSegInputsArgs& A, int i) {
  const int64_t n = A.n;
  if (A.done[i]) {
    A.horizon_out[i] = 0;
    return;
  }
  // the crossing test of ga.crossing_times on this tick's progress
  const int seg = i % A.K;
  const double s_start = A.s_start[seg];
  const double progress = A.progress[i];
  const double need = py_mod(A.s_end[seg] - s_start, A.L);
  const double c = mpcseg_travelled(progress, s_start, A.L);
  const bool lost = !tf_finite(progress);
  if (lost || c >= need) {
    double tm = INFINITY;
    if (!lost && A.tick > 0) {
      const double a = A.mem[(int64_t)MR_MS_TRAVELLED_PREV * n + i];
      tm = A.dt * ((double)(A.tick - 1) + (need - a) / (c - a));
    }
    A.times[i] = tm;
    A.ticks_done[i] = A.tick + 1;
    A.done[i] = 1;
    A.horizon_out[i] = 0;
    return;
  }
  // the solve's inputs (closed_loop.py _tick; agent.py:149, 240-249)
  const double yaw = A.state[2 * n + i], vx = A.state[3 * n + i];
  const double old_yaw = A.mem[(int64_t)MR_MS_OLD_YAW * n + i];
  double d = yaw - old_yaw;
  if (d > 3) d = yaw - (old_yaw + 3.141592653589793 * 2);
  else if (d < -3) d = yaw - (old_yaw - 3.141592653589793 * 2);
  // the torch glue divides by the host scalar dt on the device, which torch evaluates as the product with
  // 1 / dt; likewise its scalar / tensor of the speed rule below is reciprocal(tensor) * scalar
  const double yawdot = d * (1.0 / A.dt);
  const double cmd_throttle = A.mem[(int64_t)MR_MS_CMD_THROTTLE * n + i];
  const double cmd_brake = A.mem[(int64_t)MR_MS_CMD_BRAKE * n + i];
  const double thr0 = cmd_brake == 0 ? cmd_throttle : -cmd_brake;
  A.state0[0 * n + i] = A.state[0 * n + i];
  A.state0[1 * n + i] = A.state[1 * n + i];
  A.state0[2 * n + i] = yaw;
  A.state0[3 * n + i] = vx;
  A.state0[4 * n + i] = A.state[4 * n + i];
  A.state0[5 * n + i] = yawdot;
  A.state0[6 * n + i] = thr0;
  A.state0[7 * n + i] = A.mem[(int64_t)MR_MS_CMD_STEER * n + i];
  if (A.U_prev) {  // the shifted controls across a changed horizon (MPC.py:120-121)
    int Np = A.horizon_prev ? A.horizon_prev[i] : A.N;
    Np = Np < 1 ? 1 : (Np > A.N ? A.N : Np);
    for (int k = 0; k < A.N; ++k) {
      const int kp = k + 1 < Np - 1 ? k + 1 : Np - 1;
      for (int r = 0; r < 2; ++r)
        A.u_init[((int64_t)r * A.N + k) * n + i] = A.U_prev[((int64_t)r * A.N + kp) * n + i];
    }
  }
  int hz = A.N;
  if (A.horizon_in) {
    hz = A.horizon_in[i];
  } else if (A.hz_lookahead > 0.0) {  // script/test_mpc.py:32-33 as closed_loop.py clamps it; NaN speed: no solve
    const double v = vx < 1e-3 ? 1e-3 : vx;
    double h = ceil((1.0 / (A.Ts * v)) * A.hz_lookahead);
    h = h < (double)A.hz_min ? (double)A.hz_min : h;
    h = h > (double)A.N ? (double)A.N : h;
    hz = h == h ? (int)h : 0;
  }
  A.horizon_out[i] = hz;
}

// ---- every tick after the solve ----
struct MpcSegApplyArgs {
  int model, n, K, N, P;
  double dt, L;
  double* state;           // [6][n] in/out
  double* mem;             // [MR_MPCSEG_NMEM][n] in/out
  const double* progress;  // [n]
  const double* s_start;   // [K]
  const int32_t* done;     // [n]
  const double* U;         // [2][N][n] or null: (0.5, 0.0)
  const double* params;    // [P][MR_PLANT_NPAR] or null: the defaults
};
inline const char* mpcseg_apply_check(int64_t model, int64_t n, int64_t K, int64_t N, double dt, double L, int64_t P,
                                      const void* params) {
  if (model < PLANT_KIN || model > PLANT_BLEND) return "unknown plant model";
  if (n < 0) return "n < 0";
  if (K < 1) return "K < 1";
  if (N < 1 || N > 4096) return "N out of range (1..4096)";
  if (n > (int64_t)0x7fffffff / (2 * N) || n > (int64_t)0x7fffffff / 8) return "too many vehicles";
  if (!plant_dt_ok(dt)) return "dt must be a positive finite number";
  if (!(L > 0.0 && L < INFINITY)) return "L must be a positive finite number";
  if (params ? (P != 1 && P != n) : P != 0)
    return "P must be 1 (shared parameters) or n (one vector per vehicle), 0 with null params";
  return nullptr;
}

MR_HD void mpcseg_apply_vehicle(const MpcSegApplyArgs& A, int i) {
  if (A.done[i]) return;
  const int64_t n = A.n;
  // agent.py:283 before the first solve, then the first control; carla.VehicleControl: negative throttle is
  // brake (agent.py:289-306)
  const double throttle = A.U ? A.U[i] : 0.5;
  const double steer = A.U ? A.U[(int64_t)A.N * n + i] : 0.0;
  const double cmd_brake = throttle < 0 ? -throttle : 0.0;
  const double cmd_throttle = throttle < 0 ? 0.0 : throttle;
  double qd[MR_PLANT_NPAR];
  const double* q = qd;
  if (A.params) q = A.params + (int64_t)(A.P == 1 ? 0 : i) * MR_PLANT_NPAR;
  else plant_params_default(qd);
  double x[6], o[6];
  for (int c = 0; c < 6; ++c) x[c] = A.state[(int64_t)c * n + i];
  plant_step(A.model, q, x, cmd_throttle - cmd_brake, steer, A.dt, o);  // models/Model.py:83-88
  for (int c = 0; c < 6; ++c) A.state[(int64_t)c * n + i] = o[c];
  const double progress = A.progress[i];
  A.mem[(int64_t)MR_MS_OLD_YAW * n + i] = x[2];
  A.mem[(int64_t)MR_MS_PREV_PROGRESS * n + i] = progress;
  A.mem[(int64_t)MR_MS_CMD_THROTTLE * n + i] = cmd_throttle;
  A.mem[(int64_t)MR_MS_CMD_STEER * n + i] = steer;
  A.mem[(int64_t)MR_MS_CMD_BRAKE * n + i] = cmd_brake;
  A.mem[(int64_t)MR_MS_TRAVELLED_PREV * n + i] = mpcseg_travelled(progress, A.s_start[i % A.K], A.L);
}

}  // namespace mr
