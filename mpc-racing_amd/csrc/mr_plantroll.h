// Open-loop rollouts of the models/ plant (mr_plant.h, run-time parameters) along a logged drive, their
// error statistics, and the parameterised plant step (script/verify_kinematic.py, verify_dynamic.py,
// verify_blend.py, script/test_model_error.py; the objective of script/optimize_coeffs.py), fp64,
// host + gfx950.
//
// Shape, wave body and statistics are those of mr_rollout.h (ro_chunk, RoArgs, rollout_check, ro_reduce_lds,
// ro_finish); this file holds what is the plant's own: the rollout model RoPlantModel, the test of a fixed
// step and the parameterised plant step.  A lane with start s sets x_0 = log[0..5][s] and iterates
// x_k = plant_step<MODEL>(q, x_{k-1}, throttle[s+k-1], steer[s+k-1], dt_k), k = 1..H, with dt_k = ts[s+k]
// or, when dt is given, the set's fixed dt[p] (verify_*.py use the log's mean dt, optimize_coeffs.py
// searches it).  Its error at step k is e = log[0..5][s+k] - x_k, except the yaw: the plant wraps its yaw
// (atan2(sin, cos)) and the loader unwraps the log's, so the yaw error is the wrapped difference
// atan2(sin d, cos d), d = truth - prediction.
//
// The set's MR_PLANT_NPAR parameters are read once per wave, before any store, from an address that is
// the same in every lane: scalar loads, the vector in SGPRs for the whole rollout.
#pragma once
#include "mr_plant.h"
#include "mr_rollout.h"

namespace mr {

inline const char* plant_rollout_check(int64_t model, int64_t T, int64_t n_start, int64_t H, int64_t P) {
  if (model < PLANT_KIN || model > PLANT_BLEND) return "unknown plant model";
  return rollout_check(T, n_start, H, P);
}
// a fixed step must be a positive finite number
MR_HD bool plant_dt_ok(double dt) { return dt > 0.0 && dt < INFINITY; }

// plant_step<MODEL> with the set's parameters and optional fixed step (RoArgs::per_set: dt [P] or null) as a
// rollout model (mr_rollout.h ro_chunk)
template <int MODEL>
struct RoPlantModel {
  static constexpr bool wrap_yaw = true;  // the plant's yaw is in (-pi, pi], the log's is continuous
  double q[MR_PLANT_NPAR];
  bool fixed_dt;
  double dt_p;
  MR_HD RoPlantModel(const RoArgs& A, int p) {
    for (int j = 0; j < MR_PLANT_NPAR; ++j) q[j] = A.params[(int64_t)p * MR_PLANT_NPAR + j];
    fixed_dt = A.per_set != nullptr;
    dt_p = fixed_dt ? A.per_set[p] : 0.0;
  }
  MR_HD void step(const double* x, const RoStep& s, double* o) const {
    plant_step<MODEL>(q, x, s.thr, s.steer, fixed_dt ? dt_p : s.ts, o);
  }
};

// One plant step of vehicle i: state [6][n], cmd [2][n] -> out [6][n] (may alias state: a lane reads its own
// column before it writes it); parameters shared (P == 1) or one vector per vehicle (P == n).
MR_HD void pr_vehicle_step(int model, int n, int i, const double* state, const double* cmd, double dt, int P,
                           const double* params, double* out) {
  const double* q = params + (int64_t)(P == 1 ? 0 : i) * MR_PLANT_NPAR;
  double x[6], o[6];
  for (int c = 0; c < 6; ++c) x[c] = state[(int64_t)c * n + i];
  plant_step(model, q, x, cmd[i], cmd[(int64_t)n + i], dt, o);
  for (int c = 0; c < 6; ++c) out[(int64_t)c * n + i] = o[c];
}

inline const char* plant_step_params_check(int64_t model, int64_t n, int64_t P) {
  if (model < PLANT_KIN || model > PLANT_BLEND) return "unknown plant model";
  if (n < 0) return "n < 0";
  if (n > (int64_t)0x7fffffff / 6) return "too many vehicles";
  if (P != 1 && P != n) return "P must be 1 (shared parameters) or n (one vector per vehicle)";
  return nullptr;
}

}  // namespace mr
