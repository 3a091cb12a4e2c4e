// Open-loop rollouts of the models/ plant (mr_plant.h, run-time parameters) along a logged drive, their
// error statistics, and the parameterised plant step (script/verify_kinematic.py, verify_dynamic.py,
// verify_blend.py, script/test_model_error.py; the objective of script/optimize_coeffs.py), fp64,
// host + gfx950.
//
// Shape and statistics are those of mr_rollout.h: one 64-lane wavefront per (parameter set, chunk of 64
// start rows), one lane per start, the log [9][T] of RO_NLOG rows, the 25 per-step values reduced by
// ro_reduce_lds into per-chunk partials that ro_finish adds in chunk order (no atomics: bitwise repeatable,
// independent of how many sets share a launch).  A lane with start s sets x_0 = log[0..5][s] and iterates
// x_k = plant_step<MODEL>(q, x_{k-1}, throttle[s+k-1], steer[s+k-1], dt_k), k = 1..H, with dt_k = ts[s+k]
// or, when dt is given, the set's fixed dt[p] (verify_*.py use the log's mean dt, optimize_coeffs.py
// searches it).  Its error at step k is e = log[0..5][s+k] - x_k, except the yaw: the plant wraps its yaw
// (atan2(sin, cos)) and the loader unwraps the log's, so the yaw error is the wrapped difference
// atan2(sin d, cos d), d = truth - prediction.  A lane whose x_0 or x_k is not finite stops: that step and
// its later ones contribute nothing.
//
// The set's MR_PLANT_NPAR parameters are read once per wave, before any store, from an address that is
// the same in every lane: scalar loads, the vector in SGPRs for the whole rollout.
#pragma once
#include "mr_plant.h"
#include "mr_rollout.h"

namespace mr {

struct PrArgs {
  int T, n_start, H, n_chunk;
  const double* log;     // [9][T]
  const int32_t* start;  // [n_start], every entry in [0, T - 1 - H] (checked before the launch)
  const double* params;  // [P][MR_PLANT_NPAR]
  const double* dt;      // [P] or null: ts of the log
  double* partials;      // [sets of the launch][n_chunk][H][25]
  double* pred;          // optional [P][H][6][n_start]
};

inline const char* plant_rollout_check(int64_t model, int64_t T, int64_t n_start, int64_t H, int64_t P) {
  if (model < PLANT_KIN || model > PLANT_BLEND) return "unknown plant model";
  if (T < 2) return "T < 2";
  if (T > (int64_t)0x7fffffff / RO_NLOG) return "too many log rows";
  if (n_start < 1) return "n_start < 1";
  if (H < 1) return "H < 1";
  if (H > T - 1) return "H exceeds T - 1";
  if (P < 1) return "P < 1";
  if (P * ((n_start + WL - 1) / WL) > (int64_t)0x7fffffff) return "P * ceil(n_start / 64) exceeds the grid limit";
  return nullptr;
}
// a fixed step must be a positive finite number
MR_HD bool plant_dt_ok(double dt) { return dt > 0.0 && dt < INFINITY; }

template <int MODEL>
MR_WV_FN void pr_chunk(const PrArgs& A, int p, int pl, int chunk, double* lds, const Wv& w) {
  double q[MR_PLANT_NPAR];
  for (int j = 0; j < MR_PLANT_NPAR; ++j) q[j] = A.params[(int64_t)p * MR_PLANT_NPAR + j];
  const bool fixed_dt = A.dt != nullptr;
  const double dt_p = fixed_dt ? A.dt[p] : 0.0;
  const int i = chunk * WL + w.lane;
  const bool active = i < A.n_start;
  const int s = A.start[active ? i : 0];  // idle lanes of a partial chunk follow a valid start and never count
  double x[6], o[6];
  bool alive = active;
  for (int c = 0; c < 6; ++c) {
    x[c] = A.log[(int64_t)c * A.T + s];
    alive = alive && tf_finite(x[c]);
  }
  // step k + 1's controls and truth are loaded while step k computes
  RoStep cur, nxt;
  ro_load(A.log, A.T, s, 1, &cur);
  double* part = A.partials + ((int64_t)pl * A.n_chunk + chunk) * A.H * RO_NPART;
  for (int k = 1; k <= A.H; ++k) {
    if (k < A.H) ro_load(A.log, A.T, s, k + 1, &nxt);
    plant_step<MODEL>(q, x, cur.thr, cur.steer, fixed_dt ? dt_p : cur.ts, o);
    for (int c = 0; c < 6; ++c) alive = alive && tf_finite(o[c]);
    if (A.pred && active)
      for (int c = 0; c < 6; ++c)
        A.pred[(((int64_t)p * A.H + (k - 1)) * 6 + c) * A.n_start + i] = alive ? o[c] : NAN;
    double v[RO_NPART];
    for (int c = 0; c < 6; ++c) {
      double e = cur.truth[c] - o[c];
      if (c == 2) e = atan2(sin(e), cos(e));  // wrapped: the plant's yaw is in (-pi, pi], the log's is continuous
      v[4 * c + 0] = alive ? e : 0.0;
      v[4 * c + 1] = alive ? e * e : 0.0;
      v[4 * c + 2] = alive ? -e : -INFINITY;  // min e = -max(-e)
      v[4 * c + 3] = alive ? e : -INFINITY;
    }
    v[24] = alive ? 1.0 : 0.0;
    const double red = ro_reduce_lds(w, v, lds);
    const int j = w.lane >> 1;
    if (!(w.lane & 1) && j < RO_NPART)
      part[(int64_t)(k - 1) * RO_NPART + j] = (j < 24 && (j & 3) == 2) ? -red : red;
    for (int c = 0; c < 6; ++c) x[c] = alive ? o[c] : x[c];  // a stopped lane keeps its last finite state
    if (k < A.H) cur = nxt;
  }
}

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
