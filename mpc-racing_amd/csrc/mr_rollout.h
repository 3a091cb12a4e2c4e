// Open-loop rollouts of the fitted one-step vehicle model along a logged drive, their error
// statistics, and the model as a closed-loop plant (learning/compare.py:60, script/verify_dynamic.py,
// script/test_model_error.py; learning/vehicle.py:136-205 iterated), fp64, host + gfx950.
//
// The wave body, ro_chunk<Model>, is written once for every rollout (this one and the plant's, mr_plantroll.h):
// start gather, finite test, the prefetch of the next step's controls and truth, the pred store, the 25
// statistics and their reduction, the partials store and the "stopped lane keeps its state" commit.  A model
// object supplies the step from (x, RoStep) to o and whether the yaw error is wrapped: RoTyreModel below,
// RoPlantModel there.  RoArgs holds every rollout's arguments, make_ro_args fills them, rollout_check tests them.
//
// The tyre model is tf_row<false> of mr_tyrefit.h, the tyre constants tf_tyres (with its double-double
// angle), prepared once per wave.  Rollout: one 64-lane wavefront per (parameter set, chunk of 64
// start rows), one lane per start.  The log is structure-of-arrays [9][T]: X, Y, yaw, vx, vy,
// yawdot, throttle (cmd_throttle - cmd_brake), steer, ts, where ts[i] is the duration of the tick
// that ended at row i: the step from row i to row i + 1 uses ts[i + 1]
// (learning/generate_train_val_datasets.py:41-59).  A lane with start s sets x_0 = log[0..5][s] and
// iterates x_k = f(x_{k-1}, throttle[s+k-1], steer[s+k-1], ts[s+k]), k = 1..H; its error at step k
// is e = log[0..5][s+k] - x_k (truth minus prediction, the yaw component the raw difference).
// A lane whose x_0 or x_k is not finite stops: that step and its later ones contribute nothing.
// Per (set, step, component) the sum of e, the sum of e^2, min e and max e over the contributing
// lanes, and per (set, step) their count, are reduced over the wave in a fixed order (ro_reduce_lds
// below: bitwise repeatable, no atomics) into per-chunk partials; ro_finish adds the partials in
// chunk order.  Nothing depends on how many sets share a launch.
#pragma once
#include "mr_tyrefit.h"

// The 25 per-step values are reduced over the wave by one transpose through LDS (ro_reduce_lds): every
// lane stores its 25 values, lanes 2 j and 2 j + 1 reduce the lower and the upper 32 rows of column j
// serially, and one exchange joins the halves.  The additions have a fixed order, which the host build
// emulates.  (A first version used 25 butterflies wsum / wmin / wmax per step: 61 % of the kernel time
// against 24 % now)  MR_ROLLOUT_STATS=0 compiles the reductions out -- the statistics
// are then zeros -- to measure their share (tools/rollout_bench.py).
#ifndef MR_ROLLOUT_STATS
#define MR_ROLLOUT_STATS 1
#endif

namespace mr {

constexpr int RO_NLOG = 9;    // rows of the log
constexpr int RO_NPART = 25;  // per step: 6 x (sum e, sum e^2, min, max), then the count

// The arguments of every rollout.  The tyre rollout passes its mr_tyrefit_config beside them; in the kernels'
// argument blocks every field sits where it sat when the two rollouts had a struct each.
struct RoArgs {
  int T, n_start, H, n_chunk;
  const double* log;      // [9][T]
  const int32_t* start;   // [n_start], every entry in [0, T - 1 - H] (checked before the launch)
  const double* params;   // [P][parameters of the model]
  const double* per_set;  // the model's second array: the tyres' Fz [P][2]; the plant's dt [P] or null (ts of the log)
  double* partials;       // [sets of the launch][n_chunk][H][25], set by the driver of the launch
  double* pred;           // optional [P][H][6][n_start]
};
inline RoArgs make_ro_args(int T, const double* log, int n_start, const int32_t* start, int H, const double* params,
                           const double* per_set, double* pred) {
  return RoArgs{T, n_start, H, (n_start + WL - 1) / WL, log, start, params, per_set, nullptr, pred};
}

// the tests every rollout's sizes pass (a model checks its own arguments before them)
inline const char* rollout_check(int64_t T, int64_t n_start, int64_t H, int64_t P) {
  if (T < 2) return "T < 2";
  if (T > (int64_t)0x7fffffff / RO_NLOG) return "too many log rows";
  if (n_start < 1) return "n_start < 1";
  if (H < 1) return "H < 1";
  if (H > T - 1) return "H exceeds T - 1";
  if (P < 1) return "P < 1";
  if (P * ((n_start + WL - 1) / WL) > (int64_t)0x7fffffff) return "P * ceil(n_start / 64) exceeds the grid limit";
  return nullptr;
}
inline const char* tyre_rollout_check(const mr_tyrefit_config* c, int64_t T, int64_t n_start, int64_t H, int64_t P) {
  if (const char* e = tyrefit_check_config(c)) return e;
  return rollout_check(T, n_start, H, P);
}

constexpr int RO_LDS_WORDS = MR_ROLLOUT_STATS ? WL * RO_NPART : 1;  // doubles of LDS per wave

// Column j of the wave's [64][25] values reduced into lane 2 j (j < 25): v[j] is this lane's row.  Columns
// 4 c + 2, 4 c + 3 (the negated minimum, the maximum) keep the largest entry, the others are summed: rows
// 0..31 in order, rows 32..63 in order, then lower + upper.  Returns the lane's result (lanes >= 50: unused).
MR_WV_FN double ro_reduce_lds(const Wv& w, const double* v, double* lds) {
  for (int j = 0; j < RO_NPART; ++j) lds[w.lane * RO_NPART + j] = v[j];  // odd row stride: no bank conflicts
  wsync_lds(w);
  const int j = mr_min(w.lane >> 1, RO_NPART - 1), r0 = (w.lane & 1) * (WL / 2);
  const bool is_max = j < 24 && (j & 2);
  double acc_s = lds[r0 * RO_NPART + j], acc_m = acc_s;
  for (int r = 1; r < WL / 2; ++r) {
    const double x = lds[(r0 + r) * RO_NPART + j];
    acc_s = acc_s + x;
    acc_m = x > acc_m ? x : acc_m;
  }
  wsync_lds(w);  // the next step's stores come after every lane's loads
  const double mine = is_max ? acc_m : acc_s;
  const double other = wxor(w, mine, 1);
  const double lo = (w.lane & 1) ? other : mine, hi = (w.lane & 1) ? mine : other;
  return is_max ? (hi > lo ? hi : lo) : lo + hi;
}

struct RoStep {
  double thr, steer, ts, truth[6];
};
// controls and truth of step k of a lane that started at row s
MR_HD void ro_load(const double* log, int T, int s, int k, RoStep* r) {
  const int i = s + k;
  r->thr = log[(int64_t)6 * T + i - 1];
  r->steer = log[(int64_t)7 * T + i - 1];
  r->ts = log[(int64_t)8 * T + i];
  for (int c = 0; c < 6; ++c) r->truth[c] = log[(int64_t)c * T + i];
}

// The one-step model of the tyre fit as a rollout model: tf_row<false> with the set's tyre constants, prepared
// once per wave.  A rollout model supplies step(x, controls and truth of the step, o) and wrap_yaw: whether the
// yaw error is the wrapped difference.  (The plant's is RoPlantModel of mr_plantroll.h.)
template <int KIND>
struct RoTyreModel {
  static constexpr bool wrap_yaw = false;  // the log's yaw and the model's are both continuous
  const mr_tyrefit_config& V;
  const TfTyres T;
  MR_HD RoTyreModel(const mr_tyrefit_config& cfg, const RoArgs& A, int p)
      : V(cfg),
        T(tf_tyres(KIND, A.params + (int64_t)p * (KIND == MR_TYRE_PACEJKA ? 18 : 2), A.per_set + 2 * (int64_t)p)) {}
  MR_HD void step(const double* x, const RoStep& s, double* o) const {
    double row[TF_COLS];
    for (int c = 0; c < 6; ++c) row[c] = x[c];
    row[6] = s.thr;
    row[7] = s.steer;
    row[8] = s.ts;
    for (int c = 0; c < 6; ++c) row[9 + c] = s.truth[c];
    tf_row<false>(V, T, row, o, nullptr);
  }
};

// The wave body of every rollout: set p of the call, whose partials are set pl of the buffer (the sets of one
// launch), chunk `chunk` of its starts (lds: RO_LDS_WORDS doubles shared by the wave).
template <class Model>
MR_WV_FN void ro_chunk(const RoArgs& A, const Model& M, int p, int pl, int chunk, double* lds, const Wv& w) {
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
    M.step(x, cur, o);
    for (int c = 0; c < 6; ++c) alive = alive && tf_finite(o[c]);
    if (A.pred && active)
      for (int c = 0; c < 6; ++c)
        A.pred[(((int64_t)p * A.H + (k - 1)) * 6 + c) * A.n_start + i] = alive ? o[c] : NAN;
#if MR_ROLLOUT_STATS
    double v[RO_NPART];
    for (int c = 0; c < 6; ++c) {
      double e = cur.truth[c] - o[c];
      if (Model::wrap_yaw && c == 2) e = atan2(sin(e), cos(e));
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
#else
    if (w.lane == 0)
      for (int j = 0; j < RO_NPART; ++j) part[(int64_t)(k - 1) * RO_NPART + j] = 0.0;
#endif
    for (int c = 0; c < 6; ++c) x[c] = alive ? o[c] : x[c];  // a stopped lane keeps its last finite state
    if (k < A.H) cur = nxt;
  }
}
MR_WV_FN void ro_chunk_kind(const mr_tyrefit_config& cfg, const RoArgs& A, int p, int pl, int chunk, double* lds,
                            const Wv& w) {
  if (cfg.kind == MR_TYRE_PACEJKA) ro_chunk(A, RoTyreModel<MR_TYRE_PACEJKA>(cfg, A, p), p, pl, chunk, lds, w);
  else ro_chunk(A, RoTyreModel<MR_TYRE_LINEAR>(cfg, A, p), p, pl, chunk, lds, w);
}

// partials of set p (local index in the partials buffer: pl) at step k added in chunk order
MR_HD void ro_finish(int H, int n_chunk, const double* partials, int pl, int p, int k, double* stats, int32_t* count) {
  double S[RO_NPART];
  for (int c = 0; c < 6; ++c) {
    S[4 * c] = S[4 * c + 1] = 0.0;
    S[4 * c + 2] = INFINITY;
    S[4 * c + 3] = -INFINITY;
  }
  S[24] = 0.0;
  for (int ch = 0; ch < n_chunk; ++ch) {
    const double* q = partials + (((int64_t)pl * n_chunk + ch) * H + k) * RO_NPART;
    for (int c = 0; c < 6; ++c) {
      S[4 * c] += q[4 * c];
      S[4 * c + 1] += q[4 * c + 1];
      S[4 * c + 2] = q[4 * c + 2] < S[4 * c + 2] ? q[4 * c + 2] : S[4 * c + 2];
      S[4 * c + 3] = q[4 * c + 3] > S[4 * c + 3] ? q[4 * c + 3] : S[4 * c + 3];
    }
    S[24] += q[24];
  }
  const bool none = S[24] == 0.0;
  double* out = stats + ((int64_t)p * H + k) * 24;
  for (int c = 0; c < 6; ++c) {
    out[4 * c] = S[4 * c];
    out[4 * c + 1] = S[4 * c + 1];
    out[4 * c + 2] = none ? NAN : S[4 * c + 2];
    out[4 * c + 3] = none ? NAN : S[4 * c + 3];
  }
  count[(int64_t)p * H + k] = (int32_t)S[24];
}

// One model step of vehicle i: state [6][n], cmd [2][n] -> out [6][n] (may alias state: a lane reads
// its own column before it writes it); tyres shared (P == 1) or one set per vehicle (P == n).
template <int KIND>
MR_HD void ro_vehicle_step(const mr_tyrefit_config& V, int n, int i, const double* state, const double* cmd,
                           double dt, int P, const double* params, const double* Fz, double* out) {
  constexpr int np = KIND == MR_TYRE_PACEJKA ? 18 : 2;
  const int p = P == 1 ? 0 : i;
  const TfTyres T = tf_tyres(KIND, params + (int64_t)p * np, Fz + 2 * (int64_t)p);
  double row[TF_COLS], o[6];
  for (int c = 0; c < 6; ++c) row[c] = state[(int64_t)c * n + i];
  row[6] = cmd[i];
  row[7] = cmd[(int64_t)n + i];
  row[8] = dt;
  for (int c = 0; c < 6; ++c) row[9 + c] = 0.0;
  tf_row<false>(V, T, row, o, nullptr);
  for (int c = 0; c < 6; ++c) out[(int64_t)c * n + i] = o[c];
}

inline const char* vehicle_step_check(const mr_tyrefit_config* c, int64_t n, int64_t P) {
  if (const char* e = tyrefit_check_config(c)) return e;
  if (n < 0) return "n < 0";
  if (n > (int64_t)0x7fffffff / 6) return "too many vehicles";
  if (P != 1 && P != n) return "P must be 1 (shared tyres) or n (one set per vehicle)";
  return nullptr;
}

}  // namespace mr
