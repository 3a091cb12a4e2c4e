// The next tick's primal guess from the previous tick's solution (include/mpcracing.h mr_warm_shift): one
// instance per lane, fp64, shared by the gfx950 kernel and the host build.
#pragma once
#include "mr_batch.h"

namespace mr {

struct WarmShiftArgs {
  int B, NL;
  const double *X_prev, *U_prev, *S_prev;
  const int32_t *status_prev, *horizon_prev;
  const double *state0_new, *s0_new;
  const int32_t* horizon_new;
  double *u_init, *x_init, *s_init;
  int32_t* use;
};

// Instance i: shifted controls in every row of u_init; States / S_hat rows 1..Nn copied from the previous rows
// k + 1 while they exist, then extrapolated with the last control by one model step each and the last Delta-S;
// NaN in row 0 and beyond Nn.
template <int MODEL>
MR_HD void warm_shift_instance(const ProbParams<double>& P, const WarmShiftArgs& A, int i) {
  const int64_t B = A.B;
  const int NL = A.NL;
  const int Np = instance_horizon(A.horizon_prev, i, NL), Nn = instance_horizon(A.horizon_new, i, NL);
  const bool hz_ok = horizon_ok(Np, NL) && horizon_ok(Nn, NL);
  const int Npc = Np < 1 ? 1 : (Np > NL ? NL : Np);  // (the controls' shift of an instance that is not solved anyway)
  auto X = [&](const double* a, int j, int k) -> const double& { return a[((int64_t)j * (NL + 1) + k) * B + i]; };
  bool ok = hz_ok && Np >= 2 && (A.status_prev[i] == MR_STATUS_SOLVED || A.status_prev[i] == MR_STATUS_ACCEPTABLE);
  for (int k = 0; k < NL; ++k) {
    const int kp = k + 1 < Npc - 1 ? k + 1 : Npc - 1;
    for (int r = 0; r < 2; ++r) {
      const double v = A.U_prev[((int64_t)r * NL + kp) * B + i];
      A.u_init[((int64_t)r * NL + k) * B + i] = v;
      if (hz_ok && k < Nn) ok = ok && finite_f64(v);
    }
  }
  for (int j = 0; j < 6; ++j) A.x_init[((int64_t)j * (NL + 1)) * B + i] = NAN;
  A.s_init[i] = NAN;
  const double s0n = A.s0_new[i];
  double x[6], sk = s0n;
  for (int j = 0; j < 6; ++j) x[j] = A.state0_new[(int64_t)j * B + i];
  for (int k = 1; k <= NL; ++k) {
    if (hz_ok && k <= Nn) {
      if (k + 1 <= Np) {
        for (int j = 0; j < 6; ++j) x[j] = X(A.X_prev, j, k + 1);
        sk = s0n + (A.S_prev[(int64_t)(k + 1) * B + i] - A.S_prev[(int64_t)1 * B + i]);
      } else {
        const double u[2] = {A.u_init[((int64_t)0 * NL + (k - 1)) * B + i],
                             A.u_init[((int64_t)1 * NL + (k - 1)) * B + i]};
        double xn[6];
        Dyn<double, MODEL>::f(P, x, u, xn);
        for (int j = 0; j < 6; ++j) x[j] = xn[j];
        sk = sk + (A.S_prev[(int64_t)Np * B + i] - A.S_prev[(int64_t)(Np - 1) * B + i]);
      }
      for (int j = 0; j < 6; ++j) {
        A.x_init[((int64_t)j * (NL + 1) + k) * B + i] = x[j];
        ok = ok && finite_f64(x[j]);
      }
      A.s_init[(int64_t)k * B + i] = sk;
      ok = ok && finite_f64(sk);
    } else {
      for (int j = 0; j < 6; ++j) A.x_init[((int64_t)j * (NL + 1) + k) * B + i] = NAN;
      A.s_init[(int64_t)k * B + i] = NAN;
    }
  }
  A.use[i] = ok ? 1 : 0;
}

MR_HD void warm_shift_dispatch(int model, const ProbParams<double>& P, const WarmShiftArgs& A, int i) {
  switch (model) {
    case MR_MODEL_KINEMATIC: warm_shift_instance<MODEL_KIN>(P, A, i); break;
    case MR_MODEL_DYNAMIC: warm_shift_instance<MODEL_DYN>(P, A, i); break;
    case MR_MODEL_BLENDED: warm_shift_instance<MODEL_BLEND>(P, A, i); break;
    case MR_MODEL_BLENDED_PACEJKA: warm_shift_instance<MODEL_BLEND_PACEJKA>(P, A, i); break;
    default: warm_shift_instance<MODEL_DYN_PACEJKA>(P, A, i); break;
  }
}

}  // namespace mr
