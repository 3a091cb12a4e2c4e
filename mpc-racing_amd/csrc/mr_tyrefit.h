// Tyre-model fitting (learning/train.py:78-192 driving learning/vehicle.py:136-205), fp64, host + gfx950.
//
// The reference fits the lateral tyre law of its one-step vehicle model to logged rows
// (X, Y, yaw, vx, vy, yawdot, throttle, steer, dt) -> next (X, Y, yaw, vx, vy, yawdot) by minibatch
// gradient descent in torch.  Here one 64-lane wavefront is one training run: a minibatch of 64 rows
// is one row per lane, the loss and its parameter gradient are reduced with the fixed butterfly wsum
// (mr_wave_prims.h; bitwise repeatable, no atomics), and every lane applies the optimiser update
// redundantly so nothing is broadcast.  The same source runs on the host as an emulated wavefront.
//
// The one-step model is the reference's torch Vehicle.forward, NOT the plant of mr_plant.h: slip
// angles over v_x + 0.1, linear engine efficiency and steer gain, deg2rad = z / 360 * 2 * 3.14
// (control/util.py:10), no yaw wrap, no regen / penalty terms.  Evaluation order follows the Python
// expressions term by term.
//
// Pacejka parameter gradients use the cancellation-free form of pacejka_jet (mr_common.h):
//   Fy = BCD * phi * h(y),  phi = alpha * (1 + E g(B alpha)),  y = B phi,
//   g(x) = atan(x)/x - 1,   h(y) = sin(C atan y) / (C y) = sinc(C atan y) * (1 + g(y)),
// with series for g, g', sinc, sinc' near 0 (the learned coefficients live at |B alpha| ~ 1e-8,
// where autograd through (1 - E) alpha + (E / B) atan(B alpha) returns rounding noise for six of
// the nine coefficients).  Per row the partials with respect to (BCD, B, a0, E) are taken --
// a0 at fixed D and BCD, i.e. along B = BCD / (a0 D), which avoids the cancellation between
// dFy/dC and dFy/dB * dB/dC -- summed over the minibatch, and chained to a[0..8] once per step
// (the chain through pacejka_coef is linear in the sums): 9 reductions per step, not 19.
#pragma once
#include "../../include/mpcracing.h"
#include "mr_common.h"
#include "mr_wave_prims.h"

#if MR_DEVICE_BUILD
#define MR_WV_FN __device__ __forceinline__
#else
#define MR_WV_FN inline
#endif

namespace mr {

constexpr int TF_COLS = 15;     // 9 features + 6 targets per row
constexpr int TF_MAXPAR = 18;   // Pacejka: a[0..8] front, a[0..8] back; linear: stiffness front, back
constexpr int TF_NHYPER = 5;    // lr, beta1, beta2, eps, weight_decay
constexpr int TF_NSUM = 9;      // loss + 4 intermediate sums per tyre

MR_HD int tyrefit_npar(int kind) { return kind == MR_TYRE_PACEJKA ? 18 : 2; }

inline void fill_default_tyrefit_config(mr_tyrefit_config* c) {
  c->kind = MR_TYRE_PACEJKA;
  c->optimizer = MR_OPT_ADAM;
  c->epochs = 25;
  c->patience = 2;
  c->factor = 0.5;
  c->m = 1845.0; c->Iz = 3960.0; c->lf = 0.8; c->lr = 2.0; c->T_max = 743.0; c->r_wheel = 0.37;
  c->C_wheel = 2 * 3.14 * 0.37; c->R = 9.0; c->rho = 1.225; c->C_d = 0.23; c->A_f = 2.2; c->C_roll = 0.012;
  c->g = 9.81; c->max_steer_deg = 70.0;
}

// Argument errors shared by the device entry points and the host twin (NULL when fine).
inline const char* tyrefit_check_config(const mr_tyrefit_config* c) {
  if (!c) return "null config";
  if (c->kind != MR_TYRE_LINEAR && c->kind != MR_TYRE_PACEJKA) return "unknown tyre kind";
  if (c->optimizer != MR_OPT_SGD && c->optimizer != MR_OPT_ADAM && c->optimizer != MR_OPT_ADAMW)
    return "unknown optimiser";
  return nullptr;
}
inline const char* tyrefit_check_fit(const mr_tyrefit_config* c, int64_t n_train, int64_t n_val, int64_t R,
                                     int64_t perm_stride_run) {
  if (const char* e = tyrefit_check_config(c)) return e;
  if (n_train < 1) return "n_train < 1";
  if (n_val < 1) return "n_val < 1";
  if (R < 1) return "R < 1";
  if (c->epochs < 1) return "epochs < 1";
  if (c->patience < 0) return "patience < 0";
  if (n_train > (int64_t)0x7fffffff / TF_COLS || n_val > (int64_t)0x7fffffff / TF_COLS) return "too many rows";
  if (perm_stride_run != 0 && perm_stride_run < (int64_t)c->epochs * n_train)
    return "perm_stride_run must be 0 (shared) or >= epochs * n_train";
  return nullptr;
}

// g(x) = atan(x)/x - 1 and g'(x); series below |x| = 0.1 (next term x^18/19: 2e-17 of the leading one)
MR_HD void tf_g(double x, double* g0, double* g1) {
  const double x2 = x * x;
  if (fabs(x) < 0.1) {
    *g0 = x2 * (-1.0 / 3 + x2 * (1.0 / 5 + x2 * (-1.0 / 7 + x2 * (1.0 / 9 + x2 * (-1.0 / 11 + x2 * (1.0 / 13 +
          x2 * (-1.0 / 15 + x2 * (1.0 / 17))))))));
    *g1 = x * (-2.0 / 3 + x2 * (4.0 / 5 + x2 * (-6.0 / 7 + x2 * (8.0 / 9 + x2 * (-10.0 / 11 + x2 * (12.0 / 13 +
          x2 * (-14.0 / 15 + x2 * (16.0 / 17))))))));
  } else {
    const double at = atan(x), q = 1.0 / (1.0 + x2);
    *g0 = at / x - 1.0;
    *g1 = (q * x - at) / x2;
  }
}

// sinc(u) = sin(u)/u and its derivative (u cos u - sin u)/u^2; series below |u| = 0.1
MR_HD void tf_sinc(double u, double* s0, double* s1) {
  const double u2 = u * u;
  if (fabs(u) < 0.1) {
    *s0 = 1.0 + u2 * (-1.0 / 6 + u2 * (1.0 / 120 + u2 * (-1.0 / 5040 + u2 * (1.0 / 362880 + u2 * (-1.0 / 39916800)))));
    *s1 = u * (-1.0 / 3 + u2 * (1.0 / 30 + u2 * (-1.0 / 840 + u2 * (1.0 / 45360 + u2 * (-1.0 / 3991680 +
          u2 * (1.0 / 518918400))))));
  } else {
    const double s = sin(u), c = cos(u);
    *s0 = s / u;
    *s1 = (u * c - s) / u2;
  }
}

// ---- double-double helpers (value = hi + lo, |lo| <= ulp(hi) / 2) ----------------------------------
struct DD {
  double hi, lo;
};
MR_HD DD dd_two_sum(double a, double b) {
  const double s = a + b, bb = s - a;
  return {s, (a - (s - bb)) + (b - bb)};
}
MR_HD DD dd_two_prod(double a, double b) {
  const double p = a * b;
  return {p, fma(a, b, -p)};
}
MR_HD DD dd_add(DD a, DD b) {
  DD s = dd_two_sum(a.hi, b.hi);
  const DD t = dd_two_sum(a.lo, b.lo);
  s = dd_two_sum(s.hi, s.lo + t.hi);
  return dd_two_sum(s.hi, s.lo + t.lo);
}
MR_HD DD dd_mul(DD a, DD b) {
  const DD p = dd_two_prod(a.hi, b.hi);
  return dd_two_sum(p.hi, p.lo + (a.hi * b.lo + a.lo * b.hi));
}
MR_HD DD dd_mul_d(DD a, double b) {
  const DD p = dd_two_prod(a.hi, b);
  return dd_two_sum(p.hi, p.lo + a.lo * b);
}
// sin and cos of x, |x| <= pi/2, to ~1e-30 absolute: Taylor series of x / 16 in double-double
// (|x / 16| < 0.0982: the x^21 / 21! term is 1e-41), then four angle doublings
MR_HD void dd_sincos(double x, DD* s, DD* c) {
  const DD r{x * 0.0625, 0.0};
  const DD r2 = dd_mul(r, r);
  // term k + 1 = term k * r^2 * -1 / ((2k + 2)(2k + 3)) (sine) or -1 / ((2k + 1)(2k + 2)) (cosine); the
  // reciprocals as double-doubles (hi = the fp64 quotient, lo = its remainder)
  const double inv_s[9] = {1.0 / 6, 1.0 / 20, 1.0 / 42, 1.0 / 72, 1.0 / 110, 1.0 / 156, 1.0 / 210, 1.0 / 272, 1.0 / 342};
  const double inv_s_lo[9] = {9.25185853854297e-18, -2.7755575615628915e-18, 1.32169407693471e-18, 7.709882115452476e-19,
      4.415659757031872e-19, 2.2240044563805217e-19, -4.295505750037808e-19, 5.102127870520021e-20,
      1.6231330769373633e-19};
  const double inv_c[9] = {1.0 / 2, 1.0 / 12, 1.0 / 30, 1.0 / 56, 1.0 / 90, 1.0 / 132, 1.0 / 182, 1.0 / 240, 1.0 / 306};
  const double inv_c_lo[9] = {0.0, 4.625929269271485e-18, 4.625929269271486e-19, 9.912705577010326e-19, -4.2404351634988616e-19,
      -2.1026951223961299e-19, -4.2891514515910067e-19, 5.782411586589357e-20, -9.920804192677818e-20};
  DD ts = r, tc{1.0, 0.0}, ss = r, cs{1.0, 0.0};
  for (int k = 0; k < 9; ++k) {
    ts = dd_mul(dd_mul(ts, r2), DD{-inv_s[k], -inv_s_lo[k]});
    tc = dd_mul(dd_mul(tc, r2), DD{-inv_c[k], -inv_c_lo[k]});
    ss = dd_add(ss, ts);
    cs = dd_add(cs, tc);
  }
  for (int j = 0; j < 4; ++j) {  // sin 2x = 2 s c, cos 2x = 1 - 2 s^2
    const DD sc = dd_mul(ss, cs), s2 = dd_mul(ss, ss);
    ss = DD{2.0 * sc.hi, 2.0 * sc.lo};
    cs = dd_add(DD{1.0, 0.0}, DD{-2.0 * s2.hi, -2.0 * s2.lo});
  }
  *s = ss;
  *c = cs;
}

// psi = atan(a5 Fz) and sin / cos(a4 psi) of pacejka_coef.  Learned coefficients can sit on a zero
// of the cosine (pacejka-1's front tyre: cos = 1.0467e-12, where BCD = a3 sin(.) is stationary in
// a4, a5), and fp64's rounding of the product a4 * psi ~ -4208 (4.5e-13) is then a 25 % error of
// dFy/da4 and dFy/da5.  Near a zero of either function the angle is carried in double-double:
// a5 * Fz exactly, atan corrected by one Newton step on a double-double sin / cos of the fp64 value,
// the product exactly, reduced by a three-part pi / 2 (Cody-Waite: n * part exact for |n| < 2^20).
MR_HD void tf_psi_trig(double a4, double a5, double Fz, double* psi, double* s45, double* c45) {
  const double z = a5 * Fz;
  const double p0 = atan(z);
  *psi = p0;
  *s45 = sin(a4 * p0);
  *c45 = cos(a4 * p0);
  const double lim = 1e-3;
  if ((fabs(*s45) >= lim && fabs(*c45) >= lim) || !(fabs(a4 * p0) < 8e5)) return;
  const DD zz = dd_two_prod(a5, Fz);
  DD s, c;
  dd_sincos(p0, &s, &c);
  // atan(z) - p0 = atan((z c - s) / (c + z s)) with s, c = sin, cos(p0); plus the tail of z
  const DD num = dd_add(dd_mul_d(c, zz.hi), DD{-s.hi, -s.lo});
  const double delta = num.hi / (c.hi + zz.hi * s.hi) + zz.lo / (1.0 + zz.hi * zz.hi);
  const DD ps = dd_two_sum(p0, delta);
  DD th = dd_mul_d(ps, a4);
  const double n = nearbyint(th.hi * 0.63661977236758134308);
  th = dd_add(th, DD{-n * 1.57079632673412561417e+00, 0.0});
  th = dd_add(th, DD{-n * 6.07710050630396597660e-11, 0.0});
  th = dd_add(th, dd_two_prod(-n, 2.02226624871116645580e-21));
  const double sh = sin(th.hi), ch = cos(th.hi);
  const double sr = sh + ch * th.lo, cr = ch - sh * th.lo;
  const int q = (int)((long long)n & 3);
  *s45 = q == 0 ? sr : q == 1 ? cr : q == 2 ? -sr : -cr;
  *c45 = q == 0 ? cr : q == 1 ? -sr : q == 2 ? -cr : sr;
}

// pacejka_coef (mr_batch.h) with the intermediates the chain rule needs
struct TfCoef {
  TyreCoef<double> c;
  double D, psi, s45, c45;  // D, atan(a5 Fz), sin / cos(a4 psi)
};
MR_HD TfCoef tf_coef(const double* a, double Fz) {
  TfCoef t;
  t.c.C = a[0];
  t.D = (a[1] * Fz + a[2]) * Fz;
  tf_psi_trig(a[4], a[5], Fz, &t.psi, &t.s45, &t.c45);
  t.c.BCD = a[3] * t.s45;
  t.c.B = t.c.BCD / (t.c.C * t.D);
  t.c.E = a[6] * Fz * Fz + a[7] * Fz + a[8];
  t.c.K2 = t.c.E * t.c.B * t.c.B;
  return t;
}

// Fy and its partials d[0..3] with respect to (BCD, B, a0, E) at a slip angle:
// B at fixed C; a0 along B = BCD / (a0 D) at fixed D and BCD.
MR_HD double pacejka_partials(const TyreCoef<double>& c, double al, double* d) {
  double g0, g1, t0, t1, S, S1;
  tf_g(c.B * al, &g0, &g1);
  const double phi = al * (1.0 + c.E * g0);
  const double phiE = al * g0;
  const double phiB = c.E * al * al * g1;
  const double y = c.B * phi;
  tf_g(y, &t0, &t1);
  const double t = 1.0 + t0;  // atan(y)/y
  const double qy = 1.0 / (1.0 + y * y);
  const double u = c.C * atan(y);
  tf_sinc(u, &S, &S1);
  const double cu = cos(u);
  const double h = S * t;
  const double H1 = cu * qy;                     // d(y h)/dy
  const double hy = S1 * c.C * qy * t + S * t1;  // dh/dy
  d[0] = phi * h;
  d[1] = c.BCD * (H1 * phiB + phi * phi * hy);
  d[2] = -(c.BCD / c.C) * (phi * y * t1 * cu + H1 * phiB * c.B);
  d[3] = c.BCD * H1 * phiE;
  return c.BCD * phi * h;
}

// gradient with respect to a[0..8] from the sums G[0..3] of (dL/dFy) * pacejka_partials
MR_HD void pacejka_chain(const TfCoef& t, const double* a, double Fz, const double* G, double* ga) {
  const double CD = t.c.C * t.D;
  const double gb = G[0] + G[1] / CD;  // dB/dBCD = 1 / (C D)
  const double bD = -(t.c.B / t.D);    // dB/dD
  const double z = a[5] * Fz;
  ga[0] = G[2];
  ga[1] = G[1] * bD * (Fz * Fz);
  ga[2] = G[1] * bD * Fz;
  ga[3] = gb * t.s45;
  ga[4] = gb * a[3] * t.c45 * t.psi;
  ga[5] = gb * a[3] * t.c45 * a[4] * (Fz / (1.0 + z * z));
  ga[6] = G[3] * (Fz * Fz);
  ga[7] = G[3] * Fz;
  ga[8] = G[3];
}

struct TfTyres {
  int kind;
  double kf, kr;  // linear stiffnesses
  TfCoef f, r;    // Pacejka constants
};
MR_HD TfTyres tf_tyres(int kind, const double* p, const double* Fz) {
  TfTyres T;
  T.kind = kind;
  if (kind == MR_TYRE_PACEJKA) {
    T.f = tf_coef(p, Fz[0]);
    T.r = tf_coef(p + 9, Fz[1]);
    T.kf = T.kr = 0.0;
  } else {
    T.kf = p[0];
    T.kr = p[1];
    T.f = TfCoef{};
    T.r = TfCoef{};
  }
  return T;
}

// One row: prediction o[6], squared-error sum (returned), and with GRAD the per-row terms
// acc[0..3] (front) and acc[4..7] (back) = dL/dFy * dFy/d(intermediate); linear: acc[0], acc[4].
template <bool GRAD>
MR_HD double tf_row(const mr_tyrefit_config& V, const TfTyres& T, const double* x, double* o, double* acc) {
  const double X = x[0], Y = x[1], yaw = x[2], v_x = x[3], v_y = x[4], yaw_dot = x[5];
  const double throttle = x[6], steer = x[7], dt = x[8];
  // Fx
  const double wheel_rpm = (v_x / V.C_wheel) * 60;
  const double rpm = wheel_rpm * V.R * 4.5;
  const double eta = -0.00004428225806 * rpm + 1.282413306;
  const double wheel_force = throttle * eta * V.T_max * V.R / V.r_wheel;
  const double drag_force = 0.5 * V.rho * V.C_d * V.A_f * (v_x * v_x);
  const double rolling_resistance = V.C_roll * V.m * V.g;
  const double Fx = wheel_force - drag_force - rolling_resistance;
  // steer_cmd_to_angle
  const double vel = sqrt(v_x * v_x + v_y * v_y) * 3.6;
  const double gain = -0.001971664699 * vel + 0.986547;
  const double delta = ((steer * gain * V.max_steer_deg) / 360) * 2 * 3.14;
  const double theta_Vf = atan2(v_y + V.lf * yaw_dot, v_x + 0.1);
  const double theta_Vr = atan2(v_y - V.lr * yaw_dot, v_x + 0.1);
  const double af = delta - theta_Vf, ar = -theta_Vr;
  double Fyf, Fyr, df[4] = {af, 0, 0, 0}, dr[4] = {ar, 0, 0, 0};
  if (T.kind == MR_TYRE_PACEJKA) {
    Fyf = pacejka_partials(T.f.c, af, df);
    Fyr = pacejka_partials(T.r.c, ar, dr);
  } else {
    Fyf = T.kf * af;
    Fyr = T.kr * ar;
  }
  const double sd = sin(delta), cd = cos(delta);
  const double v_x_dot = ((Fx - Fyf * sd) / V.m) + (v_y * yaw_dot);
  const double v_y_dot = ((Fyf * cd + Fyr) / V.m) - (v_x * yaw_dot);
  const double yaw_dot_dot = ((Fyf * cd * V.lf) - (Fyr * V.lr)) / V.Iz;
  const double cy = cos(yaw), sy = sin(yaw);
  o[0] = X + (v_x * cy - v_y * sy) * dt;
  o[1] = Y + (v_x * sy + v_y * cy) * dt;
  o[2] = yaw + yaw_dot * dt;
  o[3] = v_x + v_x_dot * dt;
  o[4] = v_y + v_y_dot * dt;
  o[5] = yaw_dot + yaw_dot_dot * dt;
  double e[6], l = 0.0;
  for (int j = 0; j < 6; ++j) {
    e[j] = o[j] - x[9 + j];
    l += e[j] * e[j];
  }
  if (GRAD) {
    const double lf_ = 2.0 * dt * (e[4] * (cd / V.m) - e[3] * (sd / V.m) + e[5] * (cd * V.lf / V.Iz));
    const double lr_ = 2.0 * dt * (e[4] / V.m - e[5] * (V.lr / V.Iz));
    const int np = T.kind == MR_TYRE_PACEJKA ? 4 : 1;
    for (int j = 0; j < np; ++j) {
      acc[j] = lf_ * df[j];
      acc[4 + j] = lr_ * dr[j];
    }
  }
  return l;
}

// Sums over the wave of one minibatch (lane = row; idle lanes of a partial batch contribute 0):
// S[0] = sum of squared errors, S[1..4] front, S[5..8] back (linear: S[1], S[5]).  Not divided.
MR_WV_FN void tf_wave_sums(const Wv& w, const mr_tyrefit_config& V, const TfTyres& T, const double* row, bool active,
                           bool grad, double* S) {
  double o[6], acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  double l = grad ? tf_row<true>(V, T, row, o, acc) : tf_row<false>(V, T, row, o, acc);
  if (!active) {
    l = 0.0;
    for (int j = 0; j < 8; ++j) acc[j] = 0.0;
  }
  S[0] = wsum(w, l);
  for (int j = 1; j < TF_NSUM; ++j) S[j] = 0.0;
  if (!grad) return;
  if (T.kind == MR_TYRE_PACEJKA) {
    for (int j = 0; j < 8; ++j) S[1 + j] = wsum(w, acc[j]);
  } else {
    S[1] = wsum(w, acc[0]);
    S[5] = wsum(w, acc[4]);
  }
}

// mean loss and parameter gradient from the sums over `count` rows (torch's MSELoss: mean over rows x 6)
MR_HD double tf_finish(const TfTyres& T, const double* p, const double* Fz, const double* S, double count,
                       double* g) {
  const double N = count * 6.0;
  if (T.kind == MR_TYRE_PACEJKA) {
    pacejka_chain(T.f, p, Fz[0], S + 1, g);
    pacejka_chain(T.r, p + 9, Fz[1], S + 5, g + 9);
    for (int j = 0; j < 18; ++j) g[j] = g[j] / N;
  } else {
    g[0] = S[1] / N;
    g[1] = S[5] / N;
  }
  return S[0] / N;
}

MR_HD bool tf_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }  // false for NaN and inf

// ---- loss and gradient of P parameter sets over n rows --------------------------------------------
// Wave (p, chunk) reduces rows [64 chunk, 64 chunk + 64) into partials[(p * n_chunk + chunk) * 9 ..].
MR_WV_FN void tf_lossgrad_chunk(const Wv& w, const mr_tyrefit_config& V, int n, const double* rows, int p, int chunk,
                                int n_chunk, const double* params, const double* Fz, double* partials) {
  const int np = tyrefit_npar(V.kind);
  const TfTyres T = tf_tyres(V.kind, params + (int64_t)p * np, Fz + 2 * (int64_t)p);
  const int i = chunk * WL + w.lane;
  const bool active = i < n;
  const int ii = active ? i : 0;
  double row[TF_COLS], S[TF_NSUM];
  for (int c = 0; c < TF_COLS; ++c) row[c] = rows[(int64_t)c * n + ii];
  tf_wave_sums(w, V, T, row, active, true, S);
  if (w.lane == 0)
    for (int j = 0; j < TF_NSUM; ++j) partials[((int64_t)p * n_chunk + chunk) * TF_NSUM + j] = S[j];
}
// partial sums added in chunk order, then the chain rule (one thread per parameter set)
MR_HD void tf_lossgrad_finish(const mr_tyrefit_config& V, int n, int p, int n_chunk, const double* partials,
                              const double* params, const double* Fz, double* loss, double* grad) {
  const int np = tyrefit_npar(V.kind);
  double S[TF_NSUM];
  for (int j = 0; j < TF_NSUM; ++j) S[j] = 0.0;
  for (int k = 0; k < n_chunk; ++k)
    for (int j = 0; j < TF_NSUM; ++j) S[j] += partials[((int64_t)p * n_chunk + k) * TF_NSUM + j];
  const double* pp = params + (int64_t)p * np;
  const TfTyres T = tf_tyres(V.kind, pp, Fz + 2 * (int64_t)p);
  double g[TF_MAXPAR];
  loss[p] = tf_finish(T, pp, Fz + 2 * (int64_t)p, S, (double)n, g);
  for (int j = 0; j < np; ++j) grad[(int64_t)p * np + j] = g[j];
}

// ---- one training run per wavefront ------------------------------------------------------------
struct TfFitArgs {
  mr_tyrefit_config cfg;
  int n_train, n_val, R;
  const double* train;  // [15][n_train]
  const double* val;    // [15][n_val]
  const double* init;   // [R][n_par]
  const double* Fz;     // [R][2]
  const double* hyper;  // [R][5]
  const int32_t* perm;  // [epochs][n_train] (per run when perm_stride_run != 0)
  int64_t perm_stride_run;
  double* p_final;      // [R][n_par]
  double* p_best;       // [R][n_par]
  double* train_loss;   // [R][epochs]
  double* val_loss;     // [R][epochs]
  double* lr_hist;      // [R][epochs]
  int32_t* flag;        // [R]
  double* p_steps;      // optional [R][epochs * ceil(n_train / 64)][n_par]: parameters after every step
};
inline TfFitArgs make_tf_fit_args(const mr_tyrefit_config& cfg, int n_train, const double* train, int n_val,
                                  const double* val, int R, const double* init, const double* Fz,
                                  const double* hyper, const int32_t* perm, int64_t perm_stride_run, double* p_final,
                                  double* p_best, double* train_loss, double* val_loss, double* lr_hist,
                                  int32_t* flag, double* p_steps) {
  return TfFitArgs{cfg,  n_train,         n_val,   R,      train,      val,      init,    Fz,   hyper,
                   perm, perm_stride_run, p_final, p_best, train_loss, val_loss, lr_hist, flag, p_steps};
}

MR_HD void tf_load_row(const double* rows, int n, int i, double* row) {
  for (int c = 0; c < TF_COLS; ++c) row[c] = rows[(int64_t)c * n + i];
}

// KIND is a template parameter so that the parameter loops unroll and p, the moments and the gradient
// live in registers (with a run-time parameter count they are indexed stack arrays: 880 B of scratch per lane).
template <int KIND>
MR_WV_FN void tf_fit_run(const TfFitArgs& A, int run, const Wv& w) {
  const mr_tyrefit_config& V = A.cfg;
  constexpr int np = KIND == MR_TYRE_PACEJKA ? 18 : 2;
  // the loads in registers, read once: a global load inside the step would make its in-order vmcnt
  // wait drain the prefetched gathers of the next minibatch before the evaluation starts
  const double Fz[2] = {A.Fz[2 * (int64_t)run], A.Fz[2 * (int64_t)run + 1]};
  const double* hy = A.hyper + (int64_t)TF_NHYPER * run;
  double lr = hy[0];
  const double beta1 = hy[1], beta2 = hy[2], eps = hy[3], wd = hy[4];
  const int32_t* perm = A.perm + A.perm_stride_run * run;
  double p[np], best[np], m1[np], m2[np];
#pragma unroll
  for (int j = 0; j < np; ++j) {
    p[j] = A.init[(int64_t)run * np + j];
    best[j] = p[j];
    m1[j] = m2[j] = 0.0;
  }
  const int nb = (A.n_train + WL - 1) / WL, nvb = (A.n_val + WL - 1) / WL;
  double best_val = INFINITY;   // best-parameters bookkeeping (strictly lower validation loss)
  double sched_best = INFINITY; // ReduceLROnPlateau state
  int num_bad = 0, step = 0, taken = 0, epoch = 0;
  bool stopped = false;
  for (; epoch < V.epochs; ++epoch) {
    const int32_t* pe = perm + (int64_t)epoch * A.n_train;
    double running = 0.0, cur[TF_COLS], nxt[TF_COLS];
    // Latency hiding: the row index of the lane's row is loaded two minibatches ahead and the row itself
    // one ahead, so no step starts with a dependent load.  The epoch's first rows are made to arrive
    // before the loop (MR_MATERIALIZE reads them), so that the only vector-memory wait inside a step is
    // the one for the prefetched rows where they are moved into `cur`, after the step's reductions.
    int inext = 0;
    {
      const int i = w.lane < A.n_train ? pe[w.lane] : pe[0];
      tf_load_row(A.train, A.n_train, i, cur);
      if (nb > 1) inext = WL + w.lane < A.n_train ? pe[WL + w.lane] : pe[0];
      for (int c = 0; c < TF_COLS; ++c) MR_MATERIALIZE(cur[c]);
      MR_MATERIALIZE(inext);
    }
    for (int b = 0; b < nb; ++b) {
      const int cnt = mr_min(WL, A.n_train - b * WL);
      if (b + 1 < nb) {
        tf_load_row(A.train, A.n_train, inext, nxt);
        const int k = (b + 2) * WL + w.lane;
        if (b + 2 < nb) inext = k < A.n_train ? pe[k] : pe[0];
      }
      const TfTyres T = tf_tyres(KIND, p, Fz);
      double S[TF_NSUM], g[TF_MAXPAR], pn[np];
      tf_wave_sums(w, V, T, cur, w.lane < cnt, true, S);
      const double loss = tf_finish(T, p, Fz, S, (double)cnt, g);
      ++step;
      bool ok = tf_finite(loss);
      // torch.optim update rules (single-tensor forms), identical in every lane
      const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
#pragma unroll
      for (int j = 0; j < np; ++j) {
        double gj = g[j], pj = p[j];
        ok = ok && tf_finite(gj);
        if (V.optimizer == MR_OPT_SGD) {
          if (wd != 0.0) gj = gj + wd * pj;
          pj = pj - lr * gj;
        } else {
          if (V.optimizer == MR_OPT_ADAMW) pj = pj * (1.0 - lr * wd);
          else if (wd != 0.0) gj = gj + wd * pj;
          m1[j] = m1[j] + (gj - m1[j]) * (1.0 - beta1);
          m2[j] = m2[j] * beta2 + (1.0 - beta2) * gj * gj;
          const double step_size = lr / bc1;
          const double denom = sqrt(m2[j]) / sqrt(bc2) + eps;
          pj = pj + (-step_size) * (m1[j] / denom);
        }
        pn[j] = pj;
        ok = ok && tf_finite(pj);
      }
      if (!wuni(w, ok)) {  // the reference hits a breakpoint() here: stop, keep the last finite parameters
        stopped = true;
        break;
      }
#pragma unroll
      for (int j = 0; j < np; ++j) p[j] = pn[j];
      ++taken;
      if (A.p_steps && w.lane == 0)
#pragma unroll
        for (int j = 0; j < np; ++j) A.p_steps[(((int64_t)run * V.epochs + epoch) * nb + b) * np + j] = p[j];
      running += loss;
      if (b + 1 < nb)
        for (int c = 0; c < TF_COLS; ++c) cur[c] = nxt[c];
    }
    if (stopped) break;
    // validation: mean over minibatches of 64 of each batch's MSE (train.py:150-159)
    const TfTyres T = tf_tyres(KIND, p, Fz);
    double vsum = 0.0;
    for (int b = 0; b < nvb; ++b) {
      const int cnt = mr_min(WL, A.n_val - b * WL);
      const int i = b * WL + w.lane;
      double row[TF_COLS], S[TF_NSUM];
      tf_load_row(A.val, A.n_val, i < A.n_val ? i : 0, row);
      tf_wave_sums(w, V, T, row, w.lane < cnt, false, S);
      vsum += S[0] / ((double)cnt * 6.0);
    }
    const double vloss = vsum / (double)nvb;
    if (!wuni(w, tf_finite(vloss))) {
      stopped = true;
      break;
    }
    if (vloss < best_val) {
      best_val = vloss;
#pragma unroll
      for (int j = 0; j < np; ++j) best[j] = p[j];
    }
    // ReduceLROnPlateau(mode min, rel threshold 1e-4, cooldown 0, min_lr 0, eps 1e-8)
    if (vloss < sched_best * (1.0 - 1e-4)) {
      sched_best = vloss;
      num_bad = 0;
    } else {
      ++num_bad;
    }
    if (num_bad > V.patience) {
      const double new_lr = lr * V.factor;
      if (lr - new_lr > 1e-8) lr = new_lr;
      num_bad = 0;
    }
    if (w.lane == 0) {
      A.train_loss[(int64_t)run * V.epochs + epoch] = running / (double)nb;
      A.val_loss[(int64_t)run * V.epochs + epoch] = vloss;
      A.lr_hist[(int64_t)run * V.epochs + epoch] = lr;
    }
  }
  if (w.lane == 0) {
    for (int e = epoch; e < V.epochs; ++e) {  // epochs a stopped run never finished
      A.train_loss[(int64_t)run * V.epochs + e] = NAN;
      A.val_loss[(int64_t)run * V.epochs + e] = NAN;
      A.lr_hist[(int64_t)run * V.epochs + e] = NAN;
    }
    if (A.p_steps)  // steps a stopped run never took
      for (int64_t k = (int64_t)taken * np; k < (int64_t)V.epochs * nb * np; ++k)
        A.p_steps[(int64_t)run * V.epochs * nb * np + k] = NAN;
#pragma unroll
    for (int j = 0; j < np; ++j) {
      A.p_final[(int64_t)run * np + j] = p[j];
      A.p_best[(int64_t)run * np + j] = best[j];
    }
    A.flag[run] = stopped ? 1 : 0;
  }
}

}  // namespace mr
