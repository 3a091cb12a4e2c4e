// Plant models of the reference's closed loop (models/*.py), fp64, one lane per vehicle.
//
// These are the numpy "simulator-side" models the reference uses to stand in for CARLA
// (script/verify_*.py) -- NOT the MPC's internal dynamics (control/MPC.py:186-260), from which
// they differ: piecewise engine efficiency and steer gain, regenerative brake
// at throttle == 0, the Gaussian "carla_penalty", slip angles over vx (no +0.1), yaw wrapped by
// atan2(sin, cos), the kinematic yaw integrated with the new tan(delta) rate, and the true pi in
// deg2rad.  Evaluation order follows the Python expressions term by term.
#pragma once
#include <type_traits>
#include "mr_common.h"

namespace mr {

enum PlantModel { PLANT_KIN = 0, PLANT_DYN = 1, PLANT_BLEND = 2 };

// models/VehicleParameters.py:3-41 (the plant reads the class defaults)
struct PlantConst {
  static constexpr double m = 1845.0, max_steer = 70.0, T_max = 743.0, r_wheel = 0.37;
  static constexpr double C_wheel = 2 * 3.14 * 0.37, R = 9.0, rho = 1.225, C_d = 0.23, A_f = 2.2;
  static constexpr double C_roll = 0.012, regen_brake_accel = 0.2, Iz = 3960.0, lf = 0.8, lr = 2.0;
  static constexpr double Cf = 65000.0, Cr = 65000.0, g = 9.81, Vblendmin = 2.0, Vblendmax = 15.0;
};

// Model.Fx (models/Model.py:15-64); v_x of the current state
MR_HD double plant_fx(double throttle, double v_x) {
  typedef PlantConst C;
  const double regen_brake_force = throttle == 0.0 ? C::regen_brake_accel * 9.81 * C::m : 0.0;
  const double wheel_rpm = (v_x / C::C_wheel) * 60;
  const double rpm = wheel_rpm * C::R * 4.5;
  const double eta = rpm < 9000 ? 1.0 : (rpm < 9500 ? 0.88 : (rpm < 10400 ? 0.81 : (rpm < 12500 ? 0.71 : 0.675)));
  // scipy.stats.norm.pdf(throttle, loc=0.5, scale=0.0775): exp(-z**2/2) / sqrt(2 pi) / scale
  const double z = (throttle - 0.5) / 0.0775;
  const double carla_penalty = exp(-(z * z) / 2.0) / 2.5066282746310002 / 0.0775 * C::m;
  const double wheel_force = throttle * eta * C::T_max * C::R / C::r_wheel;
  const double drag_force = 0.5 * C::rho * C::C_d * C::A_f * (v_x * v_x);
  const double rolling_resistance = C::C_roll * C::m * C::g;
  return wheel_force - drag_force - rolling_resistance - regen_brake_force - carla_penalty;
}

// Model.steer_cmd_to_angle (models/Model.py:66-81): piecewise gain, numpy deg2rad = x * (pi/180)
MR_HD double plant_steer_angle(double steer_cmd, double v_x, double v_y) {
  const double vel = sqrt(v_x * v_x + v_y * v_y) * 3.6;
  const double gain = vel < 20.0 ? 1.0 : (vel < 60.0 ? 0.9 : (vel < 120.0 ? 0.8 : 0.7));
  return steer_cmd * PlantConst::max_steer * gain * (3.141592653589793 / 180.0);
}

// KinematicBicycleModel.step (models/KinematicBicycleModel.py:11-48); x = (x, y, yaw, vx, vy, r)
MR_HD void plant_kin(const double* x, double thr, double steer, double Ts, double* o) {
  typedef PlantConst C;
  const double delta = plant_steer_angle(steer, x[3], x[4]);
  const double Fx = plant_fx(thr, x[3]);
  const double cy = cos(x[2]), sy = sin(x[2]);
  o[0] = x[0] + (x[3] * cy - x[4] * sy) * Ts;
  o[1] = x[1] + (x[3] * sy + x[4] * cy) * Ts;
  const double yaw_new = x[2] + ((x[3] / (C::lr + C::lf)) * tan(delta)) * Ts;
  o[3] = x[3] + (Fx / C::m) * Ts;
  o[5] = (x[3] / (C::lr + C::lf)) * tan(delta);
  o[4] = x[5] * C::lr;
  o[2] = atan2(sin(yaw_new), cos(yaw_new));
}

// DynamicBicycleModel.step (models/DynamicBicycleModel.py:16-78), linear tyres
MR_HD void plant_dyn(const double* x, double thr, double steer, double Ts, double* o) {
  typedef PlantConst C;
  const double Fx = plant_fx(thr, x[3]);
  const double delta = plant_steer_angle(steer, x[3], x[4]);
  const double theta_Vf = atan2(x[4] + C::lf * x[5], x[3]);
  const double theta_Vr = atan2(x[4] - C::lr * x[5], x[3]);
  const double Fyf = C::Cf * (delta - theta_Vf);
  const double Fyr = C::Cr * (-theta_Vr);
  const double sd = sin(delta), cd = cos(delta);
  const double v_x_dot = ((Fx - Fyf * sd) / C::m) + (x[4] * x[5]);
  const double v_y_dot = ((Fyf * cd + Fyr) / C::m) - (x[3] * x[5]);
  const double yaw_dot_dot = ((Fyf * cd * C::lf) - (Fyr * C::lr)) / C::Iz;
  const double cy = cos(x[2]), sy = sin(x[2]);
  o[0] = x[0] + (x[3] * cy - x[4] * sy) * Ts;
  o[1] = x[1] + (x[3] * sy + x[4] * cy) * Ts;
  const double yaw_new = x[2] + x[5] * Ts;
  o[3] = x[3] + v_x_dot * Ts;
  o[4] = x[4] + v_y_dot * Ts;
  o[5] = x[5] + yaw_dot_dot * Ts;
  o[2] = atan2(sin(yaw_new), cos(yaw_new));
}

// BlendedBicycleModel.step (models/BlendedBicycleModel.py:18-58): both models from the same
// state, lambda = clip((hypot(vx, vy) - 2) / (15 - 2), 0, 1), elementwise blend (wrapped yaws)
MR_HD void plant_step(int model, const double* x, double thr, double steer, double Ts, double* o) {
  if (model == PLANT_KIN) { plant_kin(x, thr, steer, Ts, o); return; }
  if (model == PLANT_DYN) { plant_dyn(x, thr, steer, Ts, o); return; }
  double k[6], d[6];
  plant_kin(x, thr, steer, Ts, k);
  plant_dyn(x, thr, steer, Ts, d);
  const double vel = hypot(x[3], x[4]);
  double lam = (vel - PlantConst::Vblendmin) / (PlantConst::Vblendmax - PlantConst::Vblendmin);
  lam = lam < 0.0 ? 0.0 : (lam > 1.0 ? 1.0 : lam);
  for (int j = 0; j < 6; ++j) o[j] = lam * d[j] + (1 - lam) * k[j];
}

// ---- the same plant with run-time parameters -------------------------------------------------------
// One vector of MR_PLANT_NPAR doubles per parameter set: the fields of PlantConst in declaration order,
// then the three constants of the penalty term of plant_fx (amplitude factor, location, width).  The
// functions below evaluate the expressions of their constexpr twins in the same order, so with
// mr_plant_params_default's vector a step is bitwise the step above (the amplitude 1.0 multiplies
// exactly).  Literals that are no VehicleParameters field (9.81 of the regenerative brake, 4.5, 3.6, the
// rpm and speed steps, the true pi of deg2rad) stay literals.
#define MR_PP_M 0
#define MR_PP_MAX_STEER 1
#define MR_PP_T_MAX 2
#define MR_PP_R_WHEEL 3
#define MR_PP_C_WHEEL 4
#define MR_PP_R 5
#define MR_PP_RHO 6
#define MR_PP_C_D 7
#define MR_PP_A_F 8
#define MR_PP_C_ROLL 9
#define MR_PP_REGEN 10
#define MR_PP_IZ 11
#define MR_PP_LF 12
#define MR_PP_LR 13
#define MR_PP_CF 14
#define MR_PP_CR 15
#define MR_PP_G 16
#define MR_PP_VBLENDMIN 17
#define MR_PP_VBLENDMAX 18
#define MR_PP_PEN_AMP 19
#define MR_PP_PEN_LOC 20
#define MR_PP_PEN_WIDTH 21
#ifndef MR_PLANT_NPAR
#define MR_PLANT_NPAR 22
#endif
static_assert(MR_PLANT_NPAR == MR_PP_PEN_WIDTH + 1, "MR_PLANT_NPAR of mpcracing.h and the index macros disagree");

MR_HD void plant_params_default(double* q) {
  typedef PlantConst C;
  q[MR_PP_M] = C::m; q[MR_PP_MAX_STEER] = C::max_steer; q[MR_PP_T_MAX] = C::T_max; q[MR_PP_R_WHEEL] = C::r_wheel;
  q[MR_PP_C_WHEEL] = C::C_wheel; q[MR_PP_R] = C::R; q[MR_PP_RHO] = C::rho; q[MR_PP_C_D] = C::C_d;
  q[MR_PP_A_F] = C::A_f; q[MR_PP_C_ROLL] = C::C_roll; q[MR_PP_REGEN] = C::regen_brake_accel; q[MR_PP_IZ] = C::Iz;
  q[MR_PP_LF] = C::lf; q[MR_PP_LR] = C::lr; q[MR_PP_CF] = C::Cf; q[MR_PP_CR] = C::Cr; q[MR_PP_G] = C::g;
  q[MR_PP_VBLENDMIN] = C::Vblendmin; q[MR_PP_VBLENDMAX] = C::Vblendmax;
  q[MR_PP_PEN_AMP] = 1.0; q[MR_PP_PEN_LOC] = 0.5; q[MR_PP_PEN_WIDTH] = 0.0775;
}

MR_HD double plant_fx(const double* q, double throttle, double v_x) {
  const double regen_brake_force = throttle == 0.0 ? q[MR_PP_REGEN] * 9.81 * q[MR_PP_M] : 0.0;
  const double wheel_rpm = (v_x / q[MR_PP_C_WHEEL]) * 60;
  const double rpm = wheel_rpm * q[MR_PP_R] * 4.5;
  const double eta = rpm < 9000 ? 1.0 : (rpm < 9500 ? 0.88 : (rpm < 10400 ? 0.81 : (rpm < 12500 ? 0.71 : 0.675)));
  const double z = (throttle - q[MR_PP_PEN_LOC]) / q[MR_PP_PEN_WIDTH];
  const double carla_penalty =
      q[MR_PP_PEN_AMP] * (exp(-(z * z) / 2.0) / 2.5066282746310002 / q[MR_PP_PEN_WIDTH]) * q[MR_PP_M];
  const double wheel_force = throttle * eta * q[MR_PP_T_MAX] * q[MR_PP_R] / q[MR_PP_R_WHEEL];
  const double drag_force = 0.5 * q[MR_PP_RHO] * q[MR_PP_C_D] * q[MR_PP_A_F] * (v_x * v_x);
  const double rolling_resistance = q[MR_PP_C_ROLL] * q[MR_PP_M] * q[MR_PP_G];
  return wheel_force - drag_force - rolling_resistance - regen_brake_force - carla_penalty;
}

MR_HD double plant_steer_angle(const double* q, double steer_cmd, double v_x, double v_y) {
  const double vel = sqrt(v_x * v_x + v_y * v_y) * 3.6;
  const double gain = vel < 20.0 ? 1.0 : (vel < 60.0 ? 0.9 : (vel < 120.0 ? 0.8 : 0.7));
  return steer_cmd * q[MR_PP_MAX_STEER] * gain * (3.141592653589793 / 180.0);
}

MR_HD void plant_kin(const double* q, const double* x, double thr, double steer, double Ts, double* o) {
  const double delta = plant_steer_angle(q, steer, x[3], x[4]);
  const double Fx = plant_fx(q, thr, x[3]);
  const double cy = cos(x[2]), sy = sin(x[2]);
  o[0] = x[0] + (x[3] * cy - x[4] * sy) * Ts;
  o[1] = x[1] + (x[3] * sy + x[4] * cy) * Ts;
  const double yaw_new = x[2] + ((x[3] / (q[MR_PP_LR] + q[MR_PP_LF])) * tan(delta)) * Ts;
  o[3] = x[3] + (Fx / q[MR_PP_M]) * Ts;
  o[5] = (x[3] / (q[MR_PP_LR] + q[MR_PP_LF])) * tan(delta);
  o[4] = x[5] * q[MR_PP_LR];
  o[2] = atan2(sin(yaw_new), cos(yaw_new));
}

MR_HD void plant_dyn(const double* q, const double* x, double thr, double steer, double Ts, double* o) {
  const double Fx = plant_fx(q, thr, x[3]);
  const double delta = plant_steer_angle(q, steer, x[3], x[4]);
  const double theta_Vf = atan2(x[4] + q[MR_PP_LF] * x[5], x[3]);
  const double theta_Vr = atan2(x[4] - q[MR_PP_LR] * x[5], x[3]);
  const double Fyf = q[MR_PP_CF] * (delta - theta_Vf);
  const double Fyr = q[MR_PP_CR] * (-theta_Vr);
  const double sd = sin(delta), cd = cos(delta);
  const double v_x_dot = ((Fx - Fyf * sd) / q[MR_PP_M]) + (x[4] * x[5]);
  const double v_y_dot = ((Fyf * cd + Fyr) / q[MR_PP_M]) - (x[3] * x[5]);
  const double yaw_dot_dot = ((Fyf * cd * q[MR_PP_LF]) - (Fyr * q[MR_PP_LR])) / q[MR_PP_IZ];
  const double cy = cos(x[2]), sy = sin(x[2]);
  o[0] = x[0] + (x[3] * cy - x[4] * sy) * Ts;
  o[1] = x[1] + (x[3] * sy + x[4] * cy) * Ts;
  const double yaw_new = x[2] + x[5] * Ts;
  o[3] = x[3] + v_x_dot * Ts;
  o[4] = x[4] + v_y_dot * Ts;
  o[5] = x[5] + yaw_dot_dot * Ts;
  o[2] = atan2(sin(yaw_new), cos(yaw_new));
}

// MODEL as a template argument: the rollout kernel is one instantiation per model
template <int MODEL>
MR_HD void plant_step(const double* q, const double* x, double thr, double steer, double Ts, double* o) {
  if (MODEL == PLANT_KIN) { plant_kin(q, x, thr, steer, Ts, o); return; }
  if (MODEL == PLANT_DYN) { plant_dyn(q, x, thr, steer, Ts, o); return; }
  double k[6], d[6];
  plant_kin(q, x, thr, steer, Ts, k);
  plant_dyn(q, x, thr, steer, Ts, d);
  const double vel = hypot(x[3], x[4]);
  double lam = (vel - q[MR_PP_VBLENDMIN]) / (q[MR_PP_VBLENDMAX] - q[MR_PP_VBLENDMIN]);
  lam = lam < 0.0 ? 0.0 : (lam > 1.0 ? 1.0 : lam);
  for (int j = 0; j < 6; ++j) o[j] = lam * d[j] + (1 - lam) * k[j];
}
MR_HD void plant_step(int model, const double* q, const double* x, double thr, double steer, double Ts, double* o) {
  if (model == PLANT_KIN) plant_step<PLANT_KIN>(q, x, thr, steer, Ts, o);
  else if (model == PLANT_DYN) plant_step<PLANT_DYN>(q, x, thr, steer, Ts, o);
  else plant_step<PLANT_BLEND>(q, x, thr, steer, Ts, o);
}

// Host side: f(std::integral_constant<int, PLANT_*>()) for a checked run-time model -- the one place where a
// launch or a host loop picks the instantiation of a kernel or wave body templated on the model (rollout,
// drive, segment timing; mpcracing.hip and the host build).
template <class F>
inline void plant_dispatch(int model, F&& f) {
  if (model == PLANT_KIN) f(std::integral_constant<int, PLANT_KIN>());
  else if (model == PLANT_DYN) f(std::integral_constant<int, PLANT_DYN>());
  else f(std::integral_constant<int, PLANT_BLEND>());
}

}  // namespace mr
