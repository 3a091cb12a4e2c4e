"""Checker: one tick of the reference's PID agent (agent_pid.Agent.run_step, :157-237) in numpy on
``oracle.splines.Centerline``, and a drive of it against ``oracle.plant``.  TEST INFRASTRUCTURE ONLY.

The expressions are those of agent_pid.py in its order (numpy ufuncs where the reference calls numpy); the
projection is ``oracle.plant.projection`` (the reference's, with the deterministic global search).  The one
addition of the library, the clamp of cmd_steer to [-1, 1], is applied here too; ``steer`` is the unclamped law.
"""
import math

import numpy as np

from oracle import plant

ROWS = ["X", "Y", "yaw", "vx", "vy", "yawdot", "yawdot_fd", "progress", "error", "cmd_throttle", "cmd_steer",
        "cmd_brake", "target_vel", "kappa"]
WHEELBASE = 2.87


def tick(cl, x, mem, g, dt):
    """x [6], mem [4] (NaN = None), g [8] -> (dict of everything run_step computes, new mem [4])."""
    X, Y, yaw, vx, vy = (np.float64(v) for v in x[:5])
    prev, last_error, last_te, old_yaw = (np.float64(v) for v in mem)
    k, zeta, kP_steer, kD_steer, kP_throttle, kD_throttle, lookahead, factor = (np.float64(v) for v in g)
    if math.isnan(old_yaw):
        yawdot = np.nan
    elif yaw - old_yaw > 3:
        yawdot = (yaw - (old_yaw + np.pi * 2)) / dt
    elif yaw - old_yaw < -3:
        yawdot = (yaw - (old_yaw - np.pi * 2)) / dt
    else:
        yawdot = (yaw - old_yaw) / dt
    vel = np.sqrt(vx ** 2 + vy ** 2)
    bounds = plant.progress_bound(None if math.isnan(prev) else float(prev), cl.length)
    progress, dist = plant.projection(cl, float(X), float(Y), bounds)
    error = dist * cl.error_sign(float(X), float(Y), progress)
    # get_alpha / pp_delta
    tx = cl.Gx(progress + lookahead) - cl.Gx(progress)
    ty = cl.Gy(progress + lookahead) - cl.Gy(progress)
    lx = tx * np.cos(-yaw) - ty * np.sin(-yaw)
    ly = tx * np.sin(-yaw) + ty * np.cos(-yaw)
    alpha = np.arctan2(ly, lx)
    delta = np.arctan2(2 * WHEELBASE * np.sin(alpha), lookahead)
    steer = delta + error * kP_steer + (last_error - error) * kD_steer
    vel_lookahead = vel ** 2 / factor
    lower = np.clip(progress + zeta, vel_lookahead, 10000)
    kappa = np.float64(cl.mean_curvature(float(lower), float(vel_lookahead)))
    with np.errstate(divide="ignore"):
        target_vel = np.clip(k * np.sqrt(9.81 / kappa), 10, 100)
    te = target_vel - vel
    throttle = np.clip(te * kP_throttle + (te - last_te) * kD_throttle, -1, 1)
    if throttle < 0:
        brake = np.clip(-throttle, 0.5, 1)
        throttle = 0.0
    else:
        brake = 0.0
    out = dict(progress=progress, error=error, alpha=alpha, delta=delta, steer=steer, kappa=kappa,
               target_vel=target_vel, cmd_throttle=throttle, cmd_brake=brake, cmd_steer=np.clip(steer, -1, 1),
               yawdot_fd=yawdot)
    return {k: float(v) for k, v in out.items()}, np.array([progress, error, te, yaw], np.float64)


def drive(cl, model, x0, mem0, g, T, dt):
    """T ticks of tick + oracle.plant.STEP[model]: (rows name -> [T] (ROWS), final state [6], final mem [4])."""
    x, mem = [float(v) for v in x0], np.array(mem0, np.float64)
    rows = {k: [] for k in ROWS}
    for _ in range(T):
        o, mem = tick(cl, x, mem, g, dt)
        for j, name in enumerate(ROWS[:6]):
            rows[name].append(x[j])
        for name in ROWS[6:]:
            rows[name].append(o[name])
        x = [float(v) for v in plant.STEP[model](x, o["cmd_throttle"] - o["cmd_brake"], o["cmd_steer"], dt)]
    return {k: np.array(v) for k, v in rows.items()}, np.array(x), mem
