"""Generate tests/golden/pid_golden.npz / pid_golden.json: the reference's PID agent (agent_pid.py) driving the
reference's own numpy plant (models/DynamicBicycleModel.py, KinematicBicycleModel.py) on t4, tick by tick.

TEST FIXTURE GENERATOR (build container only, CPU only; no test imports it).

It imports the reference's ``agent_pid`` module (never copied) with stand-in modules for ``carla`` (a
``VehicleControl`` that holds throttle, steer, brake) and ``Logger`` (a logger that records nothing), from the
reference directory so that ``ParameterizedCenterline("t4", lanes=False, error=False)`` loads its waypoints.
``agent.progress`` is preset to the start progress: the reference's first projection is an unseeded
``dual_annealing``.  Each drive calls ``Agent.run_step`` with the transform / velocity / boundary objects CARLA
would pass (the plant's state rotated into the global frame, the yaw in degrees) and steps the plant with
``Model.step(control.throttle - control.brake, control.steer, dt = agent.last_ts)``.

Drives: plants ``dyn`` and ``kin`` x start progress 20 and 150, v0 = 14 m/s, lateral offset 0.3 m, 120 ticks of
nominally 0.05 s (the agent's ``last_ts`` is the difference of the simulation times and is what is stored).

Recorded per drive ``<plant>_<s0>/``, every array [120]:
* the inputs of the tick as the agent holds them: ``state`` [120][6] = (agent.X, agent.Y, agent.yaw, agent.vx,
  agent.vy, the plant's yaw_dot), ``mem`` [120][4] = (progress, last_error, last_throttle_error, yaw) BEFORE the
  tick (NaN for None), ``dt`` = agent.last_ts;
* everything run_step computes: ``progress, error, alpha, delta, steer`` (the reference's, not clamped), ``kappa,
  target_vel, throttle, brake, yawdot_fd`` (agent.yawdot, NaN for None).
The spline of the agent's centerline is asserted equal to the t4 table of tests/golden/golden.npz (G1).

Usage: python tests/golden/make_pid_golden.py <path to the reference checkout>
"""
import contextlib
import io
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TICKS, DT, V0, OFFSET = 120, 0.05, 14.0, 0.3
STARTS = [20.0, 150.0]


def standins():
    carla = types.ModuleType("carla")

    class VehicleControl:
        def __init__(self):
            self.throttle, self.steer, self.brake = 0.0, 0.0, 0.0

    carla.VehicleControl = VehicleControl
    logger = types.ModuleType("Logger")

    class Logger:
        def __init__(self, path):
            self.path = path

        def log(self, agent):
            pass

    logger.Logger = Logger
    sys.modules["carla"] = carla
    sys.modules["Logger"] = logger


def nan(v):
    return np.nan if v is None else float(v)


def main(ref):
    ref = os.path.abspath(ref)
    standins()
    os.chdir(ref)
    sys.path.insert(0, ref)
    import agent_pid
    from models.DynamicBicycleModel import DynamicBicycleModel
    from models.KinematicBicycleModel import KinematicBicycleModel
    from models.State import State
    NS = types.SimpleNamespace
    G = np.load(os.path.join(HERE, "golden.npz"))
    out, summary = {}, {}
    for plant, cls in [("dyn", DynamicBicycleModel), ("kin", KinematicBicycleModel)]:
        for s0 in STARTS:
            agent = agent_pid.Agent()
            cl = agent.centerline
            assert np.array_equal(cl.spline_x.t, G["t4/t"]) and np.array_equal(cl.spline_x.c, G["t4/cx"])
            assert np.array_equal(cl.spline_y.c, G["t4/cy"]) and cl.length == float(G["t4/L"])
            nx, ny = cl.unit_principal_normal(s0)
            st0 = State(float(cl.Gx(s0) + OFFSET * nx), float(cl.Gy(s0) + OFFSET * ny),
                        float(cl.unit_tangent_yaw(s0)), V0, 0.0, 0.0)
            model = cls(st0)
            agent.progress = s0
            rec = {k: [] for k in ("state", "mem", "dt", "progress", "error", "alpha", "delta", "steer", "kappa",
                                   "target_vel", "throttle", "brake", "yawdot_fd")}
            for t in range(TICKS):
                s = model.state
                c, sn = np.cos(s.yaw), np.sin(s.yaw)
                vel = NS(x=s.v_x * c - s.v_y * sn, y=s.v_x * sn + s.v_y * c, z=0.0)
                transform = NS(location=NS(x=s.x, y=s.y, z=0.0), rotation=NS(yaw=np.rad2deg(s.yaw)))
                wp = [NS(transform=NS(location=NS(x=0.0, y=0.0)))]
                rec["mem"].append([nan(agent.progress), nan(agent.last_error), nan(agent.last_throttle_error),
                                   nan(agent.yaw)])
                with contextlib.redirect_stdout(io.StringIO()):
                    control = agent.run_step([], [], vel, transform, [wp, wp], (t + 1) * DT)
                rec["state"].append([agent.X, agent.Y, agent.yaw, agent.vx, agent.vy, s.yaw_dot])
                rec["dt"].append(agent.last_ts)
                for k, v in [("progress", agent.progress), ("error", agent.error), ("alpha", agent.alpha),
                             ("delta", agent.delta), ("steer", control.steer), ("kappa", agent.kappa),
                             ("target_vel", agent.target_vel), ("throttle", control.throttle),
                             ("brake", control.brake), ("yawdot_fd", agent.yawdot)]:
                    rec[k].append(nan(v))
                model.step(control.throttle - control.brake, control.steer, dt=agent.last_ts)
            key = f"{plant}_{int(s0)}"
            for k, v in rec.items():
                out[f"{key}/{k}"] = np.array(v, np.float64)
            a = {k: np.array(v, np.float64) for k, v in rec.items()}
            assert np.isfinite(a["state"]).all() and np.isfinite(a["steer"]).all()
            brk = a["brake"] > 0
            assert not np.any((a["throttle"] == 0) & ~brk), "a tick with throttle exactly 0 that is no braking tick"
            summary[key] = dict(max_abs_steer=float(np.abs(a["steer"]).max()), braking_ticks=int(brk.sum()),
                                progress_end=float(a["progress"][-1]), max_abs_error=float(np.abs(a["error"]).max()))
            print(key, summary[key], flush=True)
    np.savez_compressed(os.path.join(HERE, "pid_golden.npz"), **out)
    with open(os.path.join(HERE, "pid_golden.json"), "w") as f:
        json.dump(dict(ticks=TICKS, dt=DT, v0=V0, offset=OFFSET, starts=STARTS, track="t4", drives=summary), f,
                  indent=1)


if __name__ == "__main__":
    main(sys.argv[1])
