"""Batched closed loop on the GPU: the reference agent's control tick for B vehicles at once.

The reference drives one car in CARLA; each tick (``agent.run_step``, agent.py:207-314) it
senses (projection onto the centerline with the previous progress as bounds, signed error,
agent.py:237-274), and from step ``start_control_at`` = 50 on solves the MPC (``run_mpc``,
agent.py:138-205: N = 15, Ts = 0.05, quartic fit over [progress - 5, progress + 40], max_error =
lookup_error(progress, 45) - car_width / 2, warm start = the previous controls) and applies the
first control; before that it applies (0.5, 0.0).  SURVEY §8(f) rank 1: the same loop with a
``models/`` plant in place of the simulator (the reference's own stand-in, script/verify_*.py).

Here every tick is four device steps on one stream, with no host synchronisation:

1. ``mr_agent_sense``  (csrc/mr_agent.h)  progress, error, cx, cy, max_error for all vehicles;
2. input glue (torch ops on the device): state0 rows, shifted warm start (MPC.py:120-121) -- with
   ``warm_start="primal"`` one ``mr_warm_shift`` launch instead, which also shifts the previous States and
   S_hat into the next solve's primal guess (``mr_solve_batch_warm``);
3. ``mr_solve_batch``  (csrc/mr_wave.h)   the B MPC solves, one wavefront each;
4. ``mr_plant_step``   (csrc/mr_plant.h)  one plant step per vehicle with the applied command
   (``plant="learned"``: ``mr_vehicle_step``, csrc/mr_rollout.h -- the one-step model of the tyre fit,
   learning/vehicle.py:136-205, with ``plant_tyres``: the model-matched plant of an MPC that carries the
   same learned tyres; ``plant_params``: ``mr_plant_step_params``, the same models/ plant with run-time
   constants, one vector or one per vehicle).

Measurement model: the plant state is the simulator truth; the agent's own derivations are kept
-- yaw rate by finite differences of the (wrapped) yaw over the tick (agent.py:240-249), the
commanded throttle fed back as ``cmd_throttle`` / ``cmd_brake`` (agent.py:289-306).  The plant's
body-frame velocities stand for the agent's rotation of the simulator's world velocity
(agent.py:252-253).  No CPU fallback: the constructor raises without a GPU.
"""
import ctypes
import math

import numpy as np
import torch

from .batch import BatchSolver
from .geometry import DeviceTrack, _ptr
from .track import CAR_WIDTH

PLANT = {"kin": 0, "dyn": 1, "blend": 2}
LOG_KEYS = ("X", "Y", "yaw", "vx", "vy", "yawdot", "progress", "error", "cmd_throttle", "cmd_steer", "cmd_brake",
            "status", "iters")


class ClosedLoop:
    def __init__(self, track="shanghai_intl_circuit", B=1, N=15, plant="blend", mpc_model="dyn",
                 precision="fp64", Ts=0.05, dt=0.05, start_control_at=50, lookback=5.0, lookahead=45.0,
                 runtime=(1000.0, 0.85, 50.0, 2.0, 5000.0), device=0, plant_tyres=None, plant_kind=None,
                 plant_params=None, horizon=None, horizon_lookahead=20.0, horizon_min=5, warm_start=None,
                 **solver_kw):
        if start_control_at < 1:
            raise ValueError("start_control_at >= 1: the MPC's yaw rate is a finite difference over one tick")
        self.track = track if isinstance(track, DeviceTrack) else DeviceTrack(track, device=device)
        self.lib = self.track.lib
        self.dev = self.track.device
        self.B, self.N = int(B), int(N)
        self.learned = None
        self.plant_params = None
        if plant_params is not None:
            # one vector [MR_PLANT_NPAR] (rollout.plant_params) or one per vehicle [B][MR_PLANT_NPAR]
            from . import abi
            if plant == "learned":
                raise ValueError('plant_params goes with plant="kin", "dyn" or "blend"')
            q = np.atleast_2d(np.asarray(plant_params, dtype=np.float64))
            if q.ndim != 2 or q.shape[1] != abi.MR_PLANT_NPAR or q.shape[0] not in (1, self.B):
                raise ValueError(f"plant_params: [{abi.MR_PLANT_NPAR}] or [{self.B}][{abi.MR_PLANT_NPAR}], "
                                 f"got {q.shape}")
            self.plant_params = torch.as_tensor(q, dtype=torch.float64, device=self.dev).contiguous()
        if plant == "learned":
            # plant_tyres: a FitResult (its best run) or (params [n_par] or [B][n_par], Fz or None) with plant_kind
            from . import rollout, tyrefit
            if plant_tyres is None:
                raise ValueError('plant="learned" needs plant_tyres (a FitResult or (params, Fz))')
            if isinstance(plant_tyres, tyrefit.FitResult):
                plant_kind = plant_tyres.kind
                plant_tyres = (plant_tyres.params, plant_tyres.Fz[plant_tyres.best_run])
            kind, params, Fz = rollout._tyres(plant_tyres, plant_kind or "pacejka")
            if params.shape[0] not in (1, self.B):
                raise ValueError(f"plant_tyres: one set or one per vehicle ({self.B}), got {params.shape[0]}")
            self.learned = dict(cfg=tyrefit.make_config(kind), P=params.shape[0],
                                params=torch.as_tensor(params, dtype=torch.float64, device=self.dev).contiguous(),
                                Fz=torch.as_tensor(Fz, dtype=torch.float64, device=self.dev).contiguous())
            self.plant = None
        else:
            if plant_tyres is not None:
                raise ValueError('plant_tyres goes with plant="learned"')
            self.plant = PLANT[plant]
        self.dt, self.start_control_at = float(dt), int(start_control_at)
        self.lookback, self.lookahead = float(lookback), float(lookahead)
        # dispatch: longest-expected-first by the previous tick's iteration counts of the same vehicles
        # (mr_config.dispatch_order 2, LPT with a distribution-agnostic estimate); results do not depend on it
        solver_kw.setdefault("dispatch_order", 2)
        self.solver = BatchSolver(N, mpc_model, precision, False, Ts, max_batch=self.B, device=device, **solver_kw)
        f = dict(dtype=torch.float64, device=self.dev)
        # RuntimeControllerParameters (control/ControllerParameters.py:26-32) as (alpha_c, d_max, q_v_y, n,
        # beta_delta), shared (5 values) or per vehicle ([5][B], e.g. a GA population); the reference's
        # NLP reads the class attribute d_max (MPC.py:50), which callers reproduce by passing 0.85
        rt = torch.as_tensor(np.asarray(runtime, dtype=np.float64), **f)
        self.runtime = (rt.reshape(5, 1).expand(5, self.B) if rt.numel() == 5 else rt.reshape(5, self.B)).contiguous()
        # horizon per vehicle (mr_solve_batch_horizons): None -- every vehicle N; "speed" -- each tick, on the
        # device, the reference's rule N_i = ceil(lookahead / (Ts * v_x)) (script/test_mpc.py:32-33,
        # agent.py:152-153), clipped to [horizon_min, N]; an int array [B] -- N_i fixed per vehicle.  N stays
        # the layout of every array; rows beyond N_i are NaN.
        self.Ts = float(Ts)
        self.horizon_mode, self.horizon = None, None
        self.horizon_lookahead, self.horizon_min = float(horizon_lookahead), int(horizon_min)
        if isinstance(horizon, str):
            if horizon != "speed":
                raise ValueError('horizon: None, "speed" or an int array [B]')
            if not 1 <= self.horizon_min <= self.N:
                raise ValueError(f"horizon_min must be in 1..N = {self.N}")
            if not self.horizon_lookahead > 0:
                raise ValueError("horizon_lookahead must be > 0")
            self.horizon_mode = "speed"
        elif horizon is not None:
            hz = np.asarray(horizon.cpu() if isinstance(horizon, torch.Tensor) else horizon)
            if hz.shape != (self.B,) or hz.dtype.kind not in "iu" or hz.min() < 1 or hz.max() > self.N:
                raise ValueError(f"horizon: an int array [{self.B}] with entries in 1..N = {self.N}")
            self.horizon_mode = "fixed"
            self.horizon = torch.as_tensor(hz.astype(np.int32), device=self.dev).contiguous()
        # warm_start: None -- the reference's start (shifted controls rolled out, S ramp, MPC.py:120-131);
        # "primal" -- from the second controlled tick on, the previous solution shifted on the device
        # (mr_warm_shift) as the guess of States and S_hat too (mr_solve_batch_warm)
        if warm_start not in (None, "primal"):
            raise ValueError('warm_start: None or "primal"')
        self.warm_start = warm_start
        if warm_start:
            self._warm = self.solver.alloc_warm(self.B)
            self._warm_used = torch.zeros(self.B, dtype=torch.int32, device=self.dev)
        self._k1 = torch.arange(1, self.N + 1, device=self.dev).reshape(self.N, 1)  # k + 1 of the warm-start gather
        self.sol = self.solver.alloc_outputs(self.B)
        self.progress = torch.empty(self.B, **f)
        self.error = torch.empty(self.B, **f)
        self.cx = torch.empty((5, self.B), **f)
        self.cy = torch.empty((5, self.B), **f)
        self.max_error = torch.empty(self.B, **f)
        self.cmd = torch.empty((2, self.B), **f)
        self.state_next = torch.empty((6, self.B), **f)

    # ------------------------------------------------------------------ state
    def reset(self, state):
        """state [6][B] = (x, y, yaw, v_x, v_y, yaw_dot) of every vehicle (host or device)."""
        f = dict(dtype=torch.float64, device=self.dev)
        self.state = torch.as_tensor(np.asarray(state, dtype=np.float64) if not isinstance(state, torch.Tensor)
                                     else state, **f).reshape(6, self.B).contiguous().clone()
        nan = torch.full((self.B,), math.nan, **f)
        self.prev_progress = nan.clone()   # agent.progress = None: first projection is global
        self.old_yaw = nan.clone()
        self.cmd_throttle = torch.zeros(self.B, **f)  # agent.py:53-55
        self.cmd_steer = torch.zeros(self.B, **f)
        self.cmd_brake = torch.zeros(self.B, **f)
        self.last_controls = None
        self.last_horizon = None  # the horizons of last_controls (horizon modes)
        self.steps = 0

    @staticmethod
    def start_states(track, s0, v0=10.0, offset=0.0):
        """Vehicles on the centerline tangent at progress s0 [B] (lateral offset along the normal)."""
        s0 = np.atleast_1d(np.asarray(s0, dtype=np.float64))
        g, _ = track.eval(s0)
        fr = track.frame(s0)
        g = g.cpu().numpy()
        yaw, nx, ny = (fr[k].cpu().numpy() for k in ("yaw", "nx", "ny"))
        B = len(s0)
        return np.stack([g[0] + offset * nx, g[1] + offset * ny, yaw, np.full(B, float(v0)), np.zeros(B),
                         np.zeros(B)])

    # ------------------------------------------------------------------ one tick
    def tick(self, stream=None):
        """agent.run_step for every vehicle; returns this tick's record (device tensors, no sync).
        Everything -- the library launches and the torch glue between them -- is ordered on ``stream``
        (torch's current stream by default), so the caching allocator and the clones see the kernels'
        order."""
        st = stream if stream is not None else torch.cuda.current_stream(self.dev)
        with torch.cuda.stream(st):
            return self._tick(st)

    def _tick(self, st):
        sp = ctypes_stream(st)
        B, s = self.B, self.state
        X, Y, yaw, vx, vy = s[0], s[1], s[2], s[3], s[4]
        # yaw rate by finite differences of the wrapped yaw (agent.py:240-249)
        d = yaw - self.old_yaw
        d = torch.where(d > 3, yaw - (self.old_yaw + np.pi * 2), torch.where(d < -3, yaw - (self.old_yaw - np.pi * 2), d))
        yawdot = d / self.dt
        # sensing + MPC inputs (agent.py:156-168, 271-274)
        self._check(self.lib.mr_agent_sense(self.track.h, B, _ptr(X.contiguous()), _ptr(Y.contiguous()),
                                            _ptr(self.prev_progress), self.lookback, self.lookahead, CAR_WIDTH / 2,
                                            _ptr(self.progress), _ptr(self.error), _ptr(self.cx), _ptr(self.cy),
                                            _ptr(self.max_error), sp))
        controlled = self.steps >= self.start_control_at
        hz = self.horizon
        if self.horizon_mode == "speed":
            hz = torch.clamp(torch.ceil(self.horizon_lookahead / (self.Ts * torch.clamp(vx, min=1e-3))),
                             self.horizon_min, self.N).to(torch.int32)
        if controlled:
            thr0 = torch.where(self.cmd_brake == 0, self.cmd_throttle, -self.cmd_brake)   # agent.py:149
            state0 = torch.stack([X, Y, yaw, vx, vy, yawdot, thr0, self.cmd_steer]).contiguous()
            u_init = None
            warm = None
            if self.warm_start and self.last_controls is not None:
                # self.sol still holds the previous tick's solution; the solve below overwrites it after the shift
                warm = self.solver.warm_shift(self.sol, state0, self.progress, self.last_horizon, hz,
                                              out=self._warm, stream=st)
                u_init = warm["u_init"]
            elif self.last_controls is not None:  # shifted warm start (MPC.py:120-121)
                lc = self.last_controls
                if hz is None:
                    u_init = torch.cat([lc[:, 1:], lc[:, -1:]], dim=1).contiguous()
                else:  # across a changed horizon: u_init[:, k, i] = U_prev[:, min(k + 1, N_prev_i - 1), i]
                    idx = torch.minimum(self._k1, (self.last_horizon.to(torch.int64) - 1).reshape(1, B))
                    u_init = torch.gather(lc, 1, idx.expand(2, self.N, B)).contiguous()
            dev_in = dict(state0=state0, s0=self.progress, cx=self.cx, cy=self.cy, max_error=self.max_error,
                          runtime=self.runtime, u_init=u_init,
                          # the previous tick's iters, read by the order kernel before this solve writes them
                          order_hint=self.sol["iters"] if self.last_controls is not None else None)
            if hz is not None:
                dev_in["horizon"] = hz
                self.last_horizon = hz
            if warm is not None:
                dev_in.update(x_init=warm["x_init"], s_init=warm["s_init"], warm_use=warm["warm_use"])
                self.sol["warm_used"] = self._warm_used
            elif self.warm_start:
                self._warm_used.zero_()  # the first controlled tick is cold
            self.solver.launch(dev_in, self.sol, stream=st)
            U = self.sol["U"]
            self.last_controls = U.clone()
            throttle, steer = U[0, 0], U[1, 0]
        else:
            throttle = torch.full((B,), 0.5, dtype=torch.float64, device=self.dev)
            steer = torch.zeros(B, dtype=torch.float64, device=self.dev)
        # carla.VehicleControl: negative throttle is brake (agent.py:289-306)
        self.cmd_brake = torch.where(throttle < 0, -throttle, torch.zeros_like(throttle))
        self.cmd_throttle = torch.where(throttle < 0, torch.zeros_like(throttle), throttle)
        self.cmd_steer = steer.clone()
        rec = dict(step=self.steps, X=X.clone(), Y=Y.clone(), yaw=yaw.clone(), vx=vx.clone(), vy=vy.clone(),
                   yawdot=yawdot, progress=self.progress.clone(), error=self.error.clone(),
                   cmd_throttle=self.cmd_throttle, cmd_steer=self.cmd_steer, cmd_brake=self.cmd_brake,
                   controlled=controlled, horizon=hz.clone() if hz is not None else None,
                   status=self.sol["status"].clone() if controlled else None,
                   iters=self.sol["iters"].clone() if controlled else None,
                   warm_used=self._warm_used.clone() if controlled and self.warm_start else None,
                   predicted_states=self.sol["X"].clone() if controlled else None,
                   controls=self.last_controls if controlled else None,
                   s_hat=self.sol["S"].clone() if controlled else None,
                   e_hat_c=self.sol["eC"].clone() if controlled else None,
                   e_hat_l=self.sol["eL"].clone() if controlled else None)
        # plant step with the simulator's command throttle - brake (models/Model.py:83-88)
        self.cmd[0] = self.cmd_throttle - self.cmd_brake
        self.cmd[1] = self.cmd_steer
        if self.plant_params is not None:
            q = self.plant_params
            self._check(self.lib.mr_plant_step_params(self.plant, B, _ptr(self.state), _ptr(self.cmd), self.dt,
                                                      q.shape[0], _ptr(q), _ptr(self.state_next), sp))
        elif self.learned is None:
            self._check(self.lib.mr_plant_step(self.plant, B, _ptr(self.state), _ptr(self.cmd), self.dt,
                                               _ptr(self.state_next), sp))
        else:
            L = self.learned
            self._check(self.lib.mr_vehicle_step(ctypes.byref(L["cfg"]), B, _ptr(self.state), _ptr(self.cmd), self.dt,
                                                 L["P"], _ptr(L["params"]), _ptr(L["Fz"]), _ptr(self.state_next), sp))
        self.state, self.state_next = self.state_next, self.state
        self.old_yaw = yaw.clone()
        self.prev_progress = self.progress.clone()
        self.steps += 1
        return rec

    def run(self, ticks, stream=None):
        """``ticks`` agent steps; returns the list of per-tick records (device tensors)."""
        return [self.tick(stream) for _ in range(int(ticks))]

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(f"libmpcracing error {rc}: {self.lib.mr_last_error().decode()}")


def ctypes_stream(st):
    return ctypes.c_void_p(st.cuda_stream)
