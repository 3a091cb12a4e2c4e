"""Which tyre fit is good: open-loop rollouts along a logged drive, and the fitted model as a plant.

The reference judges a model by rolling it forward along a logged drive and comparing it with what the car
did (learning/compare.py:60 -- per-component statistics of truth minus prediction --, script/verify_dynamic.py,
script/test_model_error.py).  ``rollout_errors`` does that for P parameter sets x every start row x H steps
in one call of ``mr_tyre_rollout`` (csrc/mr_rollout.h: one 64-lane wavefront per parameter set and chunk of
64 starts, fixed butterfly reductions, bitwise repeatable); ``vehicle_step`` is one step of the same model
for a batch of vehicles (``mr_vehicle_step``), the plant of ``ClosedLoop(plant="learned")``.

``plant_rollout_errors`` / ``plant_step`` / ``plant_params`` are the same for the ``models/`` plant of the closed
loop with its constants as data (``mr_plant_rollout``, ``mr_plant_step_params``, csrc/mr_plantroll.h;
script/verify_kinematic.py, verify_dynamic.py, verify_blend.py); ``mpcracing.plantfit`` searches them.

``host_twin=True`` runs the g++ build of the same source instead (TEST-ONLY, explicit; there is no
fallback: without it a missing GPU or library is an error).
"""
import ctypes

import numpy as np

from . import abi
from .runlog import MEMBER_NAMES
from .tyrefit import FZ_DEFAULT, N_PAR, FitResult, _Device, _Host, make_config

LOG_ROWS = ["X", "Y", "yaw", "vx", "vy", "yawdot", "throttle", "steer", "ts"]
COMPONENTS = LOG_ROWS[:6]


def load_log(steps_csv, unwrap_yaw=True):
    """The [9][T] log (LOG_ROWS) of a run's ``steps.csv`` in the reference's Logger format
    (``runlog.MEMBER_NAMES``): throttle = cmd_throttle - cmd_brake, ts = last_ts, ``None`` -> NaN.  With
    ``unwrap_yaw`` the yaw is made continuous (``numpy.unwrap``), so that a raw yaw difference is an error."""
    with open(steps_csv) as f:
        names = f.readline().strip().split(",")
        missing = [c for c in MEMBER_NAMES if c not in names]
        if missing:
            raise ValueError(f"{steps_csv}: missing columns {missing}")
        col = {c: names.index(c) for c in names}
        rows = [[np.nan if v.strip() in ("None", "") else float(v) for v in line.strip().split(",")]
                for line in f if line.strip()]
    a = np.array(rows, np.float64).reshape(len(rows), len(names))
    g = lambda c: a[:, col[c]]  # noqa: E731
    log = np.stack([g("X"), g("Y"), g("yaw"), g("vx"), g("vy"), g("yawdot"), g("cmd_throttle") - g("cmd_brake"),
                    g("cmd_steer"), g("last_ts")])
    if unwrap_yaw:
        log[2] = unwrap(log[2])
    return log


def unwrap(yaw):
    """``numpy.unwrap`` over the finite entries (a NaN row does not break the chain)."""
    yaw = np.array(yaw, np.float64)
    ok = np.isfinite(yaw)
    yaw[ok] = np.unwrap(yaw[ok])
    return yaw


def _tyres(tyres, kind):
    """(kind, params [P][n_par], Fz [P][2]) of a FitResult (every run's best parameters) or (params, Fz)."""
    if isinstance(tyres, FitResult):
        if kind is not None and kind != tyres.kind:
            raise ValueError(f"kind {kind!r} but the FitResult holds {tyres.kind!r} tyres")
        return tyres.kind, np.array(tyres.p_best, np.float64), np.array(tyres.Fz, np.float64)
    if kind not in N_PAR:
        raise ValueError(f"unknown tyre kind {kind!r} (linear, pacejka)")
    params, Fz = tyres
    params = np.atleast_2d(np.asarray(params, np.float64))
    if params.shape[1] != N_PAR[kind]:
        raise ValueError(f"params: expected [P][{N_PAR[kind]}] for {kind}, got {params.shape}")
    Fz = np.array(np.broadcast_to(np.asarray(FZ_DEFAULT if Fz is None else Fz, np.float64), (params.shape[0], 2)))
    return kind, np.ascontiguousarray(params), Fz


class RolloutErrors:
    """Statistics of truth minus prediction per parameter set, step and component ([P][H][6], COMPONENTS):
    ``count`` [P][H] rollouts that reached the step, ``mean``, ``std`` (ddof 1, as pandas ``describe()``),
    ``rmse``, ``min``, ``max``; ``sum``, ``sumsq`` as reduced; ``pred`` [P][H][6][n_start] when kept."""

    def __init__(self, stats, count, pred, starts, horizon):
        self.starts, self.horizon = starts, horizon
        self.count, self.pred = count, pred
        self.sum, self.sumsq = stats[..., 0], stats[..., 1]
        self.min, self.max = stats[..., 2], stats[..., 3]
        n = count[..., None].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            self.mean = np.where(n > 0, self.sum / n, np.nan)
            self.rmse = np.where(n > 0, np.sqrt(self.sumsq / n), np.nan)
            var = (self.sumsq - n * self.mean * self.mean) / (n - 1)
            self.std = np.where(n > 1, np.sqrt(np.maximum(var, 0.0)), np.nan)

    def position_rmse(self, step=None):
        """[P]: root mean square of the position error (X, Y) at ``step`` (1-based; default: the last)."""
        k = (self.horizon if step is None else int(step)) - 1
        n = self.count[:, k].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(n > 0, np.sqrt((self.sumsq[:, k, 0] + self.sumsq[:, k, 1]) / n), np.nan)

    def position_cost(self):
        """[P]: the sum over the steps of sumsq_X + sumsq_Y, added in step order.  For one start this is the
        square of script/optimize_coeffs.py:34-38's ``_cost`` (numpy.linalg.norm of the position differences)."""
        cost = np.zeros(self.sumsq.shape[0])
        for k in range(self.horizon):
            cost = cost + (self.sumsq[:, k, 0] + self.sumsq[:, k, 1])
        return cost


def _log(log):
    log = np.ascontiguousarray(log, np.float64)
    if log.ndim != 2 or log.shape[0] != 9:
        raise ValueError(f"log: expected [9][T], got {log.shape}")
    return log


def _rollout(name, lead, log, params, per_set, horizon, starts, keep_pred, device, host_twin):
    """What both rollouts share: the horizon and the starts, the buffers, the ``mr_<name>`` call and its result.
    lead: the entry's first argument (tyre config / plant model); per_set: the array that follows the parameters
    (Fz [P][2] / dt [P] or None)."""
    T, H, P = log.shape[1], int(horizon), params.shape[0]
    if H < 1 or H > T - 1:
        raise ValueError(f"horizon {H} outside [1, T - 1 = {T - 1}]")
    starts = np.arange(T - H, dtype=np.int32) if starts is None else np.ascontiguousarray(starts, np.int32).ravel()
    n = len(starts)
    be = _Host() if host_twin else _Device(device)
    d = [be.put(log), be.put(starts), be.put(params)] + ([be.put(per_set)] if per_set is not None else [])
    stats, count = be.empty((P, H, 6, 4)), be.empty((P, H), np.int32)
    pred = be.empty((P, H, 6, n)) if keep_pred else None
    be.call(name, lead, T, be.ptr(d[0]), n, be.ptr(d[1]), H, P, be.ptr(d[2]),
            be.ptr(d[3]) if per_set is not None else None, be.ptr(stats), be.ptr(count),
            be.ptr(pred) if keep_pred else None)
    return RolloutErrors(be.get(stats), be.get(count), be.get(pred) if keep_pred else None, starts, H)


def _step(name, lead, state, cmd, dt, params, per_set, device, host_twin):
    """One ``mr_<name>`` step of n vehicles (``vehicle_step``, ``plant_step``); lead and per_set as in ``_rollout``."""
    state = np.ascontiguousarray(state, np.float64).reshape(6, -1)
    n = state.shape[1]
    cmd = np.ascontiguousarray(cmd, np.float64).reshape(2, n)
    be = _Host() if host_twin else _Device(device)
    d = [be.put(state), be.put(cmd), be.put(params)] + ([be.put(per_set)] if per_set is not None else [])
    out = be.empty((6, n))
    be.call(name, lead, n, be.ptr(d[0]), be.ptr(d[1]), float(dt), params.shape[0], *[be.ptr(a) for a in d[2:]],
            be.ptr(out))
    return be.get(out)


def rollout_errors(log, tyres, kind=None, horizon=10, starts=None, keep_pred=False, device=0, host_twin=False,
                   **vehicle):
    """Roll the one-step model with ``tyres`` forward ``horizon`` steps from every start row of ``log`` [9][T]
    (``load_log``) and reduce truth minus prediction.  tyres: a ``FitResult`` (all its runs) or (params
    [P][n_par], Fz [P][2] or None) with ``kind``; starts: row indices in [0, T - 1 - horizon] (default: all of
    them).  Returns a RolloutErrors."""
    log = _log(log)
    kind, params, Fz = _tyres(tyres, kind)
    cfg = make_config(kind, host_twin=host_twin, **vehicle)
    return _rollout("tyre_rollout", ctypes.byref(cfg), log, params, Fz, horizon, starts, keep_pred, device, host_twin)


def vehicle_step(state, cmd, dt, tyres, kind=None, device=0, host_twin=False, **vehicle):
    """One model step of n vehicles: state [6][n], cmd [2][n] = (throttle - brake, steer) -> [6][n] (numpy).
    tyres as in ``rollout_errors``: one set shared by all vehicles, or one per vehicle."""
    kind, params, Fz = _tyres(tyres, kind)
    cfg = make_config(kind, host_twin=host_twin, **vehicle)
    return _step("vehicle_step", ctypes.byref(cfg), state, cmd, dt, params, Fz, device, host_twin)


# ---- the models/ plant with run-time parameters (csrc/mr_plant.h, mr_plantroll.h) ----
PLANT_FIELDS = ["m", "max_steer", "T_max", "r_wheel", "C_wheel", "R", "rho", "C_d", "A_f", "C_roll",
                "regen_brake_accel", "Iz", "lf", "lr", "Cf", "Cr", "g", "Vblendmin", "Vblendmax",
                "penalty_amp", "penalty_loc", "penalty_width"]
# models/VehicleParameters.py:8-38 and models/Model.py:50; the libraries' mr_plant_params_default gives the same
# vector (tests/plantroll_cases.py)
PLANT_DEFAULTS = [1845.0, 70.0, 743.0, 0.37, 2 * 3.14 * 0.37, 9.0, 1.225, 0.23, 2.2, 0.012, 0.2, 3960.0, 0.8, 2.0,
                  65000.0, 65000.0, 9.81, 2.0, 15.0, 1.0, 0.5, 0.0775]
assert len(PLANT_FIELDS) == len(PLANT_DEFAULTS) == abi.MR_PLANT_NPAR


def plant_params(**overrides):
    """[MR_PLANT_NPAR]: the plant's default parameters (the class defaults of models/VehicleParameters.py and
    the penalty term of Model.Fx, as ``mr_plant_params_default``) with ``overrides`` by field name
    (``PLANT_FIELDS``); an unknown name raises."""
    unknown = [k for k in overrides if k not in PLANT_FIELDS]
    if unknown:
        raise ValueError(f"unknown plant parameter(s) {unknown}; the fields are {PLANT_FIELDS}")
    q = np.array(PLANT_DEFAULTS, np.float64)
    for k, v in overrides.items():
        q[PLANT_FIELDS.index(k)] = float(v)
    return q


def _plant_args(model, params):
    if model not in abi.MR_PLANT:
        raise ValueError(f"unknown plant model {model!r} (kin, dyn, blend)")
    params = plant_params() if params is None else np.asarray(params, np.float64)
    params = np.ascontiguousarray(np.atleast_2d(params))
    if params.ndim != 2 or params.shape[1] != abi.MR_PLANT_NPAR or params.shape[0] < 1:
        raise ValueError(f"params: expected [P][{abi.MR_PLANT_NPAR}] with P >= 1, got {params.shape}")
    return abi.MR_PLANT[model], params


def plant_rollout_errors(log, model, params=None, dt=None, horizon=10, starts=None, keep_pred=False, device=0,
                         host_twin=False):
    """Roll the ``model`` plant ("kin", "dyn", "blend") with ``params`` [P][MR_PLANT_NPAR] (``plant_params``;
    default: one default set) forward ``horizon`` steps from every start row of ``log`` [9][T] and reduce truth
    minus prediction (the yaw error wrapped to (-pi, pi]).  The step length is the log's ``ts`` or, with ``dt``
    (a number or [P]), one fixed step per set.  One ``mr_plant_rollout`` call; returns a RolloutErrors."""
    log = _log(log)
    model, params = _plant_args(model, params)
    if dt is not None:
        dt = np.ascontiguousarray(np.broadcast_to(np.asarray(dt, np.float64), (params.shape[0],)))
    return _rollout("plant_rollout", model, log, params, dt, horizon, starts, keep_pred, device, host_twin)


def plant_step(state, cmd, dt, model, params=None, device=0, host_twin=False):
    """One plant step of n vehicles: state [6][n], cmd [2][n] = (throttle - brake, steer) -> [6][n] (numpy).
    params: one vector shared by all vehicles (default: the defaults) or one per vehicle ([n][MR_PLANT_NPAR])."""
    model, params = _plant_args(model, params)
    return _step("plant_step_params", model, state, cmd, dt, params, None, device, host_twin)
