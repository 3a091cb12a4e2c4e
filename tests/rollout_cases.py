"""Shared checks of the open-loop rollouts (csrc/mr_rollout.h, mpcracing/rollout.py) against
tests/golden/rollout_golden.* (generator: make_rollout_golden.py).

Used by test_rollout.py (host build of the source, ``KW = dict(host_twin=True)``) and test_gpu_rollout.py
(gfx950, ``KW = {}``).  Tolerance, per step and component: the error divided by ``scale`` (the largest |value|
of the component in the log) against the 50-digit values is at most 100 x ``ref_noise`` (the reference's torch
model against the same 50-digit values), floor 1e-13.  Every rollout of a (backend, pattern) is computed once
and shared by the checks.
"""
import functools
import json
import os

import numpy as np

from mpcracing import rollout as ro
from mpcracing import tyrefit as tf

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "rollout_golden.npz"))
with open(os.path.join(HERE, "golden", "rollout_golden.json")) as _f:
    META = json.load(_f)
LOG, SCALE, T = G["log"], G["scale"], int(META["T"])
KINDS = META["kinds"]
SETS = [(G[f"set{i}/params"], G[f"set{i}/Fz"]) for i in range(3)]
PATTERNS = sorted(META["patterns"])
EPS = 2.220446049250313e-16


def tol(pattern, i):
    """[H][6] scaled tolerance of set i"""
    return np.maximum(100.0 * G[f"{pattern}/ref_noise"][i], 1e-13)


@functools.lru_cache(maxsize=None)
def _golden_runs(pattern, host_twin):
    H = META["patterns"][pattern]["H"]
    return [ro.rollout_errors(LOG, SETS[i], KINDS[i], H, G[f"{pattern}/starts"], keep_pred=True, host_twin=host_twin)
            for i in range(3)]


def golden_runs(pattern, kw):
    return _golden_runs(pattern, bool(kw.get("host_twin", False)))


def check_golden(pattern, kw):
    """Predictions of all three sets against the 50-digit rollouts; returns the largest scaled error."""
    worst = 0.0
    for i, r in enumerate(golden_runs(pattern, kw)):
        ref = G[f"{pattern}/mp"][i]
        assert r.pred.shape == (1,) + ref.shape
        err = np.abs(r.pred[0] - ref).max(axis=2) / SCALE
        t = tol(pattern, i)
        print(f"{pattern} {META['sets'][i]}: max scaled error per component {np.array2string(err.max(axis=0), precision=1)}"
              f", max error / tolerance {(err / t).max():.2e}")
        assert (err <= t).all(), (pattern, i, err, t)
        worst = max(worst, float(err.max()))
    return worst


def numpy_stats(pred, starts):
    """count, mean, std (ddof 1), rmse, min, max [H][6] of truth minus prediction, pred [H][6][n]"""
    H = pred.shape[0]
    truth = np.stack([LOG[:6, starts + k] for k in range(1, H + 1)])
    e = truth - pred
    n = e.shape[2]
    with np.errstate(invalid="ignore", divide="ignore"):
        std = e.std(axis=2, ddof=1) if n > 1 else np.full(e.shape[:2], np.nan)
    return dict(mean=e.mean(axis=2), std=std, rmse=np.sqrt((e * e).mean(axis=2)), min=e.min(axis=2), max=e.max(axis=2))


def check_statistics(pattern, kw):
    starts = G[f"{pattern}/starts"]
    for i, r in enumerate(golden_runs(pattern, kw)):
        ref = numpy_stats(G[f"{pattern}/mp"][i], starts)
        assert r.count.shape == (1, ref["mean"].shape[0]) and (r.count == len(starts)).all()
        t = tol(pattern, i)
        for k, v in ref.items():
            if k == "std" and len(starts) < 2:
                assert np.isnan(getattr(r, k)).all()
                continue
            err = np.abs(getattr(r, k)[0] - v) / SCALE
            print(f"{pattern} {META['sets'][i]} {k}: max scaled error {err.max():.2e}, / tolerance {(err / t).max():.2e}")
            assert (err <= t).all(), (pattern, i, k, err, t)


def log_rows(log=LOG):
    """The training rows [T - 1][15] of a log (learning/generate_train_val_datasets.py:41-59)."""
    return np.concatenate([log[:8, :-1], log[8:9, 1:], log[:6, 1:]]).T


def check_loss_crosscheck(kw):
    rows = log_rows()
    for i, r in enumerate(golden_runs("h1", kw)):
        mse = r.sumsq[0, 0].sum() / (6.0 * r.count[0, 0])
        loss, _ = tf.loss_grad(rows, SETS[i][0], SETS[i][1], KINDS[i], **kw)
        rel = abs(mse - loss[0]) / loss[0]
        print(f"{META['sets'][i]}: H = 1 mean squared error {mse:.17g}, loss_grad {loss[0]:.17g}, relative {rel:.2e}")
        assert rel <= 1e-13, (i, mse, loss[0])


def _same(a, b):
    """bitwise, NaNs included"""
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
               for x, y in zip(a, b))


def _raw(r, p=slice(None)):
    return (r.sum[p], r.sumsq[p], r.min[p], r.max[p], r.count[p], r.pred[p])


def check_launch_shape(kw):
    """A set alone and among three, and two identical calls, are bitwise equal (70 starts: a full wave and a
    partial one of 6 lanes)."""
    starts, H = G["s3/starts"], 12
    three = np.stack([SETS[1][0], SETS[2][0], SETS[1][0] * 1.01])
    Fz = np.stack([SETS[1][1], SETS[2][1], SETS[1][1]])
    a = ro.rollout_errors(LOG, (three, Fz), "pacejka", H, starts, keep_pred=True, **kw)
    b = ro.rollout_errors(LOG, (three, Fz), "pacejka", H, starts, keep_pred=True, **kw)
    assert _same(_raw(a), _raw(b))
    assert np.isfinite(a.pred).all() and (a.count == len(starts)).all()
    for p in range(3):
        one = ro.rollout_errors(LOG, (three[p], Fz[p]), "pacejka", H, starts, keep_pred=True, **kw)
        assert _same(_raw(one), _raw(a, slice(p, p + 1))), p


def check_start_boundary(kw):
    import pytest
    H = 12
    r = ro.rollout_errors(LOG, SETS[0], "linear", H, [T - 1 - H], **kw)
    assert (r.count == 1).all() and np.isfinite(r.sum).all()
    for bad in ([T - H], [-1], [0, 5, T - H], [3, -1]):
        with pytest.raises(RuntimeError, match=r"error -1: start entry out of range"):
            ro.rollout_errors(LOG, SETS[0], "linear", H, bad, **kw)
    for H_bad in (0, T):
        with pytest.raises(ValueError):
            ro.rollout_errors(LOG, SETS[0], "linear", H_bad, [0], **kw)


def _sum_bound(e):
    """bound on the difference of two fp64 summation orders of the entries e [..., n] (n - 1 roundings each)"""
    return 4.0 * e.shape[-1] * EPS * np.abs(e).sum(axis=-1)


def check_nonfinite_ts(kw):
    """ts[r] = inf: a rollout stops at the step that reaches row r; the others are what a run over them alone gives."""
    r_bad, H = 100, 12
    log = LOG.copy()
    log[8, r_bad] = np.inf
    starts = np.arange(140, dtype=np.int32)  # 64 + 64 + 12 lanes; starts >= r_bad never use ts[r_bad]
    res = ro.rollout_errors(log, SETS[2], "pacejka", H, starts, keep_pred=True, **kw)
    for k in range(1, H + 1):
        alive = ~((starts < r_bad) & (starts + k >= r_bad))
        assert res.count[0, k - 1] == alive.sum(), (k, res.count[0, k - 1], alive.sum())
        assert np.isfinite(res.pred[0, k - 1][:, alive]).all() and np.isnan(res.pred[0, k - 1][:, ~alive]).all()
    for k in (5, H):
        alive = ~((starts < r_bad) & (starts + k >= r_bad))
        sub = ro.rollout_errors(log, SETS[2], "pacejka", k, starts[alive], keep_pred=True, **kw)
        assert sub.count[0, k - 1] == alive.sum()
        assert _same([sub.pred[0, k - 1]], [res.pred[0, k - 1][:, alive]])
        assert _same([sub.min[0, k - 1], sub.max[0, k - 1]], [res.min[0, k - 1], res.max[0, k - 1]])
        e = log[:6, starts[alive] + k] - sub.pred[0, k - 1]
        assert (np.abs(sub.sum[0, k - 1] - res.sum[0, k - 1]) <= _sum_bound(e)).all()
        assert (np.abs(sub.sumsq[0, k - 1] - res.sumsq[0, k - 1]) <= _sum_bound(e * e)).all()


def check_nan_set(kw):
    starts, H = G["c70/starts"], 12
    three = np.stack([SETS[1][0], np.full(18, np.nan), SETS[2][0]])
    Fz = np.stack([SETS[1][1], SETS[1][1], SETS[2][1]])
    r = ro.rollout_errors(LOG, (three, Fz), "pacejka", H, starts, keep_pred=True, **kw)
    assert (r.count[1] == 0).all() and (r.sum[1] == 0).all() and (r.sumsq[1] == 0).all()
    assert np.isnan(r.min[1]).all() and np.isnan(r.max[1]).all() and np.isnan(r.pred[1]).all()
    assert np.isnan(r.mean[1]).all() and np.isnan(r.rmse[1]).all() and np.isnan(r.std[1]).all()
    two = ro.rollout_errors(LOG, (three[[0, 2]], Fz[[0, 2]]), "pacejka", H, starts, keep_pred=True, **kw)
    assert _same(_raw(two), _raw(r, [0, 2]))
    assert (two.count == len(starts)).all()


def check_step_equals_rollout(kw):
    """mr_vehicle_step is bitwise the first step of the rollout, with shared and with per-vehicle tyres."""
    starts = G["h1/starts"]
    state, cmd = LOG[:6, starts], LOG[6:8, starts]
    dt = 0.05
    log = LOG.copy()
    log[8] = dt
    for i in range(3):
        r = ro.rollout_errors(log, SETS[i], KINDS[i], 1, starts, keep_pred=True, **kw)
        out = ro.vehicle_step(state, cmd, dt, SETS[i], KINDS[i], **kw)
        assert _same([out], [r.pred[0, 0]]), i
    # per-vehicle tyres: vehicle j carries set 1 or 2
    pick = np.arange(len(starts)) % 2
    params = np.stack([SETS[1 + p][0] for p in pick])
    Fz = np.stack([SETS[1 + p][1] for p in pick])
    out = ro.vehicle_step(state, cmd, dt, (params, Fz), "pacejka", **kw)
    for p in (0, 1):
        r = ro.rollout_errors(log, SETS[1 + p], "pacejka", 1, starts, keep_pred=True, **kw)
        assert _same([out[:, pick == p]], [r.pred[0, 0][:, pick == p]]), p
    import pytest
    with pytest.raises(RuntimeError, match="P must be 1"):
        ro.vehicle_step(state, cmd, dt, (params[:5], Fz[:5]), "pacejka", **kw)


def check_step_vs_dynamics(kw, eval_dynamics):
    """mr_vehicle_step against the solver's generated dynamics at dt = Ts: eval_dynamics(model, tyres, x [n][6],
    u [n][2], Ts, **config) -> f [n][6] of a MR_MODEL_DYNAMIC / MR_MODEL_DYNAMIC_PACEJKA configuration."""
    Ts = 0.05
    starts = G["h1/starts"]
    state, cmd = LOG[:6, starts], LOG[6:8, starts]
    cases = [("dyn", None, 0, dict(Cf=65000.0, Cr=65000.0))]
    for i in (1, 2):
        p, Fz = SETS[i]
        cases.append(("dyn_pacejka", ((p[:9].copy(), float(Fz[0])), (p[9:].copy(), float(Fz[1]))), i, {}))
    for model, tyres, i, cfg in cases:
        out = ro.vehicle_step(state, cmd, Ts, SETS[i], KINDS[i], **kw)
        f = eval_dynamics(model, tyres, np.ascontiguousarray(state.T), np.ascontiguousarray(cmd.T), Ts, **cfg)
        err = np.abs(out - f.T).max(axis=1) / SCALE
        print(f"{model} {META['sets'][i]}: step vs generated dynamics, scaled error per component "
              f"{np.array2string(err, precision=1)}")
        assert (err <= 1e-12).all(), (model, i, err)


def check_loader(tmp_path):
    from mpcracing.runlog import MEMBER_NAMES
    off = np.pi - LOG[2, T // 2]  # the offset yaw crosses pi in the middle of the log
    yaw = LOG[2] + off
    wrapped = -((-yaw + np.pi) % (2 * np.pi) - np.pi)  # (-pi, pi]
    assert wrapped.max() <= np.pi and wrapped.min() > -np.pi and np.abs(np.diff(wrapped)).max() > 6.0
    brake = np.where(LOG[6] < 0, -LOG[6], 0.0)
    thr = np.where(LOG[6] < 0, 0.0, LOG[6])
    path = os.path.join(str(tmp_path), "steps.csv")
    with open(path, "w") as f:
        f.write(",".join(MEMBER_NAMES) + "\n")
        for j in range(T):
            row = dict(steps=j + 1, X=LOG[0, j], Y=LOG[1, j], yaw=wrapped[j], vx=LOG[3, j], vy=LOG[4, j],
                       yawdot=None if j == 0 else LOG[5, j], progress=0.0, error=0.0, cmd_throttle=thr[j],
                       cmd_steer=LOG[7, j], cmd_brake=brake[j], next_left_lane_point_x=None,
                       next_left_lane_point_y=None, next_right_lane_point_x=None, next_right_lane_point_y=None,
                       last_ts=LOG[8, j], mpc_time=-1)
            f.write(",".join(str(row[k]) for k in MEMBER_NAMES) + "\n")
    got = ro.load_log(path)
    assert got.shape == (9, T) and np.isnan(got[5, 0])
    expect = LOG.copy()
    expect[2] = yaw - yaw[0] + wrapped[0]  # numpy.unwrap keeps the first sample
    expect[5, 0] = np.nan
    rows = [c for c in range(9) if c != 2]
    assert np.array_equal(got[rows][:, 1:], expect[rows][:, 1:]) and np.array_equal(got[rows][:4, 0], expect[rows][:4, 0])
    assert np.abs(got[2] - expect[2]).max() <= 8 * EPS * np.abs(expect[2]).max()  # wrap and unwrap round at |yaw| ~ pi
    raw = ro.load_log(path, unwrap_yaw=False)
    assert np.array_equal(raw[2], wrapped)


def check_rank(kw):
    """rank_by_rollout orders the runs by the golden position RMSE at the last step (H = 12: the first step's
    position does not depend on the tyres); a run without finite values comes last.  (The golden holds two
    Pacejka sets; the third run is the NaN set.)"""
    params = np.stack([SETS[2][0], np.full(18, np.nan), SETS[1][0]])
    Fz = np.stack([SETS[2][1], SETS[1][1], SETS[1][1]])
    z = np.zeros((3, 1))
    res = tf.FitResult("pacejka", Fz, params, params, z, z, z, np.zeros(3, np.int32), [0, 1, 2])
    starts, H = G["s3/starts"], 12
    order = res.rank_by_rollout(LOG, H, starts=starts, **kw)
    e = LOG[:2, starts + H][None] - G["s3/mp"][:, H - 1, :2, :]  # [3 sets][2][n]
    golden = np.sqrt((e * e).sum(axis=1).mean(axis=1))
    expect = [0, 2, 1] if golden[2] < golden[1] else [2, 0, 1]
    got = res.rollout.position_rmse()
    print(f"golden position RMSE at step 12: pacejka_1 {golden[2]:.6e}, pacejka_default {golden[1]:.6e}; got {got}")
    assert list(order) == expect
    # an RMSE moves by at most the largest position error of a prediction: the golden tolerance in X and Y
    bound = [float(np.hypot(*(tol("s3", i)[H - 1, :2] * SCALE[:2]))) for i in range(3)]
    assert abs(got[0] - golden[2]) <= bound[2] and abs(got[2] - golden[1]) <= bound[1]
    assert np.isnan(got[1])
