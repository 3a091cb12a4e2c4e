"""Shared checks of the plant rollouts (csrc/mr_plant.h run-time parameters, csrc/mr_plantroll.h,
mpcracing/rollout.py, mpcracing/plantfit.py) against tests/golden/plant_rollout_golden.* (generator:
make_plant_rollout_golden.py) and the log of rollout_golden.npz.

Used by test_plant_rollout.py (host build of the source, ``KW = dict(host_twin=True)``) and
test_gpu_plant_rollout.py (gfx950, ``KW = {}``).  Tolerance of the golden checks, per step and component: the
error divided by ``scale`` (the largest |value| of the component in the log) against the 50-digit values is at
most 100 x ``ref_noise`` (the reference's numpy models against the same 50-digit values), floor 1e-13 -- the
rule of rollout_cases.tol.  The rollouts of a (backend, pattern, model) are computed once, all three sets in
one call, and shared by the checks.
"""
import functools
import json
import os

import numpy as np
import pytest

from mpcracing import plantfit
from mpcracing import rollout as ro
from oracle import plant as oracle_plant

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "plant_rollout_golden.npz"))
with open(os.path.join(HERE, "golden", "plant_rollout_golden.json")) as _f:
    META = json.load(_f)
_R = np.load(os.path.join(HERE, "golden", "rollout_golden.npz"))
LOG, SCALE = _R["log"], _R["scale"]
G7 = np.load(os.path.join(HERE, "golden", "golden.npz"))
T = LOG.shape[1]
MODELS = META["models"]
PARAMS = G["params"]
PATTERNS = sorted(META["patterns"])
EPS = 2.220446049250313e-16
assert T == META["T"] and MODELS == ["kin", "dyn", "blend"]


def tol(pattern, i, m):
    """[H][6] scaled tolerance of set i, model m"""
    return np.maximum(100.0 * G[f"{pattern}/ref_noise"][i, m], 1e-13)


def wrap(d):
    return np.arctan2(np.sin(d), np.cos(d))


def _same(a, b):
    """bitwise, NaNs included"""
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
               for x, y in zip(a, b))


def _raw(r, p=slice(None)):
    return (r.sum[p], r.sumsq[p], r.min[p], r.max[p], r.count[p], r.pred[p])


@functools.lru_cache(maxsize=None)
def _golden_run(pattern, model, host_twin):
    H = META["patterns"][pattern]["H"]
    return ro.plant_rollout_errors(LOG, model, PARAMS, horizon=H, starts=G[f"{pattern}/starts"], keep_pred=True,
                                   host_twin=host_twin)


def golden_run(pattern, model, kw):
    return _golden_run(pattern, model, bool(kw.get("host_twin", False)))


def check_defaults(kw):
    """plant_params: the libraries' default vector, overrides by name, unknown names."""
    be = ro._Host() if kw.get("host_twin") else None
    q = np.full(ro.abi.MR_PLANT_NPAR, np.nan)
    import ctypes
    ptr = q.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    if be is not None:
        assert be.lib.mrh_plant_params_default(ptr) == 0
    else:
        assert ro.abi.load_product().mr_plant_params_default(ptr) == 0
    assert _same([q], [ro.plant_params()]) and _same([q], [PARAMS[0]])
    p = ro.plant_params(Cf=80000.0, Cr=50000.0, m=1700.0)
    assert _same([p], [PARAMS[1]])
    assert _same([ro.plant_params(penalty_amp=0.0, Vblendmax=25.0)], [PARAMS[2]])
    assert ro.PLANT_FIELDS == META["fields"]
    with pytest.raises(ValueError, match="unknown plant parameter"):
        ro.plant_params(mass=1.0)


def check_golden(pattern, kw):
    """Predictions of the three sets and three models against the 50-digit rollouts; returns the largest scaled
    error per model."""
    worst = {}
    for m, model in enumerate(MODELS):
        r = golden_run(pattern, model, kw)
        ref = G[f"{pattern}/mp"][:, m]
        assert r.pred.shape == ref.shape
        for i in range(3):
            err = np.abs(r.pred[i] - ref[i]).max(axis=2) / SCALE
            t = tol(pattern, i, m)
            print(f"{pattern} {model} {META['sets'][i]}: max scaled error per component "
                  f"{np.array2string(err.max(axis=0), precision=1)}, max error / tolerance {(err / t).max():.2e}")
            assert (err <= t).all(), (pattern, model, i, err, t)
            worst[model] = max(worst.get(model, 0.0), float(err.max()))
    return worst


def numpy_stats(pred, starts, log=LOG):
    """mean, std (ddof 1), rmse, min, max [H][6] of truth minus prediction (yaw wrapped), pred [H][6][n]"""
    H = pred.shape[0]
    truth = np.stack([log[:6, starts + k] for k in range(1, H + 1)])
    e = truth - pred
    e[:, 2] = wrap(e[:, 2])
    return dict(mean=e.mean(axis=2), std=e.std(axis=2, ddof=1), rmse=np.sqrt((e * e).mean(axis=2)),
                min=e.min(axis=2), max=e.max(axis=2))


def check_statistics(pattern, kw):
    starts = G[f"{pattern}/starts"]
    for m, model in enumerate(MODELS):
        r = golden_run(pattern, model, kw)
        assert (r.count == len(starts)).all()
        for i in range(3):
            ref = numpy_stats(G[f"{pattern}/mp"][i, m], starts)
            t = tol(pattern, i, m)
            for k, v in ref.items():
                err = np.abs(getattr(r, k)[i] - v) / SCALE
                print(f"{pattern} {model} {META['sets'][i]} {k}: max scaled error {err.max():.2e}, "
                      f"/ tolerance {(err / t).max():.2e}")
                assert (err <= t).all(), (pattern, model, i, k, err, t)


def check_g7(kw):
    """The G7 fixture (the reference's own 100-step plant rollouts at a fixed dt) as a one-start log through the
    dt override, default parameters: the bar tests/test_plant.py holds the host plant to."""
    cmd, dt = G7["g7_cmd"], float(G7["g7_dt"])
    n = len(cmd)  # 101 rows: 100 steps
    for model in MODELS:
        traj = G7[f"g7_{model}"]
        assert traj.shape == (n, 6)
        log = np.empty((9, n))
        log[:6] = traj.T            # truth: the reference's trajectory; row 0 is g7_init
        log[:6, 0] = G7["g7_init"]
        log[6], log[7] = cmd[:, 0], cmd[:, 1]
        log[8] = 1.0                # not the step length: the override is
        r = ro.plant_rollout_errors(log, model, dt=[dt], horizon=n - 1, starts=[0], keep_pred=True, **kw)
        assert (r.count == 1).all()
        np.testing.assert_allclose(r.pred[0, :, :, 0], traj[1:], rtol=1e-11, atol=1e-9)


def states(n, seed):
    """tests/test_plant.py::_states: throttle 0 and 0.5, every rpm and gain step, the blend corners"""
    rng = np.random.default_rng(seed)
    st = np.stack([rng.uniform(-500, 500, n), rng.uniform(-500, 500, n), rng.uniform(-3.1, 3.1, n),
                   rng.uniform(-1, 60, n), rng.uniform(-3, 3, n), rng.uniform(-1.5, 1.5, n)])
    cmd = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)])
    cmd[0, :8] = 0.0   # regenerative brake branch (throttle == 0)
    cmd[0, 8:12] = 0.5  # peak of the carla penalty
    st[3, 12:20] = np.array([9000, 9500, 10400, 12500, 8999, 9499, 10399, 12499]) * 0.37 * 2 * 3.14 / (60 * 9.0 * 4.5)
    st[3, 20:26] = [0.0, 2.0, 15.0, 20 / 3.6, 60 / 3.6, 120 / 3.6]  # blend corners, gain steps
    st[4, 20:26] = 0.0
    return st, cmd


def check_default_step_bitwise(kw, legacy_step):
    """plant_step with the default vector against the step with compile-time constants:
    legacy_step(model index, state, cmd, dt) -> [6][n] of the same backend."""
    st, cmd = states(256, 3)
    for m, model in enumerate(MODELS):
        old = legacy_step(m, st, cmd, 0.05)
        for params in (None, ro.plant_params(), PARAMS[0]):
            new = ro.plant_step(st, cmd, 0.05, model, params, **kw)
            assert _same([new], [old]), model
        assert np.isfinite(old[:, 21:]).all()
        other = ro.plant_step(st, cmd, 0.05, model, PARAMS[1], **kw)
        assert not _same([other], [old])  # the parameters are read


def check_step_equals_rollout(kw):
    """plant_step is bitwise the first step of the rollout (fixed dt), shared and per-vehicle parameters; P == n
    equals n single calls."""
    starts = G["c70/starts"]
    state, cmd = LOG[:6, starts], LOG[6:8, starts]
    dt = 0.05
    for model in MODELS:
        r = ro.plant_rollout_errors(LOG, model, PARAMS, dt=dt, horizon=1, starts=starts, keep_pred=True, **kw)
        for i in range(3):
            out = ro.plant_step(state, cmd, dt, model, PARAMS[i], **kw)
            assert _same([out], [r.pred[i, 0]]), (model, i)
        n = 7
        pick = np.arange(n) % 3
        out = ro.plant_step(state[:, :n], cmd[:, :n], dt, model, PARAMS[pick], **kw)
        for j in range(n):
            one = ro.plant_step(state[:, j], cmd[:, j], dt, model, PARAMS[pick[j]], **kw)
            assert _same([one[:, 0]], [out[:, j]]), (model, j)
            assert _same([out[:, j]], [r.pred[pick[j], 0][:, j]])
    with pytest.raises(RuntimeError, match="P must be 1"):
        ro.plant_step(state, cmd, dt, "dyn", PARAMS[:2], **kw)


def check_launch_shape(kw):
    """A set alone and among three, and two identical calls, are bitwise equal (70 starts: a full wave and a
    partial one of 6 lanes)."""
    starts, H = G["s3/starts"], 12
    for model in MODELS:
        a = golden_run("s3", model, kw)
        b = ro.plant_rollout_errors(LOG, model, PARAMS, horizon=H, starts=starts, keep_pred=True, **kw)
        assert _same(_raw(a), _raw(b))
        assert np.isfinite(a.pred).all() and (a.count == len(starts)).all()
        for p in range(3):
            one = ro.plant_rollout_errors(LOG, model, PARAMS[p], horizon=H, starts=starts, keep_pred=True, **kw)
            assert _same(_raw(one), _raw(a, slice(p, p + 1))), (model, p)


def _oracle_rollout(model, log, starts, H, dt=None):
    """oracle.plant.STEP iterated: [H][6][n]"""
    out = np.empty((H, 6, len(starts)))
    for j, s in enumerate(starts):
        x = [float(v) for v in log[:6, s]]
        for k in range(1, H + 1):
            x = oracle_plant.STEP[model](x, float(log[6, s + k - 1]), float(log[7, s + k - 1]),
                                         float(log[8, s + k]) if dt is None else dt)
            out[k - 1, :, j] = x
    return out


def check_branches(kw):
    """Throttle exactly 0.0 (regenerative brake) on 10 rows and exactly 0.5 (the penalty's peak) on 10 rows, which
    the log lacks: default parameters, H = 3, every start, against the oracle."""
    log = LOG.copy()
    zero, half = np.arange(20, 320, 30), np.arange(35, 335, 30)
    assert len(zero) == len(half) == 10 and half.max() < T
    log[6, zero], log[6, half] = 0.0, 0.5
    starts = np.arange(T - 3, dtype=np.int32)
    for model in MODELS:
        r = ro.plant_rollout_errors(log, model, horizon=3, starts=starts, keep_pred=True, **kw)
        ref = _oracle_rollout(model, log, starts, 3)
        assert (r.count == len(starts)).all()
        np.testing.assert_allclose(r.pred[0], ref, rtol=1e-11, atol=1e-9)
        # the branch is taken: the same rows without it differ
        r0 = ro.plant_rollout_errors(LOG, model, horizon=3, starts=starts, keep_pred=True, **kw)
        assert not np.array_equal(r.pred[0, 0, 3, zero], r0.pred[0, 0, 3, zero])


def check_yaw_wrap(kw):
    """1.5 rad added to every yaw of the log: truth crosses pi (and stays continuous), the plant's yaw wraps.
    Predictions against the oracle; every yaw error is the wrapped difference."""
    log = LOG.copy()
    log[2] += 1.5
    assert log[2].min() < np.pi < log[2].max()
    starts, H = np.concatenate([G["c70/starts"], G["s3/starts"][24:]]).astype(np.int32), 12
    for model in MODELS:
        r = ro.plant_rollout_errors(log, model, horizon=H, starts=starts, keep_pred=True, **kw)
        ref = _oracle_rollout(model, log, starts, H)
        # a yaw within an ulp of +-pi may wrap to either side: compare the angle on the circle
        d = r.pred[0] - ref
        d[:, 2] = wrap(d[:, 2])
        bar = 1e-9 + 1e-11 * np.abs(ref)
        assert (np.abs(d) <= bar).all(), (model, np.abs(d).max(axis=(0, 2)))
        assert np.abs(r.pred[0][:, 2]).max() <= np.pi
        truth = np.stack([log[2, starts + k] for k in range(1, H + 1)])
        raw = truth - r.pred[0][:, 2]
        assert np.abs(raw).max() > np.pi  # the raw difference would be off by 2 pi
        e = wrap(raw)
        # one lane's value: the same subtraction, then sin, cos and atan2 of two libraries (a few ulp of pi)
        bar = 16 * EPS * np.pi
        assert np.abs(r.min[0, :, 2]).max() <= np.pi and np.abs(r.max[0, :, 2]).max() <= np.pi
        assert np.abs(r.min[0, :, 2] - e.min(axis=1)).max() <= bar
        assert np.abs(r.max[0, :, 2] - e.max(axis=1)).max() <= bar
        n = len(starts)
        assert np.abs(r.sum[0, :, 2] - e.sum(axis=1)).max() <= n * bar + 4 * n * EPS * np.abs(e).sum(axis=1).max()
        assert np.abs(r.sumsq[0, :, 2] - (e * e).sum(axis=1)).max() <= \
            2 * np.pi * n * bar + 4 * n * EPS * (e * e).sum(axis=1).max()


def _raw_rollout_rc(kw, model, H, P, starts, dt=None):
    """The library's return code of a rollout call with these arguments (no Python-side checks)."""
    be = ro._Host() if kw.get("host_twin") else ro._Device(0)
    starts = np.asarray(starts, np.int32)
    d = [be.put(LOG), be.put(starts), be.put(np.tile(PARAMS[0], (max(P, 1), 1)))]
    if dt is not None:
        d.append(be.put(np.asarray(dt, np.float64)))
    stats, count = be.empty((max(P, 1), H if H > 0 else 1, 6, 4)), be.empty((max(P, 1), H if H > 0 else 1), np.int32)
    args = [model, T, be.ptr(d[0]), len(starts), be.ptr(d[1]), H, P, be.ptr(d[2]),
            be.ptr(d[3]) if dt is not None else None, be.ptr(stats), be.ptr(count), None]
    return be.lib.mrh_plant_rollout(*args, 1) if kw.get("host_twin") else be.lib.mr_plant_rollout(*args, be.stream())


def check_edges(kw):
    H = 12
    # starts at 0 and at T - 1 - H
    r = ro.plant_rollout_errors(LOG, "blend", horizon=H, starts=[0, T - 1 - H], **kw)
    assert (r.count == 2).all() and np.isfinite(r.sum).all()
    for bad in ([T - H], [-1], [0, 5, T - H]):
        with pytest.raises(RuntimeError, match=r"start entry out of range"):
            ro.plant_rollout_errors(LOG, "blend", horizon=H, starts=bad, **kw)
        assert _raw_rollout_rc(kw, 2, H, 1, bad) == -1
    for H_bad in (0, T):
        with pytest.raises(ValueError):
            ro.plant_rollout_errors(LOG, "kin", horizon=H_bad, starts=[0], **kw)
        assert _raw_rollout_rc(kw, 0, H_bad, 1, [0]) == -1
    assert _raw_rollout_rc(kw, 1, H, 0, [0]) == -1          # P = 0
    with pytest.raises(ValueError):
        ro.plant_rollout_errors(LOG, "dyn", PARAMS[:0], horizon=H, **kw)
    for bad_model in (-1, 3):
        assert _raw_rollout_rc(kw, bad_model, H, 1, [0]) == -1
    with pytest.raises(ValueError, match="unknown plant model"):
        ro.plant_rollout_errors(LOG, "learned", horizon=H, **kw)
    with pytest.raises(ValueError, match="expected"):
        ro.plant_rollout_errors(LOG, "dyn", PARAMS[:, :21], horizon=H, **kw)
    assert _raw_rollout_rc(kw, 1, H, 1, [0]) == 0
    assert _raw_rollout_rc(kw, 1, H, 2, [0], dt=[0.05, 0.01]) == 0
    for bad_dt in ([0.05, 0.0], [-0.05, 0.05], [0.05, np.nan], [np.inf, 0.05]):
        assert _raw_rollout_rc(kw, 1, H, 2, [0], dt=bad_dt) == -1
        with pytest.raises(RuntimeError, match="dt entry"):
            ro.plant_rollout_errors(LOG, "dyn", PARAMS[:2], dt=bad_dt, horizon=H, starts=[0], **kw)


def check_nan_row(kw):
    """A NaN in one start row stops that lane only (starts 3 j, H = 2: row 15 is nobody's truth or control but
    start 15's)."""
    starts, H = G["s3/starts"], 2
    log = LOG.copy()
    log[3, 15] = np.nan
    lane = int(np.where(starts == 15)[0][0])
    others = np.arange(len(starts)) != lane
    for model in MODELS:
        r = ro.plant_rollout_errors(log, model, PARAMS, horizon=H, starts=starts, keep_pred=True, **kw)
        clean = ro.plant_rollout_errors(LOG, model, PARAMS, horizon=H, starts=starts[others], keep_pred=True, **kw)
        assert (r.count == len(starts) - 1).all()
        assert np.isnan(r.pred[:, :, :, lane]).all()
        assert _same([r.pred[:, :, :, others]], [clean.pred])
        assert _same([r.min, r.max], [clean.min, clean.max])
        assert np.isfinite(r.sum).all() and np.isfinite(r.sumsq).all()


def check_nan_set(kw):
    starts, H = G["c70/starts"], 12
    three = np.stack([PARAMS[1], np.full(ro.abi.MR_PLANT_NPAR, np.nan), PARAMS[2]])
    for model in MODELS:
        r = ro.plant_rollout_errors(LOG, model, three, horizon=H, starts=starts, keep_pred=True, **kw)
        assert (r.count[1] == 0).all() and (r.sum[1] == 0).all() and (r.sumsq[1] == 0).all()
        assert np.isnan(r.min[1]).all() and np.isnan(r.max[1]).all() and np.isnan(r.pred[1]).all()
        assert np.isnan(r.mean[1]).all() and np.isnan(r.rmse[1]).all() and np.isnan(r.std[1]).all()
        g = golden_run("c70", model, kw)
        assert _same(_raw(g, [1, 2]), _raw(r, [0, 2])), model


def synthetic_log(kw, n=120, row0=100, **truth):
    """A log whose states are plant_step("dyn", truth) iterated from LOG row ``row0`` with the log's controls and
    ts: the rollout of the same backend reproduces it exactly."""
    q = ro.plant_params(**truth)
    syn = LOG[:, row0:row0 + n].copy()
    for i in range(n - 1):
        syn[:6, i + 1] = ro.plant_step(syn[:6, i], syn[6:8, i], syn[8, i + 1], "dyn", q, **kw)[:, 0]
    assert np.isfinite(syn).all()
    return syn


def check_identify(kw):
    syn = synthetic_log(kw, Cf=80000.0, Cr=50000.0)
    H = 10
    # the truth is a node of round 1: 50000 + 4 * 7500, 20000 + 4 * 7500
    res = plantfit.identify(syn, "dyn", {"Cf": (50000.0, 110000.0), "Cr": (20000.0, 80000.0)}, H, grid=9, rounds=3,
                            **kw)
    assert res.values == {"Cf": 80000.0, "Cr": 50000.0} and res.cost == 0.0
    assert _same([res.params], [ro.plant_params(Cf=80000.0, Cr=50000.0)]) and res.dt is None
    assert [h["best_cost"] for h in res.history] == [0.0, 0.0, 0.0] and res.history[0]["n_sets"] == 81
    # off the grid
    free = {"Cf": (41000.0, 97000.0), "Cr": (33000.0, 91000.0)}  # 80000 and 50000 are no nodes of linspace(.., 7)
    a = plantfit.identify(syn, "dyn", free, H, grid=7, rounds=4, **kw)
    b = plantfit.identify(syn, "dyn", free, H, grid=7, rounds=4, **kw)
    best = [h["best_cost"] for h in a.history]
    print(f"off-grid identification: {a.values}, cost {a.cost:.3e}, best cost per round {best}")
    assert all(y <= x for x, y in zip(best, best[1:]))
    assert a.cost == min(h["round_min"] for h in a.history) == best[-1]
    assert a.values == b.values and a.cost == b.cost and _same([a.params], [b.params])
    assert all(_same([x["lo"], x["hi"]], [y["lo"], y["hi"]]) and x["best_cost"] == y["best_cost"]
               and x["round_min"] == y["round_min"] and x["best_values"] == y["best_values"]
               for x, y in zip(a.history, b.history))
    for k, (lo, hi) in free.items():
        assert lo <= a.values[k] <= hi
    # dt as a free field, through both spellings
    c = plantfit.identify(syn, "dyn", {"Cf": (50000.0, 110000.0)}, H, grid=5, rounds=2, dt_free=(0.01, 0.03), **kw)
    d = plantfit.identify(syn, "dyn", {"Cf": (50000.0, 110000.0), "dt": (0.01, 0.03)}, H, grid=5, rounds=2, **kw)
    assert c.values == d.values and c.cost == d.cost and 0.01 <= c.dt <= 0.03
    with pytest.raises(ValueError):
        plantfit.identify(syn, "dyn", {"Cf": (1.0, 2.0), "Cr": (1.0, 2.0), "m": (1.0, 2.0), "Iz": (1.0, 2.0)}, H, **kw)
    with pytest.raises(ValueError, match="unknown plant parameter"):
        plantfit.identify(syn, "dyn", {"stiffness": (1.0, 2.0)}, H, **kw)


def check_position_cost(kw):
    """One start: position_cost is the square of optimize_coeffs.py's _cost (numpy.linalg.norm of the position
    differences), computed from pred."""
    s, H = 50, 20
    for model in MODELS:
        r = ro.plant_rollout_errors(LOG, model, PARAMS, horizon=H, starts=[s], keep_pred=True, **kw)
        sim = LOG[:2, s + 1:s + 1 + H].T
        for i in range(3):
            pts = r.pred[i, :, :2, 0]
            ref = np.linalg.norm(sim - pts) ** 2
            got = r.position_cost()[i]
            assert abs(got - ref) <= 1e-12 * ref, (model, i, got, ref)
