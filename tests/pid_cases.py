"""Shared checks of the PID agent (csrc/mr_pid.h, mpcracing/pid.py): test_pid.py runs them on the host build
(``KW = dict(host_twin=True)``), test_gpu_pid.py on gfx950 (``KW = {}``).  Tracks are the reference-generated
splines of tests/golden/golden.npz (G1) without lane tables (the agent never reads them); the reference of the
fixture ticks is tests/golden/pid_golden.npz (generator make_pid_golden.py), the checker tests/pid_ref.py.

Shapes: n = 70 vehicles (one full wavefront and a 6-lane one) on Shanghai, T = 40 ticks, gains and plant
parameters per vehicle drawn within 10 % of the defaults (seeded).
"""
import functools
import os

import numpy as np

import pid_ref
from mpcracing import pid, rollout
from oracle import splines as osp

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "golden.npz"))
F = np.load(os.path.join(HERE, "golden", "pid_golden.npz"))
DRIVES = ["dyn_20", "dyn_150", "kin_20", "kin_150"]
SHANGHAI = "shanghai_intl_circuit"
N, T, DT = 70, 40, 0.05
MODELS = ["kin", "dyn", "blend"]


def tables(name):
    p = name + "/"
    return (G[p + "t"], G[p + "cx"], G[p + "cy"], float(G[p + "L"]), None, None)


_tracks = {}


def track(name, KW):
    """One track object per backend and name (host blob or DeviceTrack)"""
    key = (name, bool(KW.get("host_twin")))
    if key not in _tracks:
        _tracks[key] = pid._track(tables(name), bool(KW.get("host_twin")), 0)
    return _tracks[key]


@functools.lru_cache(maxsize=None)
def centerline(name):
    return osp.from_golden(G, name)


def same(a, b):
    """bit for bit (a NaN equals a NaN)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def close(a, b, tol):
    """|a - b| <= tol + tol |b|, NaN where b is NaN"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), nan) and \
        bool(np.all(np.abs(a[~nan] - b[~nan]) <= tol + tol * np.abs(b[~nan])))


def start_state(name, s0, v0=15.0, offset=0.0):
    """[6][n] on the centerline tangent at s0 (lateral offset along the normal), from the oracle's spline"""
    cl = centerline(name)
    cols = []
    for s, v, off in zip(*np.broadcast_arrays(np.atleast_1d(s0), v0, offset)):
        nx, ny = cl.unit_principal_normal(float(s))
        cols.append([cl.Gx(float(s)) + off * nx, cl.Gy(float(s)) + off * ny, cl.unit_tangent_yaw(float(s)), v, 0.0,
                     0.0])
    return np.array(cols, np.float64).T.copy()


@functools.lru_cache(maxsize=None)
def batch():
    """(state0 [6][70], progress0 [70], gains [70][8], params [70][22])"""
    rng = np.random.default_rng(20240611)
    L = float(G[SHANGHAI + "/L"])
    s0 = np.sort(rng.uniform(10.0, L - 10.0, N))
    x0 = start_state(SHANGHAI, s0, rng.uniform(8.0, 20.0, N), rng.uniform(-0.5, 0.5, N))
    g = pid.gains()[None] * (1 + 0.1 * rng.uniform(-1, 1, (N, 8)))
    q = np.tile(rollout.plant_params(), (N, 1))
    for f in ("m", "Cf", "Cr", "Iz"):
        q[:, rollout.PLANT_FIELDS.index(f)] *= 1 + 0.1 * rng.uniform(-1, 1, N)
    return x0, s0, g, q


def run(KW, model="blend", n=slice(None), ticks=T, shared=False, **kw):
    x0, s0, g, q = batch()
    g, q = (g[0], q[0]) if shared else (g[n], q[n])
    return pid.drive(track(SHANGHAI, KW), x0[:, n], ticks, gains=g, model=model, params=q, dt=DT,
                     progress0=s0[n], **kw, **KW)


def result_same(a, b, cols=slice(None)):
    assert sorted(a.rows) == sorted(b.rows)
    for k in a.rows:
        assert same(a.rows[k][:, cols], b.rows[k]), k
    assert same(a.state[:, cols], b.state) and same(a.mem[:, cols], b.mem)
    assert same(a.ticks_done[cols], b.ticks_done)


# ---- 1. teacher-forced parity with the reference's ticks ----
def fixture_ticks(drive):
    p = drive + "/"
    return {k[len(p):]: F[k] for k in F.files if k.startswith(p)}


def check_defaults(KW, default_fn):
    assert same(default_fn(), pid.gains()) and same(pid.gains(), [1.1, 15, 0.1, 0.1, 0.82954, 1.21341, 3.0, 40])
    assert pid.gains(kP_steer=5.0)[2] == 5.0
    try:
        pid.gains(kI=1.0)
    except ValueError as e:
        assert "unknown gain" in str(e)
    else:
        raise AssertionError("unknown gain accepted")


def lib_ticks(drive, KW):
    """the library's one-tick entry on every tick of a fixture drive: (out [8][120], mem [4][120])"""
    f = fixture_ticks(drive)
    out, mem = np.full((8, len(f["dt"])), np.nan), np.full((4, len(f["dt"])), np.nan)
    for dt in np.unique(f["dt"]):  # the agent's last_ts differs in its last bits from tick to tick
        m = f["dt"] == dt
        o, mm = pid.control(track("t4", KW), f["state"][m].T, f["mem"][m].T, pid.gains(), dt, **KW)
        out[:, m], mem[:, m] = o, mm
    return out, mem


def check_teacher_forced(drive, KW, tol=1e-12):
    f = fixture_ticks(drive)
    out, mem = lib_ticks(drive, KW)
    got = dict(zip(pid.OUT_ROWS, out))
    ref = dict(progress=f["progress"], error=f["error"], cmd_throttle=f["throttle"],
               cmd_steer=np.clip(f["steer"], -1, 1), cmd_brake=f["brake"], target_vel=f["target_vel"],
               kappa=f["kappa"], yawdot_fd=f["yawdot_fd"])
    bad = []
    for k in pid.OUT_ROWS:
        err = np.nanmax(np.abs(got[k] - ref[k]) / (1 + np.abs(ref[k])))
        print(f"{drive} {k}: max scaled error {err:.3e}")
        if not close(got[k], ref[k], tol):
            bad.append(k)
    assert not bad, bad
    # the memory the tick leaves is the next tick's input of the fixture
    assert close(mem[0], f["progress"], tol) and close(mem[1], f["error"], tol)
    assert close(mem[2], f["target_vel"] - np.hypot(f["state"][:, 3], f["state"][:, 4]), tol)
    assert same(mem[3], f["state"][:, 2])


def check_ref_teacher_forced(drive, tol=1e-12):
    f = fixture_ticks(drive)
    cl = centerline("t4")
    keys = dict(progress="progress", error="error", alpha="alpha", delta="delta", steer="steer", kappa="kappa",
                target_vel="target_vel", cmd_throttle="throttle", cmd_brake="brake", yawdot_fd="yawdot_fd")
    got = {k: [] for k in keys}
    for t in range(len(f["dt"])):
        o, _ = pid_ref.tick(cl, f["state"][t], f["mem"][t], pid.gains(), f["dt"][t])
        for k in keys:
            got[k].append(o[k])
    bad = [k for k, fk in keys.items() if not close(got[k], f[fk], tol)]
    assert not bad, bad


# ---- 2. free-running parity ----
FREE_T = 200
FREE_S0 = [1500.0, 2600.0]


@functools.lru_cache(maxsize=None)
def free_reference(model):
    """pid_ref + oracle.plant from both starts: rows name -> [200][2]"""
    x0 = start_state(SHANGHAI, FREE_S0)
    runs = [pid_ref.drive(centerline(SHANGHAI), model, x0[:, j], [s, 0.0, 0.0, np.nan], pid.gains(), FREE_T, DT)[0]
            for j, s in enumerate(FREE_S0)]
    return {k: np.stack([r[k] for r in runs], 1) for k in pid_ref.ROWS}


def check_free_running(model, KW, tol=1e-6):
    ref = free_reference(model)
    res = pid.drive(track(SHANGHAI, KW), start_state(SHANGHAI, FREE_S0), FREE_T, model=model, dt=DT,
                    progress0=FREE_S0, **KW)
    assert same(res.ticks_done, [FREE_T, FREE_T])
    bad = []
    for k in pid.LOG_ROWS:
        print(f"{model} {k}: max scaled error {np.nanmax(np.abs(res.rows[k] - ref[k]) / (1 + np.abs(ref[k]))):.3e}")
        if not close(res.rows[k], ref[k], tol):
            bad.append(k)
    assert not bad, bad


def check_against_host(model, KW, tol=1e-6):
    """the device drive of the batch against the host twin's"""
    dev, host = run(KW, model), run(dict(host_twin=True), model)
    assert same(dev.ticks_done, host.ticks_done) and same(host.ticks_done, np.full(N, T))
    bad = [k for k in pid.LOG_ROWS if not close(dev.rows[k], host.rows[k], tol)]
    assert not bad, bad
    assert close(dev.state, host.state, tol) and close(dev.mem, host.mem, tol)


# ---- 3. bitwise ----
def stepwise(KW, model, shared):
    """T launches of the one-tick entry and the plant step: (rows, state, mem)"""
    x0, s0, g, q = batch()
    g, q = (g[0], q[0]) if shared else (g, q)
    tr = track(SHANGHAI, KW)
    x = x0.copy()
    mem = np.zeros((4, N))
    mem[0], mem[3] = s0, np.nan
    rows = {k: [] for k in pid.LOG_ROWS}
    for _ in range(T):
        out, mem = pid.control(tr, x, mem, g, DT, **KW)
        for j, k in enumerate(pid.LOG_ROWS[:6]):
            rows[k].append(x[j])
        rows["yawdot_fd"].append(out[7])
        for j, k in enumerate(pid.OUT_ROWS[:7]):
            rows[k].append(out[j])
        x = rollout.plant_step(x, np.stack([out[2] - out[4], out[3]]), DT, model, q, **KW)
    return {k: np.stack(v) for k, v in rows.items()}, x, mem


def check_fused_equals_stepwise(model, shared, KW):
    res = run(KW, model, shared=shared)
    rows, x, mem = stepwise(KW, model, shared)
    assert same(res.ticks_done, np.full(N, T))
    for k in pid.LOG_ROWS:
        assert same(res.rows[k], rows[k]), k
    assert same(res.state, x) and same(res.mem, mem)
    assert np.isfinite(res.state).all()


def check_continuation(KW, model="blend"):
    whole = run(KW, model)
    x0, s0, g, q = batch()
    a = run(KW, model, ticks=25)
    b = pid.drive(track(SHANGHAI, KW), a.state, 15, gains=g, model=model, params=q, dt=DT, mem0=a.mem, **KW)
    for k in pid.LOG_ROWS:
        assert same(whole.rows[k], np.concatenate([a.rows[k], b.rows[k]])), k
    assert same(whole.state, b.state) and same(whole.mem, b.mem)
    assert same(a.ticks_done, np.full(N, 25)) and same(b.ticks_done, np.full(N, 15))


def check_alone_equals_batch(KW, model="blend"):
    whole = run(KW, model)
    for i in (0, 63, 64, 69):
        result_same(whole, run(KW, model, n=slice(i, i + 1)), cols=slice(i, i + 1))


def check_shared_equals_copies(KW, model="blend"):
    x0, s0, g, q = batch()
    shared = run(KW, model, shared=True)
    copies = pid.drive(track(SHANGHAI, KW), x0, T, gains=np.tile(g[0], (N, 1)), model=model,
                       params=np.tile(q[0], (N, 1)), dt=DT, progress0=s0, **KW)
    result_same(shared, copies)


def check_repeatable(KW, model="blend"):
    result_same(run(KW, model), run(KW, model))


def check_mask_subsets(KW, model="dyn"):
    whole = run(KW, model)
    for rows in (["progress"], ["kappa", "X"], ["yaw", "yawdot_fd", "cmd_brake", "target_vel"], pid.LOG_ROWS[1::2]):
        part = run(KW, model, rows=rows)
        assert sorted(part.rows) == sorted(rows)
        for k in rows:
            assert same(part.rows[k], whole.rows[k]), k
        assert same(part.state, whole.state) and same(part.mem, whole.mem) and same(part.ticks_done, whole.ticks_done)
    none = run(KW, model, rows=[])
    assert none.rows == {} and same(none.state, whole.state) and same(none.ticks_done, whole.ticks_done)


# ---- 4. the drive's log under the plant rollouts ----
def check_exact_rollouts(KW):
    q = rollout.plant_params(Cf=80000.0, Cr=50000.0)
    res = pid.drive(track(SHANGHAI, KW), start_state(SHANGHAI, [1500.0]), 80, model="dyn", params=q, dt=DT,
                    progress0=1500.0, **KW)
    assert res.ticks_done[0] == 80
    yaw = res.rows["yaw"][:, 0]
    assert yaw.min() >= 0.76 and yaw.max() <= 2.0  # never wraps: the unwrapped log is the plant's own yaw
    log = res.log(0, yawdot="plant")
    assert same(log[2], yaw)
    err = rollout.plant_rollout_errors(log, "dyn", params=q, dt=DT, horizon=12, **KW)
    assert np.all(err.count == 80 - 12)
    for c, name in enumerate(rollout.COMPONENTS):
        if name == "yaw":
            assert np.all(np.abs(err.min[..., c]) <= 1e-15) and np.all(np.abs(err.max[..., c]) <= 1e-15)
        else:
            assert np.all(err.min[..., c] == 0.0) and np.all(err.max[..., c] == 0.0), name


# ---- 5. edges ----
def check_steer_saturates(KW):
    x0, s0, g, q = batch()
    g = g.copy()
    g[:, 2] = 5.0
    res = pid.drive(track(SHANGHAI, KW), x0, T, gains=g, model="blend", params=q, dt=DT, progress0=s0, **KW)
    steer = res.rows["cmd_steer"]
    steer = steer[np.isfinite(steer)]
    assert np.all(np.abs(steer) <= 1.0) and np.any(steer == 1.0) and np.any(steer == -1.0)


def check_command_ranges(KW):
    for model in MODELS:
        res = run(KW, model)
        thr, brk = res.rows["cmd_throttle"], res.rows["cmd_brake"]
        assert np.all(thr * brk == 0) and np.all((brk == 0) | ((brk >= 0.5) & (brk <= 1)))
        assert np.all((thr >= 0) & (thr <= 1))
    assert np.any(brk > 0) and np.any(thr > 0)


def check_straight_track(KW):
    from scipy.interpolate import make_interp_spline
    s = np.linspace(0.0, 500.0, 101)
    sx, sy = make_interp_spline(s, s), make_interp_spline(s, np.zeros_like(s))
    tab = (sx.t, sx.c, sy.c, 500.0, None, None)
    x = np.array([[100.0], [0.2], [0.0], [15.0], [0.0], [0.0]])
    out, mem = pid.control(tab, x, [[100.0], [0.0], [0.0], [np.nan]], pid.gains(), DT, **KW)
    o = dict(zip(pid.OUT_ROWS, out[:, 0]))
    assert o["kappa"] == 0.0 and o["target_vel"] == 100.0
    assert abs(o["progress"] - 100.0) < 1e-4 and abs(abs(o["error"]) - 0.2) < 1e-9 and np.isnan(o["yawdot_fd"])


def check_nan_gain_stops_one_vehicle(KW, lane=5, model="blend"):
    x0, s0, g, q = batch()
    whole = run(KW, model)
    g = g.copy()
    g[lane, 4] = np.nan
    res = pid.drive(track(SHANGHAI, KW), x0, T, gains=g, model=model, params=q, dt=DT, progress0=s0, **KW)
    others = np.arange(N) != lane
    assert res.ticks_done[lane] == 0 and same(res.ticks_done[others], np.full(N - 1, T))
    for k in pid.LOG_ROWS:
        assert np.isnan(res.rows[k][:, lane]).all(), k
        assert same(res.rows[k][:, others], whole.rows[k][:, others]), k
    assert same(res.state[:, others], whole.state[:, others]) and same(res.mem[:, others], whole.mem[:, others])
    assert same(res.state[:, lane], x0[:, lane]) and same(res.mem[:, lane], [s0[lane], 0.0, 0.0, np.nan])


def check_global_first_projection(KW):
    """progress0 = NaN: tick 0 projects globally (the oracle's search, bit for bit), and the drive is that of
    progress0 = its result.  The two drives differ by one Brent run with other brackets: both locate the
    minimiser to scipy's xatol = 1e-5 (within ~2e-5 of each other), every row depends on the progress with a
    sensitivity of order 1 over 5 ticks, so the rows agree within 1e-4."""
    from oracle import plant
    s0 = np.array([20.0, 400.0, 900.0])
    x0 = start_state("t4", s0, 14.0, 0.3)
    tr = track("t4", KW)
    a = pid.drive(tr, x0, 5, model="dyn", dt=DT, progress0=None, **KW)
    for j in range(3):
        assert a.rows["progress"][0, j] == plant.projection(centerline("t4"), x0[0, j], x0[1, j], None)[0]
    b = pid.drive(tr, x0, 5, model="dyn", dt=DT, progress0=a.rows["progress"][0], **KW)
    assert same(a.ticks_done, [5, 5, 5]) and same(b.ticks_done, [5, 5, 5])
    for k in pid.LOG_ROWS:
        assert close(a.rows[k], b.rows[k], 1e-4), k


# ---- 6. fitness and the csv round trip ----
def check_evaluate_gains(KW):
    import torch
    from mpcracing import ga
    pop = np.array([[0.1, 0.1, 0.82954, 1.21341], [0.2, 0.05, 1.0, 1.0], [0.05, 0.2, 0.6, 1.5]])
    bounds = [100.0, 130.0, 160.0]
    times, res = pid.evaluate_gains(track(SHANGHAI, KW), pop, bounds, 70, v0=15.0, model="blend", dt=DT, **KW)
    assert times.shape == (3, 2) and sorted(res.rows) == ["progress"] and res.rows["progress"].shape == (70, 6)
    recs = [{"progress": torch.from_numpy(row.copy())} for row in res.rows["progress"]]
    ref = ga.segment_times(recs, np.tile(bounds[:-1], 3), np.tile(bounds[1:], 3), float(G[SHANGHAI + "/L"]), DT)
    assert same(times, ref.reshape(3, 2))
    assert np.isfinite(times).all() and np.all((times > 1.0) & (times < 3.5))  # 30 m at 10 to 25 m/s
    assert len(np.unique(times)) == 6  # the gains reach the vehicles
    full = np.tile(pid.gains(), (3, 1))
    full[:, 2:6] = pop
    assert same(pid.evaluate_gains(track(SHANGHAI, KW), full, bounds, 70, v0=15.0, dt=DT, **KW)[0], times)


def check_csv_round_trip(KW, tmp_path):
    res = run(KW, "blend", n=slice(3, 6))
    for i in (0, 2):
        res.write_run(str(tmp_path / f"run{i}"), i)
        back = rollout.load_log(str(tmp_path / f"run{i}" / "steps.csv"))
        assert same(back, res.log(i)) and np.isnan(back[5, 0]) and np.isfinite(back[5, 1:]).all()
        assert back.shape == (9, T) and np.all(back[8] == DT)
    assert same(res.log(1, yawdot="plant")[5], res.rows["yawdot"][:, 1])
