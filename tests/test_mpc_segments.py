"""The glue kernels of the MPC's segment drives (csrc/mr_mpcseg.h) through the host build, bit for bit against a
numpy restatement of their rules (include/mpcracing.h): the population's runtime vectors, the per-tick crossing
test and solve inputs, the applied command with one plant step.  The crossing times are also held to
``ga.crossing_times`` on the same progress rows, the plant step to ``rollout.plant_step``.  No GPU."""
import ctypes

import numpy as np
import pytest

from mpcracing import abi, ga, rollout

NMEM = abi.MR_MPCSEG_NMEM
OLD_YAW, PREV_PROGRESS, CMD_THROTTLE, CMD_STEER, CMD_BRAKE, TRAVELLED_PREV = range(6)
SENTINEL = 777.0  # what the caller's arrays hold where a kernel must not write


@pytest.fixture(scope="module")
def lib():
    return abi.load_host_twin()


def p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def eq(a, b):
    """bitwise equality, NaN == NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- the restatement
def travelled_of(progress, s_start, L):
    tr = np.mod(progress - s_start, L)
    return np.where(tr > 0.5 * L, tr - L, tr)


def ref_runtime(genes, lo, hi, K, d_max):
    rt = np.repeat(lo[None, :] + genes * (hi - lo)[None, :], K, axis=0).T.copy()
    if not np.isnan(d_max):
        rt[1] = d_max
    return rt


def ref_inputs(tick, dt, L, K, N, state, progress, mem, s_start, s_end, U_prev, hz_prev, hz_in, speed, out):
    """out: dict of state0, u_init, horizon, done, times, ticks_done, updated in place like the kernel's arrays"""
    n = state.shape[1]
    seg = np.arange(n) % K
    was_done = out["done"] != 0
    need = np.mod(s_end - s_start, L)[seg]
    with np.errstate(invalid="ignore", divide="ignore"):
        c = travelled_of(progress, s_start[seg], L)
        lost = ~np.isfinite(progress)
        fin = ~was_done & (lost | (c >= need))
        a = mem[TRAVELLED_PREV]
        tm = dt * ((tick - 1) + (need - a) / (c - a))
        tm = np.where(lost | (tick == 0), np.inf, tm)
    out["times"][fin] = tm[fin]
    out["ticks_done"][fin] = tick + 1
    out["done"][fin] = 1
    on = ~was_done & ~fin
    out["horizon"][~on] = 0
    yaw, old = state[2], mem[OLD_YAW]
    with np.errstate(invalid="ignore"):
        d = yaw - old
        d = np.where(d > 3, yaw - (old + np.pi * 2), np.where(d < -3, yaw - (old - np.pi * 2), d))
        yawdot = d * (1.0 / dt)  # a division by a host scalar as torch evaluates it on the device
    thr0 = np.where(mem[CMD_BRAKE] == 0, mem[CMD_THROTTLE], -mem[CMD_BRAKE])
    s0 = np.stack([state[0], state[1], yaw, state[3], state[4], yawdot, thr0, mem[CMD_STEER]])
    out["state0"][:, on] = s0[:, on]
    if U_prev is not None:
        Np = np.full(n, N) if hz_prev is None else hz_prev
        for i in np.nonzero(on)[0]:
            for k in range(N):
                out["u_init"][:, k, i] = U_prev[:, min(k + 1, Np[i] - 1), i]
    if hz_in is not None:
        hz = hz_in.copy()
    elif speed is not None:
        lookahead, Ts, hz_min = speed
        with np.errstate(invalid="ignore"):
            h = np.clip(np.ceil((1.0 / (Ts * np.maximum(state[3], 1e-3))) * lookahead), hz_min, N)
        hz = np.where(np.isnan(h), 0, h).astype(np.int32)
    else:
        hz = np.full(n, N, np.int32)
    out["horizon"][on] = hz[on]


def ref_apply(model, dt, L, K, N, state, mem, progress, s_start, done, U, params):
    n = state.shape[1]
    thr = U[0, 0] if U is not None else np.full(n, 0.5)
    steer = U[1, 0] if U is not None else np.zeros(n)
    brake = np.where(thr < 0, -thr, 0.0)
    cthr = np.where(thr < 0, 0.0, thr)
    new = rollout.plant_step(state, np.stack([cthr - brake, steer]), dt, model, params, host_twin=True)
    on = done == 0
    mem[OLD_YAW, on] = state[2, on]
    mem[PREV_PROGRESS, on] = progress[on]
    mem[CMD_THROTTLE, on] = cthr[on]
    mem[CMD_STEER, on] = steer[on]
    mem[CMD_BRAKE, on] = brake[on]
    with np.errstate(invalid="ignore"):
        mem[TRAVELLED_PREV, on] = travelled_of(progress, s_start[np.arange(n) % K], L)[on]
    state[:, on] = new[:, on]


# ---------------------------------------------------------------- the host build
def call_inputs(lib, tick, dt, L, K, N, state, progress, mem, s_start, s_end, U_prev, hz_prev, hz_in, speed, out):
    n = state.shape[1]
    lookahead, Ts, hz_min = speed if speed is not None else (0.0, 0.05, 1)
    rc = lib.mrh_mpcseg_inputs(n, K, N, tick, dt, L, p(state), p(progress), p(mem), p(s_start), p(s_end), p(U_prev),
                               p(hz_prev), p(hz_in), lookahead, Ts, hz_min, p(out["state0"]),
                               p(out["u_init"]) if U_prev is not None else None, p(out["horizon"]), p(out["done"]),
                               p(out["times"]), p(out["ticks_done"]))
    assert rc == 0, lib.mrh_tyrefit_last_error()


def call_apply(lib, model, dt, L, K, N, state, mem, progress, s_start, done, U, params):
    n = state.shape[1]
    q = None if params is None else np.ascontiguousarray(np.atleast_2d(params))
    rc = lib.mrh_mpcseg_apply(abi.MR_PLANT[model], n, K, N, dt, L, p(state), p(mem), p(progress), p(s_start),
                              p(done), p(U), 0 if q is None else q.shape[0], p(q))
    assert rc == 0, lib.mrh_tyrefit_last_error()


def outputs(n, N, T):
    return dict(state0=np.full((8, n), SENTINEL), u_init=np.full((2, N, n), SENTINEL),
                horizon=np.full(n, -5, np.int32), done=np.zeros(n, np.int32), times=np.full(n, np.inf),
                ticks_done=np.full(n, T, np.int32))


def start_state(n, rng):
    s = np.zeros((6, n))
    s[0], s[1] = rng.uniform(-50, 50, n), rng.uniform(-50, 50, n)
    s[2] = rng.uniform(-np.pi, np.pi, n)
    s[3], s[4], s[5] = rng.uniform(0.5, 25, n), rng.uniform(-0.5, 0.5, n), rng.uniform(-0.3, 0.3, n)
    return s


def start_mem(n):
    m = np.zeros((NMEM, n))
    m[OLD_YAW] = m[PREV_PROGRESS] = np.nan
    return m


L_TRACK = 100.0
# the segments: one that wraps the lap end among them
SEGS = {1: ([20.0], [26.0]), 3: ([20.0, 95.0, 50.0], [26.0, 5.0, 58.0]),
        5: ([20.0, 95.0, 50.0, 0.0, 70.0], [26.0, 5.0, 58.0, 7.5, 79.0])}
KINDS = ["cross", "behind", "at_once", "lost", "never", "cross_slow"]


def progress_rows(n, K, T, dt, rng):
    """[T][n] synthetic sensed progress: vehicle i is of kind KINDS[i % 6] on segment i % K"""
    s_start, s_end = (np.array(a) for a in SEGS[K])
    prog = np.zeros((T, n))
    kinds = []
    for i in range(n):
        kind = KINDS[i % len(KINDS)]
        kinds.append(kind)
        s0, need = s_start[i % K], np.mod(s_end[i % K] - s_start[i % K], L_TRACK)
        v = rng.uniform(18.0, 30.0)
        off = rng.uniform(0.0, 0.2)
        if kind == "behind":
            off = -rng.uniform(0.001, 0.05)  # the first projection just behind the start
        elif kind == "at_once":
            off = need + rng.uniform(0.0, 1.0)  # beyond the end at tick 0
        elif kind == "never":
            v = 0.5
        elif kind == "cross_slow":
            v = rng.uniform(16.5, 18.0)  # the 10 m segment takes nearly all 14 ticks
        prog[:, i] = np.mod(s0 + off + v * dt * np.arange(T), L_TRACK)
        if kind == "lost":
            prog[2 + i % 3:, i] = np.nan
    return prog, kinds, s_start, s_end


@pytest.mark.parametrize("N", [1, 15])
@pytest.mark.parametrize("n", [1, 63, 65, 130])
@pytest.mark.parametrize("mode", ["plain", "speed", "fixed"])
def test_drive_matches_restatement(lib, n, N, mode):
    """T ticks of inputs -> apply on synthetic progress rows and random controls: every array of the host build
    equals the restatement's after every tick; the times are ``ga.crossing_times`` of the rows."""
    rng = np.random.default_rng(100 * n + N)
    K = 1 if n == 1 else (3 if n == 63 else 5)
    T, dt = 14, 0.05
    prog, kinds, s_start, s_end = progress_rows(n, K, T, dt, rng)
    model = ["kin", "dyn", "blend"][(n + N) % 3]
    state = start_state(n, rng)
    mem = start_mem(n)
    if mode == "speed":
        state[3, ::7] = 1e-5  # below the rule's floor
    state_r, mem_r = state.copy(), mem.copy()
    out, out_r = outputs(n, N, T), outputs(n, N, T)
    hz_in = rng.integers(1, N + 1, n).astype(np.int32) if mode == "fixed" else None
    speed = (20.0, 0.05, min(5, N)) if mode == "speed" else None
    hz_hist, U = [], None
    for t in range(T):
        # the previous tick's controls with NaN beyond its horizon, as the solve leaves them
        U_prev, hz_prev = (U, hz_hist[-1]) if t >= 2 else (None, None)
        if U_prev is not None and mode == "plain" and t % 2:
            hz_prev = None  # NULL: N
        args = (t, dt, L_TRACK, K, N, state, prog[t].copy(), mem, s_start, s_end, U_prev,
                None if hz_prev is None else np.maximum(hz_prev, 1).astype(np.int32), hz_in, speed)
        call_inputs(lib, *args, out)
        ref_inputs(*args[:5], state_r, prog[t].copy(), mem_r, *args[8:], out_r)
        on = out_r["horizon"] > 0
        for k in ("horizon", "done", "times", "ticks_done"):
            assert eq(out[k], out_r[k]), (t, k)
        assert eq(out["state0"][:, on], out_r["state0"][:, on]), t
        if U_prev is not None:
            assert eq(out["u_init"][:, :, on], out_r["u_init"][:, :, on]), t
        assert eq(out["horizon"] == 0, out["done"] != 0)
        hz_hist.append(out["horizon"].copy())
        U = None
        if t >= 1:
            U = rng.uniform(-1, 1, (2, N, n))
            for i in range(n):
                U[:, out["horizon"][i]:, i] = np.nan
        before = state.copy(), mem.copy()
        call_apply(lib, model, dt, L_TRACK, K, N, state, mem, prog[t].copy(), s_start, out["done"], U, None)
        ref_apply(model, dt, L_TRACK, K, N, state_r, mem_r, prog[t], s_start, out_r["done"], U, None)
        assert eq(state, state_r) and eq(mem, mem_r), t
        fin = out["done"] != 0
        assert eq(state[:, fin], before[0][:, fin]) and eq(mem[:, fin], before[1][:, fin]), t
    seg = np.arange(n) % K
    with np.errstate(invalid="ignore"):
        want = ga.crossing_times(prog, s_start[seg], s_end[seg], L_TRACK, dt)
    assert eq(out["times"], want)
    for i, kind in enumerate(kinds):
        if kind in ("cross", "behind", "cross_slow"):
            assert np.isfinite(out["times"][i]) and 2 <= out["ticks_done"][i] <= T, (i, kind)
        elif kind == "at_once":
            assert out["times"][i] == np.inf and out["ticks_done"][i] == 1 and out["done"][i] == 1
        elif kind == "lost":
            assert out["times"][i] == np.inf and out["ticks_done"][i] == 3 + i % 3 and out["done"][i] == 1
        else:
            assert out["times"][i] == np.inf and out["ticks_done"][i] == T and out["done"][i] == 0


def test_behind_start_is_negative_travelled(lib):
    """A first projection slightly behind the start counts as negative distance, not as a lap: the vehicle
    drives on, and its crossing interpolates from that negative value."""
    s_start, s_end = np.array([95.0]), np.array([5.0])  # wraps the lap end
    dt, T = 0.05, 3
    prog = np.array([[94.99], [99.0], [5.5]])
    state, mem, out = start_state(1, np.random.default_rng(0)), start_mem(1), outputs(1, 15, T)
    for t in range(T):
        call_inputs(lib, t, dt, L_TRACK, 1, 15, state, prog[t].copy(), mem, s_start, s_end, None, None, None, None,
                    out)
        call_apply(lib, "blend", dt, L_TRACK, 1, 15, state, mem, prog[t].copy(), s_start, out["done"], None, None)
        if t == 0:
            assert out["done"][0] == 0 and mem[TRAVELLED_PREV, 0] == np.mod(94.99 - 95.0, 100.0) - 100.0 < 0
    a, c = np.mod(99.0 - 95.0, 100.0), np.mod(5.5 - 95.0, 100.0)
    assert out["times"][0] == dt * (1 + (10.0 - a) / (c - a)) and out["ticks_done"][0] == 3


def test_yaw_rate_wraps_and_brake_feeds_back(lib):
    """The wrapped finite difference just beyond +-3, not at 3 itself, NaN for the first tick; a braking command
    comes back as a negative throttle."""
    old = np.array([-1.5, 1.5, -1.5, 0.25, np.nan, 3.1, -3.1])
    yaw = np.array([1.5000001, -1.5000001, 1.5, 0.2, 0.3, -3.1, 3.1])
    n, N, dt = len(old), 15, 0.05
    state, mem = start_state(n, np.random.default_rng(1)), start_mem(n)
    state[2], mem[OLD_YAW] = yaw, old
    mem[CMD_THROTTLE] = [0.4, 0.0, 0.0, 0.7, 0.1, 0.0, 0.2]
    mem[CMD_BRAKE] = [0.0, 0.6, 0.0, 0.0, 0.0, 1.0, 0.3]
    mem[CMD_STEER] = np.linspace(-0.3, 0.3, n)
    s_start, s_end, prog = np.array([20.0]), np.array([60.0]), np.full(n, 21.0)
    out, out_r = outputs(n, N, 4), outputs(n, N, 4)
    args = (1, dt, L_TRACK, 1, N, state, prog, mem, s_start, s_end, None, None, None, None)
    call_inputs(lib, *args, out)
    ref_inputs(*args, out_r)
    assert eq(out["state0"], out_r["state0"]) and (out["horizon"] == N).all()
    yd = out["state0"][5]
    assert yd[0] == (1.5000001 - (-1.5 + np.pi * 2)) * (1.0 / dt) and yd[0] < 0
    assert yd[1] == (-1.5000001 - (1.5 - np.pi * 2)) * (1.0 / dt) and yd[1] > 0
    assert yd[2] == 3.0 * (1.0 / dt) and np.isnan(yd[4])
    assert abs(yd[5] * dt - (2 * np.pi - 6.2)) < 1e-12 and abs(yd[6] * dt + (2 * np.pi - 6.2)) < 1e-12
    assert eq(out["state0"][6], np.array([0.4, -0.6, 0.0, 0.7, 0.1, -1.0, -0.3]))
    assert eq(out["state0"][7], mem[CMD_STEER])


@pytest.mark.parametrize("N", [1, 15])
def test_u_init_gather(lib, N):
    """u_init[:, k, i] = U_prev[:, min(k + 1, Np_i - 1), i] for Np_i in {1, 2, N}: NaN rows beyond Np_i are never
    picked."""
    n, dt = 9, 0.05
    rng = np.random.default_rng(2)
    Np = np.array([1, 2, N] * 3, np.int32).clip(1, N)
    U = rng.uniform(-1, 1, (2, N, n))
    for i in range(n):
        U[:, Np[i]:, i] = np.nan
    state, mem, out = start_state(n, rng), start_mem(n), outputs(n, N, 4)
    call_inputs(lib, 2, dt, L_TRACK, 1, N, state, np.full(n, 21.0), mem, np.array([20.0]), np.array([60.0]), U, Np,
                None, None, out)
    for i in range(n):
        for k in range(N):
            assert eq(out["u_init"][:, k, i], U[:, min(k + 1, Np[i] - 1), i])
    assert np.isfinite(out["u_init"]).all()


def test_done_vehicle_is_left_alone(lib):
    """done != 0: inputs writes horizon 0 and nothing else, apply nothing at all."""
    n, N, dt = 65, 15, 0.05
    rng = np.random.default_rng(3)
    state, mem, out = start_state(n, rng), start_mem(n), outputs(n, N, 9)
    mem[OLD_YAW], mem[PREV_PROGRESS] = rng.uniform(-1, 1, n), 20.5
    out["done"][::2] = 1
    out["times"][:] = 1.25
    fin = out["done"] != 0
    U_prev, U = rng.uniform(-1, 1, (2, N, n)), rng.uniform(-1, 1, (2, N, n))
    s_start, s_end, prog = np.array([20.0]), np.array([60.0]), np.full(n, 21.0)
    call_inputs(lib, 3, dt, L_TRACK, 1, N, state, prog, mem, s_start, s_end, U_prev, None, None, None, out)
    assert (out["horizon"][fin] == 0).all() and (out["horizon"][~fin] == N).all()
    assert (out["state0"][:, fin] == SENTINEL).all() and (out["u_init"][:, :, fin] == SENTINEL).all()
    assert (out["times"] == 1.25).all() and (out["ticks_done"] == 9).all() and eq(out["done"] != 0, fin)
    s_b, m_b = state.copy(), mem.copy()
    call_apply(lib, "blend", dt, L_TRACK, 1, N, state, mem, prog, s_start, out["done"], U, None)
    assert eq(state[:, fin], s_b[:, fin]) and eq(mem[:, fin], m_b[:, fin])
    assert (state[:, ~fin] != s_b[:, ~fin]).any(axis=0).all() and (mem[PREV_PROGRESS, ~fin] == 21.0).all()


@pytest.mark.parametrize("params", ["default", "shared", "per_vehicle"])
@pytest.mark.parametrize("model", ["kin", "dyn", "blend"])
def test_apply_plant_step_is_plant_step_params(lib, model, params):
    """apply's plant step is ``rollout.plant_step`` (mr_plant_step_params) bitwise: no parameters (the
    defaults), one vector, one per vehicle; braking and the uncontrolled tick's (0.5, 0.0) included."""
    n, N, dt = 65, 4, 0.05
    rng = np.random.default_rng(4)
    q = None
    if params == "shared":
        q = rollout.plant_params(m=1700.0, Cf=70000.0, lf=0.9)
    elif params == "per_vehicle":
        q = np.tile(rollout.plant_params(), (n, 1))
        q[:, rollout.PLANT_FIELDS.index("m")] = rng.uniform(1500, 2000, n)
        q[:, rollout.PLANT_FIELDS.index("Cr")] = rng.uniform(5e4, 8e4, n)
    for U in (rng.uniform(-1, 1, (2, N, n)), None):
        state, mem = start_state(n, rng), start_mem(n)
        s_b = state.copy()
        call_apply(lib, model, dt, L_TRACK, 1, N, state, mem, np.full(n, 21.0), np.array([20.0]),
                   np.zeros(n, np.int32), U, q)
        thr = U[0, 0] if U is not None else np.full(n, 0.5)
        steer = U[1, 0] if U is not None else np.zeros(n)
        want = rollout.plant_step(s_b, np.stack([thr, steer]), dt, model, q, host_twin=True)
        assert eq(state, want)
        assert eq(mem[CMD_BRAKE], np.where(thr < 0, -thr, 0.0)) and eq(mem[CMD_THROTTLE], np.where(thr < 0, 0.0, thr))
        assert eq(mem[CMD_STEER], steer) and eq(mem[OLD_YAW], s_b[2]) and eq(mem[TRAVELLED_PREV], np.full(n, 1.0))


def test_runtime_vectors(lib):
    """runtime[d][ind K + k] = lo[d] + genes[ind][d] (hi[d] - lo[d]); the d_max override; a zero-width range."""
    rng = np.random.default_rng(5)
    for n_ind, K in ((1, 1), (7, 3), (26, 5)):
        genes = rng.uniform(0, 1, (n_ind, 5))
        lo = np.array([200.0, 0.5, 50.0, 1.0, 1000.0])
        hi = np.array([2000.0, 1.5, 50.0, 4.0, 9000.0])  # q_v_y: zero width
        for d_max in (np.nan, 0.85):
            rt = np.full((5, n_ind * K), SENTINEL)
            assert lib.mrh_mpcseg_runtime(n_ind, K, p(genes), p(lo), p(hi), d_max, p(rt)) == 0
            assert eq(rt, ref_runtime(genes, lo, hi, K, d_max))
            assert (rt[2] == 50.0).all() and (np.isnan(d_max) or (rt[1] == 0.85).all())
            for ind in range(n_ind):
                for k in range(K):
                    assert rt[0, ind * K + k] == lo[0] + genes[ind, 0] * (hi[0] - lo[0])


def test_argument_checks(lib):
    n, N = 4, 15
    state, mem, out = start_state(n, np.random.default_rng(6)), start_mem(n), outputs(n, N, 4)
    one = np.array([20.0])
    base = [n, 1, N, 0, 0.05, L_TRACK, p(state), p(np.full(n, 21.0)), p(mem), p(one), p(one), None, None, None, 0.0,
            0.05, 1, p(out["state0"]), None, p(out["horizon"]), p(out["done"]), p(out["times"]), p(out["ticks_done"])]
    assert lib.mrh_mpcseg_inputs(*base) == 0
    for idx, bad in ((1, 0), (2, 0), (4, 0.0), (5, np.inf), (11, p(out["u_init"]))):
        a = list(base)
        a[idx] = bad
        assert lib.mrh_mpcseg_inputs(*a) != 0, idx
    a = list(base)
    a[14], a[16] = 20.0, N + 1  # the speed rule with hz_min beyond N
    assert lib.mrh_mpcseg_inputs(*a) != 0
    ok = [2, n, 1, N, 0.05, L_TRACK, p(state), p(mem), p(np.full(n, 21.0)), p(one), p(out["done"]), None, 0, None]
    assert lib.mrh_mpcseg_apply(*ok) == 0
    for idx, bad in ((0, 3), (4, -1.0), (12, 1)):
        a = list(ok)
        a[idx] = bad
        assert lib.mrh_mpcseg_apply(*a) != 0, idx
