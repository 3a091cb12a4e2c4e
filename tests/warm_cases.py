"""Shared by tests/test_warm_start.py, tests/test_gpu_warm_start.py and tests/golden/make_warm_golden.py: the primal
warm start (include/mpcracing.h mr_solve_batch_warm, mr_warm_shift).

* ``shift_numpy``: the shift rule of mr_warm_shift restated in numpy, one instance at a time -- the yardstick of
  the shift kernel and of its host twin, and what builds the guesses of the golden cases.
* ``host_solve`` / ``host_shift``: the host builds' entries (mrh_solve_batch[_scalar]_warm, mrh_warm_shift) on numpy
  arrays, with sentinel-prefilled outputs and guards as tests/horizon_cases.host_solve.
* the golden cases (tests/golden/warm_golden.npz, generator make_warm_golden.py): the oracle's
  solve_ipopt(p, w0=w, log=True, rules=PRODUCT) from each guess, and what a build's solve is held to against it
  (the bars of tests/ipopt_trace_cases.py, unchanged).
"""
import ctypes
import json
import os

import numpy as np

import horizon_cases as hc
import host_twin as ht
import ipopt_trace_cases as itc

HERE = os.path.dirname(os.path.abspath(__file__))
NPZ = os.path.join(HERE, "golden", "warm_golden.npz")
INDEX = os.path.join(HERE, "golden", "warm_golden.json")
OPTIONS = dict(tol=1e-8, acceptable_tol=1e-6, acceptable_iter=15, max_iter=500)
IN_KEYS = ("state0", "s0", "cx", "cy", "max_error", "runtime", "u_init")
SENTINEL = hc.SENTINEL

# case -> model, N (the new tick's horizon = the layout), previous horizon, lane rows, tyres, rough guess
CASES = {
    "a_dyn15": dict(model="dyn", N=15, Np=15, lane=False, tyres=None, rough=False),
    "b_kin8": dict(model="kin", N=8, Np=8, lane=False, tyres=None, rough=False),
    "c_blend16_from12": dict(model="blend", N=16, Np=12, lane=False, tyres=None, rough=False),
    "d_blendpac8": dict(model="blend_pacejka", N=8, Np=8, lane=False, tyres="pacejka-2", rough=False),
    "e_dynlane8": dict(model="dyn", N=8, Np=8, lane=True, tyres=None, rough=False),
    "f_dyn15_rough": dict(model="dyn", N=15, Np=15, lane=False, tyres=None, rough=True),
}
TS = 0.05


def case_tyres(case):
    from mpcracing import workload as wl
    t = CASES[case]["tyres"]
    return wl.tyre_coeffs(t) if t else None


def oracle_problem(case, sub, N=None):
    """oracle.nlp.MPCProblem of the B = 1 instance ``sub`` (ABI layout) under the case's configuration."""
    from mpcracing import workload as wl
    from oracle.nlp import MPCProblem
    c = CASES[case]
    inst = wl.instance_dicts(sub)[0]
    kw = {}
    if sub.get("u_init") is not None:  # MPCProblem shifts last_controls itself (make_ipopt_trace_golden.oracle_solve)
        cols = [(float(a), float(s)) for a, s in zip(*sub["u_init"][:, :, 0])]
        kw["last_controls"] = [(0.0, 0.0)] + cols[:-1]
    return MPCProblem(inst["state0"], inst["s0"], inst["cx"], inst["cy"], inst["max_error"], N=N or c["N"], Ts=TS,
                      model=c["model"], lane_bounds=c["lane"], tyres=case_tyres(case), **kw)


def model_step(prob):
    """x, u -> f(x, u): one step of the oracle's MPC model (oracle.dynamics through MPCProblem.F), fp64."""
    import torch
    from oracle import dynamics as dyn
    M = dyn._torch_ns()

    def step(x, u):
        xt = torch.tensor(np.asarray(x, np.float64)).reshape(6, 1)
        ut = torch.tensor(np.asarray(u, np.float64)).reshape(2, 1)
        return prob.F(xt, ut, M).reshape(6).numpy()
    return step


def shift_numpy(X, U, S, status, Np, Nn, state0_new, s0_new, step):
    """mr_warm_shift for one instance.  X [6][NL+1], U [2][NL], S [NL+1] of the previous tick (layout NL), its
    status and horizon Np; the new tick's state0 (rows 0..5 read), progress and horizon Nn; ``step(x, u)`` the MPC
    model.  Returns u_init [2][NL], x_init [6][NL+1], s_init [NL+1], use and the boolean rows of x_init that are
    extrapolated (the others are copies)."""
    NL = U.shape[1]
    hz_ok = 1 <= Np <= NL and 1 <= Nn <= NL
    Npc = min(max(Np, 1), NL)
    u_init = np.stack([U[:, min(k + 1, Npc - 1)] for k in range(NL)], axis=1)
    x_init = np.full((6, NL + 1), np.nan)
    s_init = np.full(NL + 1, np.nan)
    extrap = np.zeros(NL + 1, bool)
    ok = hz_ok and Np >= 2 and int(status) in (0, 1)
    if hz_ok:
        ok = ok and bool(np.isfinite(u_init[:, :Nn]).all())
        x, sk = np.array(state0_new[:6], np.float64), float(s0_new)
        with np.errstate(all="ignore"):
            for k in range(1, Nn + 1):
                if k + 1 <= Np:
                    x = X[:, k + 1].copy()
                    sk = s0_new + (S[k + 1] - S[1])
                else:
                    x = step(x, u_init[:, k - 1])
                    sk = sk + (S[Np] - S[Np - 1])
                    extrap[k] = True
                x_init[:, k], s_init[k] = x, sk
        ok = ok and bool(np.isfinite(x_init[:, 1:Nn + 1]).all() and np.isfinite(s_init[1:Nn + 1]).all())
    return u_init, x_init, s_init, int(ok), extrap


def w0_of(sub, x_init, s_init, N):
    """The oracle's start vector (U, S_hat, States: MPCProblem.split) of the B = 1 instance ``sub`` with the guess:
    X_0 = state0, S_0 = s0, rows 1..N from the guess, U = u_init (or throttle0 / steer0 repeated)."""
    u = sub["u_init"][:, :N, 0] if sub.get("u_init") is not None else np.repeat(sub["state0"][6:8, :1], N, axis=1)
    S = np.concatenate([sub["s0"][:1], s_init[1:N + 1]])
    X = np.concatenate([sub["state0"][:6, :1], x_init[:, 1:N + 1]], axis=1)
    return np.concatenate([u.reshape(-1), S, X.reshape(-1)])


# ---- the host builds ----

def _tyre_args(tyres):
    if tyres is None:
        return None, 0.0, None, 0.0, ()
    (af, Fzf), (ar, Fzr) = tyres
    af, ar = np.asarray(af, np.float64), np.asarray(ar, np.float64)
    PD = ctypes.POINTER(ctypes.c_double)
    return af.ctypes.data_as(PD), Fzf, ar.ctypes.data_as(PD), Fzr, (af, ar)


def host_solve(cfg, batch, horizon=None, warm=None, scalar=False, duals=False, tyres=None, nthreads=8,
               prefill=None, guard=0, trace_instance=-1, trace_cap=0, entry="warm"):
    """mrh_solve_batch[_scalar]_warm on numpy arrays (``entry="horizons"``: the _horizons entry, without a guess).
    ``warm``: None (a NULL mr_warm) or dict(x_init [6][N+1][B], s_init [N+1][B], use int32 [B] or absent); the
    outputs then carry ``used``.  Outputs are pre-filled with ``prefill`` (-1 in the integer ones) and followed by
    ``guard`` pre-filled elements (out["guard"]), as tests/horizon_cases.host_solve."""
    N = cfg.N
    B = batch["s0"].shape[0]
    arr = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in batch.items() if v is not None}
    inp = ht.abi.MRInputs(*[ht._p(arr.get(k)) for k in IN_KEYS])
    fill = 0.0 if prefill is None else prefill
    shapes = {"X": (6, N + 1, B), "U": (2, N, B), "S": (N + 1, B), "eC": (N, B), "eL": (N, B), "status": (B,),
              "iters": (B,), "obj": (B,), "kkt": (B,), "constr_viol": (B,)}
    if duals:
        shapes["lam_g"] = (13 * N + 9, B)
    if warm is not None:
        shapes["used"] = (B,)
    out, tails = {}, {}
    for k, shp in shapes.items():
        n = int(np.prod(shp))
        flat = np.full(n + guard, -1, np.int32) if k in ("status", "iters", "used") else np.full(n + guard, fill)
        out[k], tails[k] = flat[:n].reshape(shp), flat[n:]
    if trace_cap:
        out["trace"] = np.zeros((trace_cap, 8))
    o = ht.abi.MROutputs(*[ht._p(out.get(k)) for k in ("X", "U", "S", "eC", "eL", "status", "iters", "obj", "kkt",
                                                       "trace")], trace_instance, trace_cap, ht._p(out.get("lam_g")),
                         None, ht._p(out["constr_viol"]))
    pa, Fzf, pb, Fzr, _keep = _tyre_args(tyres)
    hz = None
    if horizon is not None:
        hz = np.ascontiguousarray(horizon, np.int32)
        assert hz.shape == (B,)
    hp = hz.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if hz is not None else None
    if entry == "horizons":
        assert warm is None
        fn = ht.lib().mrh_solve_batch_scalar_horizons if scalar else ht.lib().mrh_solve_batch_horizons
        rc = fn(ctypes.byref(cfg), pa, Fzf, pb, Fzr, B, ctypes.byref(inp), ctypes.byref(o), hp, nthreads)
    else:
        wp = None
        if warm is not None:
            wa = dict(x_init=np.ascontiguousarray(warm["x_init"], np.float64),
                      s_init=np.ascontiguousarray(warm["s_init"], np.float64),
                      use=None if warm.get("use") is None else np.ascontiguousarray(warm["use"], np.int32))
            assert wa["x_init"].shape == (6, N + 1, B) and wa["s_init"].shape == (N + 1, B)
            wm = ht.abi.MRWarm(ht._p(wa["x_init"]), ht._p(wa["s_init"]), ht._p(wa["use"]), ht._p(out["used"]))
            wp = ctypes.byref(wm)
        fn = ht.lib().mrh_solve_batch_scalar_warm if scalar else ht.lib().mrh_solve_batch_warm
        rc = fn(ctypes.byref(cfg), pa, Fzf, pb, Fzr, B, ctypes.byref(inp), ctypes.byref(o), hp, wp, nthreads)
    assert rc == 0
    if guard:
        out["guard"] = tails
    return out


def host_shift(cfg, X, U, S, status, horizon_prev, state0_new, s0_new, horizon_new, tyres=None):
    """mrh_warm_shift on numpy arrays of a batch (layout cfg.N).  Returns dict(u_init, x_init, s_init, use)."""
    N = cfg.N
    B = s0_new.shape[0]
    f = lambda a: np.ascontiguousarray(a, np.float64)  # noqa: E731
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, np.int32)  # noqa: E731
    a = [f(X), f(U), f(S), i32(status), i32(horizon_prev), f(state0_new), f(s0_new), i32(horizon_new)]
    assert a[0].shape == (6, N + 1, B) and a[1].shape == (2, N, B) and a[2].shape == (N + 1, B)
    out = dict(u_init=np.full((2, N, B), SENTINEL), x_init=np.full((6, N + 1, B), SENTINEL),
               s_init=np.full((N + 1, B), SENTINEL), use=np.full(B, -1, np.int32))
    pa, Fzf, pb, Fzr, _keep = _tyre_args(tyres)
    rc = ht.lib().mrh_warm_shift(ctypes.byref(cfg), pa, Fzf, pb, Fzr, B, *[ht._p(v) for v in a],
                                 *[ht._p(out[k]) for k in ("u_init", "x_init", "s_init", "use")])
    assert rc == 0
    return out


# ---- shift cases (no oracle solve: a made-up previous solution) ----

def shift_batch(NL=12, seed=5):
    """A batch for the shift kernel: per instance (Np, Nn, status), a smooth made-up previous solution whose rows
    beyond Np are NaN (as a solve returns them), and the new tick's state.  The instances: Np = Nn, Np < Nn
    (extrapolated tail), Np > Nn, the layout horizon on both sides, Np = 2 (the least that shifts), Np = 1,
    previous status 1, 2 and 3, a NaN in X_prev, and a progress that wrapped past the lap end between the ticks."""
    rows = [(8, 8, 0), (5, 9, 0), (12, 4, 0), (12, 12, 1), (2, 6, 0), (1, 3, 0), (8, 8, 2), (8, 8, 3), (8, 8, 0),
            (7, 12, 0)]
    B = len(rows)
    rng = np.random.default_rng(seed)
    X, U, S = np.full((6, NL + 1, B), np.nan), np.full((2, NL, B), np.nan), np.full((NL + 1, B), np.nan)
    state0, s0 = np.zeros((8, B)), np.zeros(B)
    for i, (Np, _Nn, _st) in enumerate(rows):
        k = np.arange(Np + 1)
        v = rng.uniform(8.0, 30.0)
        yaw = rng.uniform(-3.0, 3.0)
        X[:, :Np + 1, i] = [100.0 * i + v * TS * k * np.cos(yaw), -50.0 + v * TS * k * np.sin(yaw),
                            yaw + 0.01 * k, v + 0.1 * k, 0.05 * np.sin(k), 0.02 * np.cos(k)]
        U[:, :Np, i] = [rng.uniform(-0.3, 0.6, Np), rng.uniform(-0.2, 0.2, Np)]
        S[:Np + 1, i] = 300.0 + 40.0 * i + v * TS * k
        state0[:6, i] = X[:, 1, i] + rng.normal(0.0, 0.01, 6)
        state0[6:, i] = U[:, 0, i]
        s0[i] = S[1, i] + 0.02
    X[3, 4, 8] = np.nan  # instance 8: a NaN in a row the shift copies
    S[:, 9] += 5440.0 - S[1, 9]  # instance 9: the previous S_hat runs past the lap end (L = 5451 m) ...
    s0[9] = S[1, 9] + 0.02 - 5451.0  # ... and the measured progress of the new tick has wrapped
    return dict(X=X, U=U, S=S, status=np.array([r[2] for r in rows], np.int32),
                Np=np.array([r[0] for r in rows], np.int32), Nn=np.array([r[1] for r in rows], np.int32),
                state0=state0, s0=s0, use=np.array([1, 1, 1, 1, 1, 0, 0, 0, 0, 1], np.int32))


def check_shift(got, sb, step, label):
    """``got`` (dict u_init, x_init, s_init, use of the whole batch) against shift_numpy per instance: copied
    values and NaN rows bitwise, extrapolated States to 1e-13 relative (the bar of the dynamics values), the
    extrapolated progress bitwise (sums of copied values), the use flags equal."""
    worst = 0.0
    for i in range(sb["s0"].shape[0]):
        u, x, s, use, ex = shift_numpy(sb["X"][..., i], sb["U"][..., i], sb["S"][..., i], sb["status"][i],
                                       int(sb["Np"][i]), int(sb["Nn"][i]), sb["state0"][:, i], sb["s0"][i], step)
        assert use == sb["use"][i], (label, i, "the case's own expectation")
        assert int(got["use"][i]) == use, (label, i, int(got["use"][i]), use)
        assert hc.bit_equal(got["u_init"][..., i], u), (label, i, "u_init")
        assert hc.bit_equal(got["s_init"][:, i], s), (label, i, "s_init")
        gx = got["x_init"][..., i]
        assert hc.bit_equal(gx[:, ~ex], x[:, ~ex]), (label, i, "copied / NaN rows of x_init")
        if ex.any():
            with np.errstate(invalid="ignore"):
                d = np.abs(gx[:, ex] - x[:, ex]) / np.maximum(np.abs(x[:, ex]), 1e-300)
            d = np.where(gx[:, ex] == x[:, ex], 0.0, d)
            if np.isfinite(x[:, ex]).all():
                worst = max(worst, float(d.max()))
                assert d.max() <= 1e-13, (label, i, "extrapolated States", float(d.max()))
            else:
                assert np.array_equal(np.isfinite(gx[:, ex]), np.isfinite(x[:, ex])), (label, i)
    print(f"{label}: extrapolated States within {worst:.1e} relative")


# ---- the golden cases ----

_cache = {}


def fixture():
    """(arrays keyed "<case>/<name>", index keyed by case); loaded once and never modified."""
    if not _cache:
        with np.load(NPZ) as z:
            arrays = {k: z[k] for k in z.files}
        for v in arrays.values():
            v.setflags(write=False)
        with open(INDEX) as f:
            _cache["f"] = (arrays, json.load(f))
    return _cache["f"]


def case_batch(case):
    """(inputs of the new tick as a B = 1 batch, warm dict(x_init, s_init)) of a golden case."""
    arrays, _ = fixture()
    sub = {k: (np.array(arrays[f"{case}/in_{k}"]) if f"{case}/in_{k}" in arrays else None) for k in IN_KEYS}
    warm = dict(x_init=np.array(arrays[f"{case}/x_init"]), s_init=np.array(arrays[f"{case}/s_init"]))
    return sub, warm


def case_cfg(case, precision="fp64", **kw):
    c = CASES[case]
    opt = dict(OPTIONS)
    opt.update(kw)
    return ht.config(c["N"], c["model"], precision, c["lane"], TS, **opt)


def check_case(case, o, label):
    """A build's warm solve ``o`` (trace of instance 0, lam_g, used) of a golden case against the oracle's log: the
    trace at the bars of tests/ipopt_trace_cases.py, status and iterations equal, obj to 1e-10, lam_g to 1e-7 of
    its largest entry (the lane rows carry no Opti multiplier: case e is compared on the rows it shares)."""
    fx = fixture()
    assert int(o["used"][0]) == 1, (label, case, "the guess was not taken")
    itc.check_rows(case, o["trace"], label, fx=fx)
    itc.check_whole(case, o["status"][0], o["iters"][0], o["obj"][0], label, fx=fx)
    e = fx[1][case]
    assert (int(o["status"][0]), int(o["iters"][0])) == (e["status"], e["iters"]), (label, case)
    np.testing.assert_allclose(o["obj"][0], e["obj"], rtol=1e-10, err_msg=f"{label} {case}: objective")
    if "lam_g" in o:
        itc.check_lam_g(case, np.asarray(o["lam_g"])[:, 0], label, fx=fx)


# ---- a mixed batch: layout 16, horizons {2, 8, 15, 16}, warm and cold instances interleaved ----

MIXED_NL = 16
MIXED_NN = np.array([2, 8, 15, 16, 16, 15, 8, 2], np.int32)  # the new tick's horizons
MIXED_NP = np.array([4, 8, 15, 12, 16, 15, 6, 2], np.int32)  # the previous tick's (3, 6, 7: a tail to extrapolate)
MIXED_WANT = np.array([1, 0, 1, 1, 0, 1, 1, 1], np.int32)    # the caller's use flags: cold instances between warm ones
MIXED_MODEL = "dyn"


def mixed_batch():
    """(new tick's inputs [..][8] with u_init, warm dict(x_init, s_init, use), horizons): C2's first eight states
    under the dynamic model, one tick after a cold solve by the host scalar build (fp64) at the horizons MIXED_NP;
    the guess is shift_numpy's.  Built once, never modified."""
    if "mixed" not in _cache:
        from mpcracing import workload as wl
        from oracle.nlp import MPCProblem
        base = wl.make_batch("C2", limit=8)
        cfg = ht.config(MIXED_NL, MIXED_MODEL, "fp64", False, TS, **OPTIONS)
        prev = host_solve(cfg, base, horizon=MIXED_NP, scalar=True, entry="horizons")
        B = 8
        new = {k: (None if v is None else v.copy()) for k, v in base.items()}
        new["state0"][:6] = prev["X"][:, 1] + np.array([0.03, -0.02, 0.001, 0.04, 0.01, -0.003])[:, None]
        new["state0"][6:] = prev["U"][:, 0]
        new["s0"] = prev["S"][1] + 0.02
        inst = wl.instance_dicts(new)[0]
        step = model_step(MPCProblem(inst["state0"], inst["s0"], inst["cx"], inst["cy"], inst["max_error"],
                                     N=MIXED_NL, Ts=TS, model=MIXED_MODEL))
        u = np.zeros((2, MIXED_NL, B))
        x = np.zeros((6, MIXED_NL + 1, B))
        s = np.zeros((MIXED_NL + 1, B))
        use = np.zeros(B, np.int32)
        for i in range(B):
            u[..., i], x[..., i], s[..., i], use[i], _ex = shift_numpy(
                prev["X"][..., i], prev["U"][..., i], prev["S"][..., i], prev["status"][i], int(MIXED_NP[i]),
                int(MIXED_NN[i]), new["state0"][:, i], new["s0"][i], step)
        assert (use == 1).all(), (use, prev["status"])  # every previous solve converged: the pattern below decides
        new["u_init"] = u
        for v in list(new.values()) + [x, s]:
            if v is not None:
                v.setflags(write=False)
        _cache["mixed"] = (new, dict(x_init=x, s_init=s, use=MIXED_WANT.copy()), MIXED_NN.copy())
    return _cache["mixed"]


def one_warm(warm, i, N):
    """Instance i of a guess as the B = 1 guess of a solver with horizon N (rows cut to N + 1)."""
    return dict(x_init=np.ascontiguousarray(warm["x_init"][:, :N + 1, i:i + 1]),
                s_init=np.ascontiguousarray(warm["s_init"][:N + 1, i:i + 1]),
                use=None if warm.get("use") is None else np.ascontiguousarray(warm["use"][i:i + 1]))


# ---- the closed loop with the primal warm start, on the CPU ----

def closed_loop_run(cl, state0, ticks, N=15, start_control_at=2, dt=0.05, Ts=0.05, lookback=5.0, lookahead=45.0,
                    runtime=(1000.0, 0.85, 50.0, 2.0, 5000.0), plant_model="blend", solver_cfg=None):
    """tests/closed_loop_ref.run with ClosedLoop(warm_start="primal")'s start: from the second controlled tick on,
    shift_numpy of the previous solution (the oracle's dynamic model for the tail) and mrh_solve_batch_warm (the
    emulated wave).  Records as closed_loop_ref.run's, plus warm_used on the controlled ticks."""
    import math

    from oracle import plant
    from oracle.nlp import MPCProblem
    state = np.array(state0, dtype=np.float64)
    B = state.shape[1]
    prev, old_yaw = [None] * B, [None] * B
    cmd_thr, cmd_brake, cmd_steer = np.zeros(B), np.zeros(B), np.zeros(B)
    last = None
    rt = np.tile(np.asarray(runtime, dtype=np.float64).reshape(5, 1), (1, B))
    cfg = solver_cfg if solver_cfg is not None else ht.config(N, "dyn", "fp64", False, Ts)
    step_fn = None
    recs = []
    for step in range(ticks):
        X, Y, yaw, vx, vy = (state[j].copy() for j in range(5))
        yawdot = np.full(B, math.nan)
        for i in range(B):
            if old_yaw[i] is not None:
                d = yaw[i] - old_yaw[i]
                if d > 3:
                    d = yaw[i] - (old_yaw[i] + np.pi * 2)
                elif d < -3:
                    d = yaw[i] - (old_yaw[i] - np.pi * 2)
                yawdot[i] = d / dt
        sense = [plant.agent_sense(cl, float(X[i]), float(Y[i]), prev[i], lookback, lookahead) for i in range(B)]
        prog = np.array([r[0] for r in sense])
        rec = dict(step=step, X=X, Y=Y, yaw=yaw, vx=vx, vy=vy, yawdot=yawdot, progress=prog,
                   error=np.array([r[1] for r in sense]))
        if step >= start_control_at:
            thr0 = np.where(cmd_brake == 0, cmd_thr, -cmd_brake)
            batch = dict(state0=np.stack([X, Y, yaw, vx, vy, yawdot, thr0, cmd_steer]), s0=prog,
                         cx=np.array([r[2] for r in sense]).T, cy=np.array([r[3] for r in sense]).T,
                         max_error=np.array([r[4] for r in sense]), runtime=rt, u_init=None)
            warm = None
            if last is not None:
                if step_fn is None:
                    step_fn = model_step(MPCProblem(dict(x=0.0, y=0.0, yaw=0.0, v_x=10.0, v_y=0.0, yaw_dot=0.0,
                                                         throttle=0.0, steer=0.0), 0.0, [0.0] * 5, [0.0] * 5, 1.0,
                                                    N=N, Ts=Ts, model="dyn"))
                u, x, s = np.zeros((2, N, B)), np.zeros((6, N + 1, B)), np.zeros((N + 1, B))
                use = np.zeros(B, np.int32)
                for i in range(B):
                    u[..., i], x[..., i], s[..., i], use[i], _ex = shift_numpy(
                        last["X"][..., i], last["U"][..., i], last["S"][..., i], last["status"][i], N, N,
                        batch["state0"][:, i], prog[i], step_fn)
                batch["u_init"] = u
                warm = dict(x_init=x, s_init=s, use=use)
            out = host_solve(cfg, batch, warm=warm)
            last = out
            throttle, steer = out["U"][0, 0].copy(), out["U"][1, 0].copy()
            rec.update(status=out["status"].copy(), iters=out["iters"].copy(), U=out["U"].copy(),
                       warm_used=out["used"].copy() if warm is not None else np.zeros(B, np.int32))
        else:
            throttle, steer = np.full(B, 0.5), np.zeros(B)
        cmd_brake = np.where(throttle < 0, -throttle, 0.0)
        cmd_thr = np.where(throttle < 0, 0.0, throttle)
        cmd_steer = steer.copy()
        rec.update(cmd_throttle=cmd_thr.copy(), cmd_brake=cmd_brake.copy(), cmd_steer=cmd_steer.copy())
        state = np.array([plant.STEP[plant_model](list(state[:, i]), float(cmd_thr[i] - cmd_brake[i]),
                                                  float(cmd_steer[i]), dt) for i in range(B)]).T
        old_yaw = list(yaw)
        prev = list(prog)
        recs.append(rec)
    return recs, state
