"""The MPC's segment drives and the weight-tuning GA on the GPU (mpcracing/mpc.py, csrc/mr_mpcseg.h).

``mpc.segment_times`` against ``ga.evaluate_population`` -- the same vehicles through ``ClosedLoop``, every one
solved on every tick, the crossing times found on the host -- bit for bit, ``inf`` included: a vehicle's solve
does not depend on its batch neighbours or on the dispatch order (tests/test_gpu_warm_start.py), and a
full-horizon instance under ``mr_solve_batch_horizons`` has ``mr_solve_batch``'s bits
(tests/test_gpu_horizons.py), so leaving finished vehicles out of the solve changes nothing for the others.
``mpc.tune_weights`` against a loop of ``mpc.segment_times`` and ``ga.breed`` written here.

Shapes of tests/test_gpu_closed_loop.py::test_ga_evaluate_population_matches_cpu_loop with a third segment of
60 m that no vehicle can cover in the 2 s of the drive."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TRACK = "shanghai_intl_circuit"
N, TICKS, V0, DT = 15, 40, 14.0, 0.05
POP = np.array([[1000.0, 0.85, 50.0, 2.0, 5000.0],     # RuntimeControllerParameters defaults
                [600.0, 0.85, 20.0, 3.0, 2000.0]])
BOUNDS = np.array([120.0, 135.0, 150.0, 210.0])
SOLVER = dict(tol=1e-10, acceptable_iter=0)
MODES = {"plain": {}, "plant_dyn": dict(plant="dyn"),
         "speed_primal": dict(horizon="speed", warm_start="primal"), "poll": dict(poll_every=4)}


@pytest.fixture(scope="module")
def dtrack():
    from mpcracing.geometry import DeviceTrack
    return DeviceTrack(TRACK)


_REF = {}


def reference(dtrack, mode):
    """``ga.evaluate_population`` of the mode (once per distinct drive): its times, the records' progress [T][B]
    and states [T+1][5][B] -- the last row from a second drive of one more tick, whose first T ticks are the
    same drive."""
    from mpcracing import ga
    kw = {k: v for k, v in MODES[mode].items() if k != "poll_every"}
    key = tuple(sorted(kw.items()))
    if key not in _REF:
        times, recs = ga.evaluate_population(dtrack, POP, BOUNDS, TICKS, v0=V0, N=N, **SOLVER, **kw)
        _, more = ga.evaluate_population(dtrack, POP, BOUNDS, TICKS + 1, v0=V0, N=N, **SOLVER, **kw)
        prog = np.stack([r["progress"].cpu().numpy() for r in recs])
        states = np.stack([np.stack([r[k].cpu().numpy() for k in ("X", "Y", "yaw", "vx", "vy")]) for r in more])
        assert np.array_equal(prog, np.stack([r["progress"].cpu().numpy() for r in more[:TICKS]]), equal_nan=True)
        _REF[key] = times, prog, states
    return _REF[key]


@pytest.mark.parametrize("mode", list(MODES))
def test_segment_times_match_evaluate_population(dtrack, mode):
    from mpcracing import mpc
    want, prog, states = reference(dtrack, mode)
    times, ticks_done, final = mpc.segment_times(dtrack, POP, BOUNDS, TICKS, v0=V0, N=N, **SOLVER, **MODES[mode])
    P, K = POP.shape[0], len(BOUNDS) - 1
    print(mode, "times", times.tolist(), "ticks_done", ticks_done.tolist())
    assert times.shape == (P, K) and ticks_done.shape == (P, K) and final.shape == (6, P * K)
    # not all inf: the default individual covers the two 15 m segments, nobody the 60 m one
    assert np.isfinite(want[0, :2]).all() and np.isinf(want[:, 2]).all(), want
    assert np.array_equal(times, want), (times, want)
    # ticks_done - 1 is the first record tick whose progress has passed the segment's end
    s0, s1 = np.tile(BOUNDS[:-1], P), np.tile(BOUNDS[1:], P)
    L = dtrack.length
    tr = np.mod(prog - s0[None, :], L)
    tr = np.where(tr > 0.5 * L, tr - L, tr)
    passed = tr >= np.mod(s1 - s0, L)[None, :]
    for i in range(P * K):
        hit = np.nonzero(passed[:, i])[0]
        if np.isfinite(times.flat[i]):
            assert len(hit) and ticks_done.flat[i] - 1 == hit[0], (i, ticks_done.flat[i], hit[:1])
            # neither solved nor stepped after the crossing tick: the state that record started from
            assert np.array_equal(final[:5, i], states[hit[0], :, i]), i
        else:
            assert not len(hit) and ticks_done.flat[i] == TICKS, (i, ticks_done.flat[i])
            assert np.array_equal(final[:5, i], states[TICKS, :, i]), i  # driven to the end
    assert np.isfinite(final).all()


TUNE = dict(islands=1, population=2, pairs=1, seed=3, ticks=TICKS, v0=V0, N=N, keep_times=True, **SOLVER)
RANGES = {"alpha_c": (400.0, 1600.0), "q_v_y": (10.0, 90.0), "n": (1.0, 4.0), "beta_delta": (1000.0, 9000.0)}


def test_tune_weights_matches_loop_of_segment_times_and_breed(dtrack):
    """G = 2, I = 1, P = 2, K = 2: the gene mapping, the reset between the generations and the carried averages,
    against the generations written out; a second call gives the same bits."""
    from mpcracing import ga, mpc
    bounds, G, P = BOUNDS[:3], 2, 2
    K = len(bounds) - 1
    res = mpc.tune_weights(dtrack, bounds, G, RANGES, **TUNE)
    names = ["alpha_c", "q_v_y", "n", "beta_delta"]
    assert res.genes == names
    cols = [mpc.RUNTIME_FIELDS.index(k) for k in names]
    lo = np.array([RANGES[k][0] for k in names])
    hi = np.array([RANGES[k][1] for k in names])
    genes = ga.random(TUNE["seed"], 0, ga.INIT_GENERATION, 0, P * len(names)).reshape(P, len(names))
    avg = np.full(K, TICKS * DT / 2)
    for g in range(G):
        w = np.tile(np.array(mpc.RUNTIME_DEFAULTS), (P, 1))
        w[:, cols] = lo + genes * (hi - lo)
        t, _, _ = mpc.segment_times(dtrack, w, bounds, TICKS, v0=V0, N=N, **SOLVER)
        print("generation", g, "times", t.tolist())
        assert np.isfinite(t).any()
        assert np.array_equal(res.times[g, 0], t), (g, res.times[g, 0], t)
        br = ga.breed(genes, t, avg, pairs=1, lo=0.0, hi=1.0, seed=TUNE["seed"], generation=g)
        assert res.best_reward[g, 0] == br.best_r and res.best_index[g, 0] == br.best_idx
        assert np.array_equal(res.best_genes[g, 0], br.best_genes)
        genes, avg, r = br.genes, br.avg, br.r
    assert np.array_equal(res.population[0], genes) and np.array_equal(res.avg[0], avg)
    assert np.array_equal(res.rewards[0], r)
    w = np.tile(np.array(mpc.RUNTIME_DEFAULTS), (P, 1))
    w[:, cols] = lo + genes * (hi - lo)
    assert np.array_equal(res.weights[0], w)
    assert ((genes >= 0) & (genes <= 1)).all()
    again = mpc.tune_weights(dtrack, bounds, G, RANGES, **TUNE)
    for k in ("population", "weights", "best_reward", "best_index", "best_genes", "avg", "rewards", "ticks_done",
              "times"):
        assert np.array_equal(getattr(res, k), getattr(again, k)), k


def test_inputs_kernel_has_the_bits_of_the_torch_glue():
    """``mr_mpcseg_inputs`` on gfx950 against the expressions of ``ClosedLoop._tick`` evaluated by torch on the
    device (yaw rate, fed-back throttle, the speed rule of the horizon, the shifted controls): bit for bit.  torch
    evaluates ``tensor / host scalar`` as a product with the reciprocal and ``scalar / tensor`` as
    ``reciprocal(tensor) * scalar``; the kernel states the same operations."""
    import ctypes
    import torch
    from mpcracing import abi
    lib = abi.load_product()
    n, Nh, dt, Ts, lookahead, hz_min = 130, 15, 0.05, 0.05, 20.0, 5
    g = torch.Generator(device="cuda").manual_seed(11)
    f = dict(dtype=torch.float64, device="cuda")
    rnd = lambda *s: torch.rand(*s, generator=g, **f)  # noqa: E731
    state = torch.stack([rnd(n) * 100, rnd(n) * 100, (rnd(n) - 0.5) * 6.28, rnd(n) * 45, rnd(n) - 0.5,
                         rnd(n) - 0.5]).contiguous()
    state[3, ::9] = 1e-5  # below the floor of the speed rule
    mem = torch.zeros((abi.MR_MPCSEG_NMEM, n), **f)
    mem[0] = state[2] + (rnd(n) - 0.5) * 0.2
    mem[0, ::5] -= 6.2  # differences beyond +-3: the wrap
    mem[0, 1::5] += 6.2
    mem[2], mem[3], mem[4] = rnd(n), rnd(n) - 0.5, torch.where(rnd(n) < 0.5, rnd(n), torch.zeros(n, **f))
    U_prev = rnd(2, Nh, n)
    hz_prev = torch.randint(1, Nh + 1, (n,), generator=g, device="cuda").to(torch.int32)
    progress = torch.full((n,), 121.0, **f)
    s_start, s_end = torch.tensor([120.0], **f), torch.tensor([300.0], **f)
    state0, u_init = torch.empty((8, n), **f), torch.empty((2, Nh, n), **f)
    hz, done = torch.empty(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    times, ticks_done = torch.full((n,), np.inf, **f), torch.zeros(n, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = lib.mr_mpcseg_inputs(n, 1, Nh, 3, dt, 5451.0, p(state), p(progress), p(mem), p(s_start), p(s_end), p(U_prev),
                              p(hz_prev), None, lookahead, Ts, hz_min, p(state0), p(u_init), p(hz), p(done), p(times),
                              p(ticks_done), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.mr_last_error()
    # closed_loop.py _tick, lines 183-185, 194-195, 197-198, 211-212
    yaw, old_yaw, vx = state[2], mem[0], state[3]
    d = yaw - old_yaw
    d = torch.where(d > 3, yaw - (old_yaw + np.pi * 2), torch.where(d < -3, yaw - (old_yaw - np.pi * 2), d))
    yawdot = d / dt
    want_hz = torch.clamp(torch.ceil(lookahead / (Ts * torch.clamp(vx, min=1e-3))), hz_min, Nh).to(torch.int32)
    thr0 = torch.where(mem[4] == 0, mem[2], -mem[4])
    want0 = torch.stack([state[0], state[1], yaw, vx, state[4], yawdot, thr0, mem[3]])
    k1 = torch.arange(1, Nh + 1, device="cuda").reshape(Nh, 1)
    idx = torch.minimum(k1, (hz_prev.to(torch.int64) - 1).reshape(1, n))
    want_u = torch.gather(U_prev, 1, idx.expand(2, Nh, n))
    torch.cuda.synchronize()
    assert (d.abs() < 0.5).all() and (d.abs() > 0.08).any()  # the wrapped differences are small again
    assert torch.equal(state0, want0) and torch.equal(hz, want_hz) and torch.equal(u_init, want_u)
    assert int(done.sum()) == 0 and len(torch.unique(hz)) > 3
