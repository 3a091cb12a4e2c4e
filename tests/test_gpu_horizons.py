"""One horizon per instance in one batched solve on the gfx950 build: BatchSolver.solve(batch with "horizon") and
ClosedLoop(horizon=).

tests/test_horizons.py holds the host builds to the same checks.  The device build is repeatable
(test_repeated_solves_are_bitwise_identical), so instance i of a mixed batch under the layout horizon 63 is compared
bit for bit with the solve of that instance by a BatchSolver(N_i), and the whole-solve columns with the IPOPT oracle
log.  The closed loop with fixed horizons is compared bit for bit with B = 1 loops at N = N_i; with the speed rule
its recorded horizons are the numpy formula of its recorded speeds and a tick is re-solved by uniform handles.
Every solve here is B <= 14.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import horizon_cases as hc  # noqa: E402
from mpcracing.batch import BatchSolver  # noqa: E402

G = hc.G
FAMILY_PREC = [("kin", "fp64"), ("dyn_lane", "fp64"), ("blend_par", "fp64"), ("blend_par", "fp32")]
_handles = {}
_cache = {}


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _handle(cases, N, precision="fp64", options="prefix", order=0):
    model, lane, Ts, over, tyres = hc.family_config(cases)
    key = (N, model, precision, lane, Ts, options, tuple(sorted(over.items())), order)
    if key not in _handles:
        _handles[key] = BatchSolver(N, model, precision, lane, Ts, max_batch=14, tyres=tyres, dispatch_order=order,
                                    **G.OPTIONS[options], **over)
    return _handles[key]


def _duals(cases):
    return not G.CASES[cases[0]]["lane"]


def _mixed(cases, precision="fp64", options="prefix", u_init=None, tag="", order=0):
    key = ("mixed", tuple(cases), precision, options, tag, order)
    if key not in _cache:
        batch = hc.mixed_inputs(cases, u_init)
        _cache[key] = (batch, _np(_handle(cases, hc.NL, precision, options, order).solve(
            dict(batch, horizon=hc.horizons(cases)), duals=_duals(cases))))
    return _cache[key]


def _uniform(cases, i, batch, precision="fp64", options="prefix", tag=""):
    """Instance i alone through a BatchSolver(N_i) without a horizon: the existing entry point."""
    key = ("one", cases[i], precision, options, tag)
    if key not in _cache:
        N = G.CASES[cases[i]]["N"]
        _cache[key] = _np(_handle(cases, N, precision, options).solve(hc.one_instance(batch, i, N),
                                                                     duals=_duals(cases)))
    return _cache[key]


@pytest.mark.parametrize("family,precision", FAMILY_PREC, ids=[f"{f}-{p}" for f, p in FAMILY_PREC])
def test_gpu_mixed_batch_equals_uniform_solves(family, precision):
    cases = hc.FAMILIES[family]
    batch, o = _mixed(cases, precision)
    for i, case in enumerate(cases):
        N = G.CASES[case]["N"]
        one = _uniform(cases, i, batch, precision)
        assert one["iters"][0] > 0
        hc.assert_column_is_uniform_solve(hc.column(o, i), one, N, f"gfx950 {family} {precision} [{i}] N={N}")


def test_gpu_u_init_is_read_with_the_layout_stride():
    cases = hc.FAMILIES["kin"]
    Ns = hc.horizons(cases)
    batch, o = _mixed(cases, u_init=hc.nan_padded_u_init(Ns), tag="u_init")
    for i in range(len(cases)):
        one = _uniform(cases, i, batch, tag="u_init")
        assert np.isfinite(one["X"]).all() and np.isfinite(one["U"]).all()
        hc.assert_column_is_uniform_solve(hc.column(o, i), one, int(Ns[i]), f"gfx950 kin u_init [{i}] N={Ns[i]}")


def test_gpu_instance_order_does_not_matter():
    cases = hc.FAMILIES["kin"]
    batch, o = _mixed(cases)
    perm = np.random.default_rng(5).permutation(len(cases))
    p = _np(_handle(cases, hc.NL).solve(dict(hc.permuted(batch, perm), horizon=hc.horizons(cases)[perm]),
                                        duals=True))
    for k, v in o.items():
        assert hc.bit_equal(p[k], v[..., perm]), k


@pytest.mark.parametrize("order", [1, 2])
def test_gpu_dispatch_order_does_not_matter(order):
    """The kin batch of 14 under dispatch_order 1 and 2 against order 0.  Order 2 takes the instances by decreasing
    order_hint: the hint 0, 1, .. 13 starts instance 13 first and instance 0 last, the reverse of order 0."""
    cases = hc.FAMILIES["kin"]
    batch, o = _mixed(cases)
    b = dict(batch, horizon=hc.horizons(cases))
    if order == 2:
        b["order_hint"] = np.arange(len(cases), dtype=np.int32)
    p = _np(_handle(cases, hc.NL, order=order).solve(b, duals=True))
    for k, v in o.items():
        assert hc.bit_equal(p[k], v), (order, k)


@pytest.mark.parametrize("name", sorted(hc.WHOLE_BATCHES))
def test_gpu_mixed_batch_against_oracle(name):
    cases = hc.WHOLE_BATCHES[name]
    _batch, o = _mixed(cases, options="whole")
    checked = 0
    for i, case in enumerate(cases):
        if G.CASES[case]["kind"] == "whole":
            hc.check_against_oracle(case, hc.column(o, i), f"gfx950 mixed[{i}]", device=True)
            checked += 1
    assert checked == {"kin": 2, "blend_par": 1}[name]


def test_gpu_out_of_range_horizons_are_not_solved():
    """Horizons [0, 17, 64, -3] under N = 63 (tests/test_horizons.py): sentinel-filled buffers with a guard band."""
    cases = ["kin_N17"] * 4
    hz = np.array([0, 17, 64, -3], np.int32)
    batch = hc.mixed_inputs(cases)
    s = _handle(cases, hc.NL)
    B, guard = 4, 256
    shapes = {k: tuple(v.shape) for k, v in s.alloc_outputs(B, duals=True).items()}
    flat, out = {}, {}
    for k, shp in shapes.items():
        n = int(np.prod(shp))
        if k in ("status", "iters"):
            flat[k] = torch.full((n + guard,), -1, dtype=torch.int32, device=s.device)
        else:
            flat[k] = torch.full((n + guard,), hc.SENTINEL, dtype=torch.float64, device=s.device)
        out[k] = flat[k][:n].view(shp)
    s.launch(s.to_device(dict(batch, horizon=hz)), out)
    torch.cuda.synchronize()
    o = _np(out)
    for i in (0, 2, 3):
        hc.assert_not_solved(hc.column(o, i), f"instance {i}")
    hc.assert_column_is_uniform_solve(hc.column(o, 1), _uniform(cases, 1, batch), 17, "instance 1")
    want = {"X": 6 * 18, "U": 2 * 17, "S": 18, "eC": 17, "eL": 17, "obj": 1, "kkt": 1, "constr_viol": 1,
            "lam_g": 13 * 17 + 9}
    for k, n in want.items():
        assert int(np.isfinite(o[k]).sum()) == n == int(np.isfinite(o[k][..., 1]).sum()), k
        assert not (o[k] == hc.SENTINEL).any(), k
    for k, shp in shapes.items():
        tail = flat[k][int(np.prod(shp)):].cpu().numpy()
        assert (tail == (-1 if k in ("status", "iters") else hc.SENTINEL)).all(), k


def test_gpu_horizon_argument_is_checked():
    cases = ["kin_N17"] * 2
    s = _handle(cases, hc.NL)
    dev_in = s.to_device(dict(hc.mixed_inputs(cases), horizon=np.array([17, 17], np.int32)))
    out = s.alloc_outputs(2)
    for bad in (dev_in["horizon"][:1], dev_in["horizon"].to(torch.int64), dev_in["horizon"].cpu()):
        with pytest.raises(ValueError, match="horizon"):
            s.launch(dict(dev_in, horizon=bad), out)


# ---------------------------------------------------------------------------------------------- closed loop
TRACK, TICKS = "t4", 4
SPEEDS = np.array([6.0, 12.0, 25.0, 40.0])
S0 = np.array([20.0, 300.0, 600.0, 900.0])
REC_ROWS = {"predicted_states": (1, 1), "controls": (1, 0), "s_hat": (0, 1), "e_hat_c": (0, 0), "e_hat_l": (0, 0)}


@pytest.fixture(scope="module")
def dtrack():
    from mpcracing.geometry import DeviceTrack
    return DeviceTrack(TRACK)


def _starts(dtrack):
    from mpcracing.closed_loop import ClosedLoop
    x0 = ClosedLoop.start_states(dtrack, S0, v0=10.0)
    x0[3] = SPEEDS
    return x0


def _host_rec(rec):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in rec.items()}


def test_gpu_closed_loop_fixed_horizons_equal_single_loops(dtrack):
    """B = 4 with horizon = [5, 9, 15, 15] under N = 15: vehicle i's records are, bit for bit, those of a
    ClosedLoop(B = 1, N = N_i) driving that vehicle alone; predictions beyond N_i are NaN."""
    from mpcracing.closed_loop import ClosedLoop
    hz = np.array([5, 9, 15, 15], np.int32)
    x0 = _starts(dtrack)
    loop = ClosedLoop(dtrack, B=4, N=15, start_control_at=1, mpc_model="dyn", precision="fp64", horizon=hz)
    loop.reset(x0)
    recs = [_host_rec(r) for r in loop.run(TICKS)]
    for i, N in enumerate(hz):
        one = ClosedLoop(dtrack, B=1, N=int(N), start_control_at=1, mpc_model="dyn", precision="fp64")
        one.reset(x0[:, i:i + 1])
        ref = [_host_rec(r) for r in one.run(TICKS)]
        for t, (a, b) in enumerate(zip(recs, ref)):
            assert a["controlled"] == b["controlled"] == (t >= 1)
            assert np.array_equal(a["horizon"], hz) and b["horizon"] is None
            for k, v in b.items():
                if k in ("step", "controlled", "horizon"):
                    continue
                if v is None:  # (an uncontrolled tick has no solve)
                    assert a[k] is None, (t, k)
                    continue
                mine = a[k][..., i]
                if k in REC_ROWS:
                    ax, extra = REC_ROWS[k]
                    n = int(N) + extra
                    assert np.isnan(np.take(mine, np.arange(n, mine.shape[ax]), axis=ax)).all(), (i, t, k)
                    mine = np.take(mine, np.arange(n), axis=ax)
                assert hc.bit_equal(mine, v[..., 0]), (i, t, k)
        assert all(r["iters"][0] > 0 for r in ref[1:])


def test_gpu_closed_loop_speed_rule(dtrack):
    """horizon = "speed" under N = 40: each tick's horizons are the numpy formula of that tick's recorded speeds,
    at least three distinct values occur, and tick 2's solve of every vehicle is, in status (and bit for bit in its
    outputs), the solve of that tick's inputs by a BatchSolver(N_i)."""
    from mpcracing.closed_loop import ClosedLoop
    N, la, hmin, Ts = 40, 20.0, 5, 0.05
    loop = ClosedLoop(dtrack, B=4, N=N, start_control_at=1, mpc_model="dyn", precision="fp64", horizon="speed")
    assert (loop.horizon_lookahead, loop.horizon_min) == (la, hmin)
    loop.reset(_starts(dtrack))
    recs, inputs2 = [], None
    for t in range(TICKS):
        recs.append(_host_rec(loop.tick()))
        if t == 2:  # the sensing outputs of tick 2, before the next tick overwrites them
            torch.cuda.synchronize()
            inputs2 = {k: getattr(loop, k).cpu().numpy().copy() for k in ("progress", "cx", "cy", "max_error")}
    seen = set()
    for t, r in enumerate(recs):
        want = np.clip(np.ceil(la / (Ts * np.maximum(r["vx"], 1e-3))), hmin, N).astype(np.int32)
        assert r["horizon"].dtype == np.int32 and np.array_equal(r["horizon"], want), (t, r["horizon"], want)
        seen |= set(want.tolist())
    assert len(seen) >= 3, seen
    # tick 2 again, vehicle by vehicle, by uniform handles
    r1, r2 = recs[1], recs[2]
    thr0 = np.where(r1["cmd_brake"] == 0, r1["cmd_throttle"], -r1["cmd_brake"])
    state0 = np.stack([r2[k] for k in ("X", "Y", "yaw", "vx", "vy", "yawdot")] + [thr0, r1["cmd_steer"]])
    for i in range(4):
        Ni, Np = int(r2["horizon"][i]), int(r1["horizon"][i])
        u_init = np.stack([r1["controls"][:, min(k + 1, Np - 1), i] for k in range(Ni)], axis=1)[:, :, None]
        assert np.isfinite(u_init).all()
        b = dict(state0=state0[:, i:i + 1], s0=inputs2["progress"][i:i + 1], cx=inputs2["cx"][:, i:i + 1],
                 cy=inputs2["cy"][:, i:i + 1], max_error=inputs2["max_error"][i:i + 1],
                 runtime=loop.runtime.cpu().numpy()[:, i:i + 1], u_init=u_init)
        one = _np(BatchSolver(Ni, "dyn", "fp64", False, Ts, max_batch=1).solve(b))
        assert int(r2["status"][i]) == int(one["status"][0]), (i, r2["status"][i], one["status"][0])
        assert int(r2["iters"][i]) == int(one["iters"][0])
        assert hc.bit_equal(r2["controls"][:, :Ni, i], one["U"][:, :, 0]), i
        assert np.isnan(r2["controls"][:, Ni:, i]).all()
