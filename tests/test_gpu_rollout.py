"""Open-loop rollouts and the model step on gfx950 (mr_tyre_rollout, mr_vehicle_step), and the learned plant of
the closed loop, against tests/golden/rollout_golden.* and the host build of the same source.

The checks of test_rollout.py run again through rollout_cases with the device library.  Device against host
build: the golden tolerance (100 x the reference's own error against mpmath, floor 1e-13, of the component's
scale) -- not bitwise, the two libm differ.  Launch-shape independence, repeatability and step-against-rollout
are bitwise.  ``ClosedLoop(plant="learned")``: after every tick the state is the host build's mrh_vehicle_step
of the previous state and the applied command; ``plant="blend"`` stays bitwise what it was before the learned
plant existed (tests/golden/closed_loop_blend_golden.npz, recorded with that commit's library).
All cases run at the fixture's sizes (T = 330, at most 140 starts, H <= 40).
"""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import rollout_cases as rc
from mpcracing import rollout as ro

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KW = {}


def _blend_setup():
    spec = importlib.util.spec_from_file_location("make_blend_loop_golden",
                                                  os.path.join(HERE, "golden", "make_blend_loop_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _eval_dynamics(model, tyres, x, u, Ts, **cfg):
    from mpcracing.batch import BatchSolver
    s = BatchSolver(15, model, "fp64", Ts=Ts, max_batch=1, tyres=tyres, **cfg)
    X, U = torch.from_numpy(x).cuda().contiguous(), torch.from_numpy(u).cuda().contiguous()
    f = torch.zeros((len(x), 6), dtype=torch.float64, device="cuda")
    rc_ = s.lib.mr_eval_dynamics(s.h, len(x), ctypes.c_void_p(X.data_ptr()), ctypes.c_void_p(U.data_ptr()), None,
                                 ctypes.c_void_p(f.data_ptr()), None, None,
                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc_ == 0
    torch.cuda.synchronize()
    return f.cpu().numpy()


@pytest.mark.parametrize("pattern", rc.PATTERNS)
def test_device_predictions_match_mpmath_and_host(pattern):
    rc.check_golden(pattern, KW)
    for i, (d, h) in enumerate(zip(rc.golden_runs(pattern, KW), rc.golden_runs(pattern, dict(host_twin=True)))):
        t = rc.tol(pattern, i)
        err = np.abs(d.pred[0] - h.pred[0]).max(axis=2) / rc.SCALE
        print(f"{pattern} {rc.META['sets'][i]}: device vs host predictions, max scaled error {err.max():.2e}")
        assert (err <= t).all(), (pattern, i, err)
        assert np.array_equal(d.count, h.count)
        for k in ("mean", "std", "rmse", "min", "max"):
            a, b = getattr(d, k)[0], getattr(h, k)[0]
            if np.isnan(b).all():
                assert np.isnan(a).all()
                continue
            es = np.abs(a - b) / rc.SCALE
            assert (es <= t).all(), (pattern, i, k, es)


@pytest.mark.parametrize("pattern", rc.PATTERNS)
def test_device_statistics_match_numpy(pattern):
    rc.check_statistics(pattern, KW)


def test_device_one_step_error_is_the_fit_loss():
    rc.check_loss_crosscheck(KW)


def test_device_launch_shape_independence_bitwise():
    rc.check_launch_shape(KW)


def test_device_start_boundary():
    rc.check_start_boundary(KW)


def test_device_nonfinite_step_stops_its_rollout_only():
    rc.check_nonfinite_ts(KW)


def test_device_nan_parameter_set_leaves_neighbours_unchanged():
    rc.check_nan_set(KW)


def test_device_vehicle_step_is_first_rollout_step_bitwise():
    rc.check_step_equals_rollout(KW)


def test_device_vehicle_step_matches_solver_dynamics():
    rc.check_step_vs_dynamics(KW, _eval_dynamics)


def test_device_rank_by_rollout():
    rc.check_rank(KW)


def test_device_vehicle_step_in_place_and_host_pointer():
    from mpcracing import abi, tyrefit
    lib = abi.load_product()
    cfg = tyrefit.make_config("pacejka")
    starts = rc.G["c70/starts"]
    state, cmd = rc.LOG[:6, starts], rc.LOG[6:8, starts]
    ref = ro.vehicle_step(state, cmd, 0.05, rc.SETS[2], "pacejka")
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    S, C, Pm, Fz = d(state), d(cmd), d(rc.SETS[2][0][None]), d(rc.SETS[2][1][None])
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.mr_vehicle_step(ctypes.byref(cfg), len(starts), P(S), P(C), 0.05, 1, P(Pm), P(Fz), P(S), st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(S.cpu().numpy(), ref)  # out aliases state
    h = np.zeros((6, 4))
    hp = h.ctypes.data_as(ctypes.c_void_p)
    assert lib.mr_vehicle_step(ctypes.byref(cfg), 4, hp, hp, 0.05, 1, P(Pm), P(Fz), hp, None) == -1
    assert b"not a HIP device pointer" in lib.mr_last_error()


def test_closed_loop_learned_plant_steps_with_the_model():
    from mpcracing.closed_loop import ClosedLoop
    m = _blend_setup()
    p, Fz = rc.SETS[2]
    tyres = ((p[:9].copy(), float(Fz[0])), (p[9:].copy(), float(Fz[1])))
    # the MPC carries the same learned tyres as its plant
    loop = m.make_loop(ClosedLoop, "learned", plant_tyres=(p, Fz), plant_kind="pacejka", mpc_model="dyn_pacejka",
                       tyres=tyres)
    t = rc.tol("h1", 2)[0]  # one step of this parameter set
    for tick in range(m.TICKS):
        prev = loop.state.cpu().numpy()
        r = loop.tick()
        torch.cuda.synchronize()
        cmd = np.stack([(r["cmd_throttle"] - r["cmd_brake"]).cpu().numpy(), r["cmd_steer"].cpu().numpy()])
        ref = ro.vehicle_step(prev, cmd, loop.dt, (p, Fz), "pacejka", host_twin=True)
        got = loop.state.cpu().numpy()
        # scale: the component's largest value in the fixture's log or in this state, whichever is larger
        err = np.abs(got - ref).max(axis=1) / np.maximum(np.abs(ref).max(axis=1), rc.SCALE)
        print(f"tick {tick}: controlled {r['controlled']}, status {r['status'].tolist() if r['controlled'] else None}, "
              f"state vs host model step, scaled error {err}")
        assert np.isfinite(got).all() and (err <= t).all(), (tick, err, t)
    with pytest.raises(ValueError, match="plant_tyres"):
        ClosedLoop(loop.track, B=4, plant="learned")
    with pytest.raises(ValueError, match="plant_tyres"):
        ClosedLoop(loop.track, B=4, plant="blend", plant_tyres=(p, Fz))


def test_closed_loop_blend_plant_bitwise_unchanged():
    from mpcracing.closed_loop import PLANT, ClosedLoop
    assert PLANT == {"kin": 0, "dyn": 1, "blend": 2}
    m = _blend_setup()
    golden = np.load(os.path.join(HERE, "golden", "closed_loop_blend_golden.npz"))
    out = m.run_blend(ClosedLoop)
    assert sorted(out) == sorted(golden.files)
    for k in golden.files:
        g = golden[k]
        assert out[k].dtype == g.dtype and out[k].shape == g.shape, k
        assert np.array_equal(np.ascontiguousarray(out[k]).view(np.uint8), np.ascontiguousarray(g).view(np.uint8)), k
