"""The plant with run-time parameters, its rollouts and the identification on gfx950 (mr_plant_step_params,
mr_plant_rollout), and ``ClosedLoop(plant_params=...)``.

The checks of test_plant_rollout.py run again through plantroll_cases with the device library; the bitwise
reference of the default vector is mr_plant_step (the kernel with compile-time constants).  The closed loop
with the default vector is bitwise tests/golden/closed_loop_blend_golden.npz; with other parameters each tick's
state is ``plant_step`` of the previous state and the applied command.  All cases run at the fixture's sizes
(T = 330, at most 327 starts, H <= 40, at most 81 parameter sets).
"""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import plantroll_cases as pc
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


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _legacy_step(model, state, cmd, dt):
    """mr_plant_step: the kernel whose constants are compile-time"""
    from mpcracing import abi
    lib = abi.load_product()
    S, C = _dev(state), _dev(cmd)
    out = torch.empty_like(S)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.mr_plant_step(int(model), S.shape[1], _P(S), _P(C), float(dt), _P(out), st) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_device_default_parameters_and_overrides():
    pc.check_defaults(KW)


@pytest.mark.parametrize("pattern", pc.PATTERNS)
def test_device_predictions_match_mpmath(pattern):
    pc.check_golden(pattern, KW)


@pytest.mark.parametrize("pattern", pc.PATTERNS)
def test_device_statistics_match_numpy(pattern):
    pc.check_statistics(pattern, KW)


def test_device_g7_through_the_dt_override():
    pc.check_g7(KW)


def test_device_default_vector_is_the_compile_time_plant_bitwise():
    pc.check_default_step_bitwise(KW, _legacy_step)


def test_device_plant_step_is_first_rollout_step_bitwise():
    pc.check_step_equals_rollout(KW)


def test_device_launch_shape_independence_bitwise():
    pc.check_launch_shape(KW)


def test_device_throttle_zero_and_half_match_oracle():
    pc.check_branches(KW)


def test_device_yaw_error_is_wrapped():
    pc.check_yaw_wrap(KW)


def test_device_start_boundary_and_argument_errors():
    pc.check_edges(KW)


def test_device_nan_start_row_stops_its_lane_only():
    pc.check_nan_row(KW)


def test_device_nan_parameter_set_leaves_neighbours_unchanged():
    pc.check_nan_set(KW)


def test_device_identify():
    pc.check_identify(KW)


def test_device_position_cost_is_the_squared_norm():
    pc.check_position_cost(KW)


def test_device_plant_step_in_place_and_host_pointer():
    from mpcracing import abi
    lib = abi.load_product()
    starts = pc.G["c70/starts"]
    state, cmd = pc.LOG[:6, starts], pc.LOG[6:8, starts]
    ref = ro.plant_step(state, cmd, 0.05, "blend", pc.PARAMS[1])
    S, C, Q = _dev(state), _dev(cmd), _dev(pc.PARAMS[1][None])
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.mr_plant_step_params(2, len(starts), _P(S), _P(C), 0.05, 1, _P(Q), _P(S), st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(S.cpu().numpy(), ref)  # out aliases state
    h = np.zeros((6, 4))
    hp = h.ctypes.data_as(ctypes.c_void_p)
    assert lib.mr_plant_step_params(2, 4, hp, hp, 0.05, 1, _P(Q), hp, None) == -1
    assert b"not a HIP device pointer" in lib.mr_last_error()
    hl = np.ascontiguousarray(pc.LOG)
    one = np.zeros(1, np.int32)
    stats, count = torch.empty((1, 3, 6, 4), dtype=torch.float64, device="cuda"), torch.empty((1, 3), dtype=torch.int32,
                                                                                             device="cuda")
    assert lib.mr_plant_rollout(2, pc.T, hl.ctypes.data_as(ctypes.c_void_p), 1, one.ctypes.data_as(ctypes.c_void_p), 3,
                                1, _P(Q), None, _P(stats), _P(count), None, None) == -1
    assert b"not a HIP device pointer" in lib.mr_last_error()


def test_closed_loop_default_plant_params_bitwise_unchanged():
    from mpcracing.closed_loop import ClosedLoop
    m = _blend_setup()
    golden = np.load(os.path.join(HERE, "golden", "closed_loop_blend_golden.npz"))
    loop = m.make_loop(ClosedLoop, "blend", plant_params=ro.plant_params())
    recs = loop.run(m.TICKS)
    torch.cuda.synchronize()
    out = {"state": loop.state.cpu().numpy()}
    for t, r in enumerate(recs):
        for k in m.KEYS:
            if r[k] is not None:
                out[f"tick{t}/{k}"] = r[k].cpu().numpy()
    assert sorted(out) == sorted(golden.files)
    for k in golden.files:
        g = golden[k]
        assert out[k].dtype == g.dtype and out[k].shape == g.shape, k
        assert np.array_equal(np.ascontiguousarray(out[k]).view(np.uint8), np.ascontiguousarray(g).view(np.uint8)), k


@pytest.mark.parametrize("per_vehicle", [False, True])
def test_closed_loop_steps_with_plant_params(per_vehicle):
    from mpcracing.closed_loop import ClosedLoop
    m = _blend_setup()
    B = len(m.S0)
    if per_vehicle:
        q = np.stack([ro.plant_params(Cf=60000.0 + 10000.0 * j, m=1700.0 + 50.0 * j) for j in range(B)])
    else:
        q = ro.plant_params(Cf=80000.0)
    loop = m.make_loop(ClosedLoop, "blend", plant_params=q)
    moved = False
    for tick in range(m.TICKS):
        prev = loop.state.cpu().numpy()
        r = loop.tick()
        torch.cuda.synchronize()
        cmd = np.stack([(r["cmd_throttle"] - r["cmd_brake"]).cpu().numpy(), r["cmd_steer"].cpu().numpy()])
        ref = ro.plant_step(prev, cmd, loop.dt, "blend", q)
        got = loop.state.cpu().numpy()
        assert np.isfinite(got).all() and pc._same([got], [ref]), tick
        moved = moved or not pc._same([got], [ro.plant_step(prev, cmd, loop.dt, "blend")])
    assert moved  # the parameters reached the plant
    with pytest.raises(ValueError, match="plant_params goes with"):
        ClosedLoop(loop.track, B=B, plant="learned", plant_params=q, plant_tyres=(np.array([65000.0, 65000.0]), None),
                   plant_kind="linear")
    with pytest.raises(ValueError, match="plant_params: "):
        ClosedLoop(loop.track, B=B, plant="blend", plant_params=np.zeros((B + 1, 22)))
