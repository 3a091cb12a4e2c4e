"""The models/ plant with run-time parameters, its rollouts along a logged drive and the identification on top
(csrc/mr_plant.h, csrc/mr_plantroll.h, mpcracing/rollout.py, mpcracing/plantfit.py) on the host build of the
source, against tests/golden/plant_rollout_golden.* (the reference's numpy models iterated, and the same
rollouts in mpmath at 50 digits; generator make_plant_rollout_golden.py).

* predictions of three parameter sets x three models on three start patterns vs mpmath: scaled error at most
  100 x the numpy models' own (floor 1e-13), per step and component;
* count, mean, std (ddof 1), rmse, min, max (yaw error wrapped) vs numpy on the 50-digit predictions, same
  tolerance;
* the G7 fixture through the dt override (rtol 1e-11, atol 1e-9, as tests/test_plant.py);
* bitwise: the default vector vs the compile-time plant (mrh_plant_step), plant_step vs the rollout's first
  step, a set alone vs among three, per-vehicle parameters vs single calls;
* throttle exactly 0 and 0.5, and a log whose yaw crosses pi, against oracle.plant;
* edges: NaN rows and sets, start and argument checks;
* plantfit.identify on a synthetic log, RolloutErrors.position_cost.
"""
import numpy as np
import pytest

import plantroll_cases as pc
import track_twin

KW = dict(host_twin=True)


def test_default_parameters_and_overrides():
    pc.check_defaults(KW)


@pytest.mark.parametrize("pattern", pc.PATTERNS)
def test_predictions_match_mpmath(pattern):
    pc.check_golden(pattern, KW)


@pytest.mark.parametrize("pattern", pc.PATTERNS)
def test_statistics_match_numpy(pattern):
    pc.check_statistics(pattern, KW)


def test_g7_through_the_dt_override():
    pc.check_g7(KW)


def test_default_vector_is_the_compile_time_plant_bitwise():
    pc.check_default_step_bitwise(KW, track_twin.plant_step)


def test_plant_step_is_first_rollout_step_bitwise():
    pc.check_step_equals_rollout(KW)


def test_launch_shape_independence_bitwise():
    pc.check_launch_shape(KW)


def test_throttle_zero_and_half_match_oracle():
    pc.check_branches(KW)


def test_yaw_error_is_wrapped():
    pc.check_yaw_wrap(KW)


def test_start_boundary_and_argument_errors():
    pc.check_edges(KW)


def test_nan_start_row_stops_its_lane_only():
    pc.check_nan_row(KW)


def test_nan_parameter_set_leaves_neighbours_unchanged():
    pc.check_nan_set(KW)


def test_identify():
    pc.check_identify(KW)


def test_position_cost_is_the_squared_norm():
    pc.check_position_cost(KW)


def test_closed_loop_rejects_plant_params_for_the_learned_plant():
    """The argument check comes before anything touches the GPU."""
    from mpcracing import closed_loop, rollout

    class _Track(closed_loop.DeviceTrack):
        def __init__(self):  # no device
            self.lib, self.device = None, "cpu"

    with pytest.raises(ValueError, match="plant_params goes with"):
        closed_loop.ClosedLoop(_Track(), B=2, plant="learned", plant_params=rollout.plant_params())
    with pytest.raises(ValueError, match="plant_params: "):
        closed_loop.ClosedLoop(_Track(), B=2, plant="blend", plant_params=np.zeros((3, 22)))
