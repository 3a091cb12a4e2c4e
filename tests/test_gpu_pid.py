"""The PID agent on gfx950 (mr_pid_control, mr_pid_drive) through pid_cases, at n = 70 (one full wavefront and a
6-lane one), T = 40, gains and plant parameters per vehicle.

* one tick on the fixture's ticks against the host twin: progress and error bit for bit (the sensing is built
  without FP contraction on both sides), the other outputs within 1e-12; and against the fixture itself;
* the fused drive = T launches of mr_pid_control + mr_plant_step_params, bit for bit, every row, model, state,
  mem and ticks_done, also with G = P = 1;
* the device drive against the host twin's: every row within 1e-6, ticks_done equal;
* bitwise on the device: 25 + 15 = 40, vehicles 0, 63, 64, 69 alone = in the batch, two launches equal,
  shared = copies, row subsets;
* a NaN-gain vehicle in lane 5 leaves the other 69 unchanged;
* the drive's log rolled out again by plant_rollout_errors on the GPU: errors exactly 0.
"""
import numpy as np
import pytest

import pid_cases as pc
from mpcracing import pid

pytestmark = pytest.mark.gpu

KW = {}
HOST = dict(host_twin=True)


@pytest.mark.parametrize("drive", pc.DRIVES)
def test_device_one_tick_matches_host_twin_and_reference(drive):
    dev, dmem = pc.lib_ticks(drive, KW)
    host, hmem = pc.lib_ticks(drive, HOST)
    got, ref = dict(zip(pid.OUT_ROWS, dev)), dict(zip(pid.OUT_ROWS, host))
    assert pc.same(got["progress"], ref["progress"]) and pc.same(got["error"], ref["error"])
    bad = [k for k in pid.OUT_ROWS if not pc.close(got[k], ref[k], 1e-12)]
    assert not bad, bad
    assert pc.same(dmem[0], hmem[0]) and pc.same(dmem[1], hmem[1]) and pc.same(dmem[3], hmem[3])
    assert pc.close(dmem[2], hmem[2], 1e-12)
    pc.check_teacher_forced(drive, KW)


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("model", pc.MODELS)
def test_device_fused_drive_is_iterated_launches_bitwise(model, shared):
    pc.check_fused_equals_stepwise(model, shared, KW)


@pytest.mark.parametrize("model", pc.MODELS)
def test_device_drive_matches_host_twin(model):
    pc.check_against_host(model, KW)


def test_device_continuation_is_bitwise():
    pc.check_continuation(KW)


def test_device_vehicle_alone_equals_vehicle_in_batch():
    pc.check_alone_equals_batch(KW)


def test_device_two_launches_are_equal():
    pc.check_repeatable(KW)


def test_device_shared_gains_and_parameters_equal_copies():
    pc.check_shared_equals_copies(KW)


def test_device_row_subsets_equal_rows_of_the_full_log():
    pc.check_mask_subsets(KW)


def test_device_nan_gain_stops_its_vehicle_only():
    pc.check_nan_gain_stops_one_vehicle(KW, lane=5)


def test_device_drive_log_rolls_out_exactly():
    pc.check_exact_rollouts(KW)


def test_device_edges_and_fitness():
    pc.check_steer_saturates(KW)
    pc.check_command_ranges(KW)
    pc.check_straight_track(KW)
    pc.check_evaluate_gains(KW)
