"""The GA on gfx950 (mr_pid_segment_times, mr_ga_breed, pid.tune_gains) through evolve_cases, at 72 vehicles (one
full wavefront and an 8-lane one):

* the fused segment timing = pid.evaluate_gains on the device, bit for bit, every plant, parameters shared and per
  vehicle; ticks_done = crossing tick + 1; the same with a cap of 4096 ticks;
* unfinished and zero-length segments, a NaN gain vector, two launches, a gain vector alone;
* the device's times against the host build's within 1e-6, ticks_done equal;
* the breeding against tests/ga_ref.py and, on identical times, against the host build: same decisions, same genes;
* tune_gains = its generations as separate calls with synchronises in between, bit for bit;
* the argument errors of the product library.
"""
import pytest

import evolve_cases as ec
import pid_cases as pc

pytestmark = pytest.mark.gpu

KW = {}


@pytest.mark.parametrize("shared", [False, True], ids=["per_vehicle", "shared"])
@pytest.mark.parametrize("model", pc.MODELS)
def test_device_fused_timing_is_evaluate_gains_bitwise(model, shared):
    ec.check_fused_equals_evaluate_gains(model, shared, KW)


def test_device_unfinished_and_zero_length_segments():
    ec.check_unfinished_and_zero_length(KW)


def test_device_nan_gains_stop_their_vehicles_only():
    ec.check_nan_gains_stop_their_vehicles_only(KW)


def test_device_two_launches_equal_and_a_gain_vector_alone():
    ec.check_repeatable_and_alone(KW)


@pytest.mark.parametrize("model", pc.MODELS)
def test_device_timing_matches_host_twin(model):
    ec.check_timing_against_host(model, KW)


@pytest.mark.parametrize("shape", ec.SHAPES, ids=lambda s: "P%d_K%d_D%d_pairs%d" % s)
def test_device_breeding_matches_reference(shape):
    ec.check_breed(shape, KW)


def test_device_breeding_edges():
    ec.check_breed_edges(KW)


def test_device_breeding_decides_as_host_twin():
    ec.check_breed_against_host(KW)


def test_device_tune_gains_is_its_generations_one_by_one():
    ec.check_tune(KW)


def test_device_tune_gains_default_population_and_other_genes():
    ec.check_tune_default_population(KW)


def test_device_segment_time_argument_errors():
    ec.check_segment_errors(KW)


def test_device_breed_argument_errors():
    ec.check_breed_errors(KW)
