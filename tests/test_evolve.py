"""The GA on the host build (TEST-ONLY g++ build of csrc/mr_ga.h and csrc/mr_pid.h; no GPU) through
evolve_cases: the random stream of both libraries against numpy's Philox, the fused segment timing against
pid.evaluate_gains bit for bit, the breeding against tests/ga_ref.py, a whole tune_gains run against its generations
as separate calls, and the argument errors."""
import pytest

import evolve_cases as ec
import pid_cases as pc

KW = dict(host_twin=True)


@pytest.mark.parametrize("host_twin", [True, False], ids=["host_build", "product_library"])
def test_stream_is_numpy_philox(host_twin):
    ec.check_stream(host_twin)


@pytest.mark.parametrize("shared", [False, True], ids=["per_vehicle", "shared"])
@pytest.mark.parametrize("model", pc.MODELS)
def test_fused_timing_is_evaluate_gains_bitwise(model, shared):
    ec.check_fused_equals_evaluate_gains(model, shared, KW)


def test_unfinished_and_zero_length_segments():
    ec.check_unfinished_and_zero_length(KW)


def test_nan_gains_stop_their_vehicles_only():
    ec.check_nan_gains_stop_their_vehicles_only(KW)


def test_two_calls_equal_and_a_gain_vector_alone():
    ec.check_repeatable_and_alone(KW)


@pytest.mark.parametrize("shape", ec.SHAPES, ids=lambda s: "P%d_K%d_D%d_pairs%d" % s)
def test_breeding_matches_reference(shape):
    ec.check_breed(shape, KW)


def test_breeding_edges():
    ec.check_breed_edges(KW)


def test_tune_gains_is_its_generations_one_by_one():
    ec.check_tune(KW)


def test_tune_gains_default_population_and_other_genes():
    ec.check_tune_default_population(KW)


def test_segment_time_argument_errors():
    ec.check_segment_errors(KW)


def test_breed_argument_errors():
    ec.check_breed_errors(KW)
