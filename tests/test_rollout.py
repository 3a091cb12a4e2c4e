"""Open-loop rollouts, their statistics and the model step (csrc/mr_rollout.h) on the host build of the source,
against tests/golden/rollout_golden.* (the reference's torch model iterated, and the same rollouts in mpmath at
50 digits; generator make_rollout_golden.py).

* predictions of three parameter sets (linear 65000, Pacejka defaults, the learned pacejka-1) on four start
  patterns vs mpmath: scaled error at most 100 x the torch model's own (floor 1e-13), per step and component.
  Measured maxima (host build): 7.0e-16 at H = 12, 2.8e-15 at H = 40, 1.8e-16 at H = 1 -- the floor decides
  everywhere, also for pacejka-1, where torch itself is 1.8e-6 off (its (1 - E) a + (E / B) atan(B a) cancels
  ten digits at E ~ 1e10);
* count, mean, std (ddof 1), rmse, min, max vs numpy on the 50-digit predictions, same tolerance;
* H = 1: the summed squared error is the fit's loss (mr_tyre_loss_grad) on the rows built from the log;
* bitwise: two identical calls, a set alone vs among three, mr_vehicle_step vs the rollout's first step;
* start rows outside [0, T - 1 - H] are an argument error; a non-finite step stops its rollout only;
* mr_vehicle_step vs the solver's generated dynamics (MR_MODEL_DYNAMIC with Cf = Cr = 65000,
  MR_MODEL_DYNAMIC_PACEJKA) at dt = Ts: 1e-12 of the component's scale;
* load_log on a re-wrapped yaw, FitResult.rank_by_rollout.
"""
import ctypes

import numpy as np
import pytest

import host_twin as ht
import rollout_cases as rc

KW = dict(host_twin=True)


def _eval_dynamics(model, tyres, x, u, Ts, **cfg):
    c = ht.config(15, model, Ts=Ts, **cfg)
    P = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    out = np.zeros((len(x), 6))
    for i in range(len(x)):
        f, J, H, nu = np.zeros(6), np.zeros(48), np.zeros(36), np.zeros(6)
        assert ht.lib().mrh_eval_dynamics(ctypes.byref(c), P(tyres[0][0]) if tyres else None,
                                          tyres[0][1] if tyres else 0.0, P(tyres[1][0]) if tyres else None,
                                          tyres[1][1] if tyres else 0.0, P(x[i]), P(u[i]), P(nu), P(f), P(J), P(H)) == 0
        out[i] = f
    return out


@pytest.mark.parametrize("pattern", rc.PATTERNS)
def test_predictions_match_mpmath(pattern):
    rc.check_golden(pattern, KW)


@pytest.mark.parametrize("pattern", rc.PATTERNS)
def test_statistics_match_numpy(pattern):
    rc.check_statistics(pattern, KW)


def test_one_step_error_is_the_fit_loss():
    rc.check_loss_crosscheck(KW)


def test_launch_shape_independence_bitwise():
    rc.check_launch_shape(KW)


def test_start_boundary():
    rc.check_start_boundary(KW)


def test_nonfinite_step_stops_its_rollout_only():
    rc.check_nonfinite_ts(KW)


def test_nan_parameter_set_leaves_neighbours_unchanged():
    rc.check_nan_set(KW)


def test_vehicle_step_is_first_rollout_step_bitwise():
    rc.check_step_equals_rollout(KW)


def test_vehicle_step_matches_solver_dynamics():
    rc.check_step_vs_dynamics(KW, _eval_dynamics)


def test_load_log_unwraps_yaw(tmp_path):
    rc.check_loader(tmp_path)


def test_rank_by_rollout():
    rc.check_rank(KW)


def test_argument_errors():
    from mpcracing import rollout as ro
    with pytest.raises(ValueError, match=r"\[9\]\[T\]"):
        ro.rollout_errors(rc.LOG[:8], rc.SETS[0], "linear", 3, **KW)
    with pytest.raises(ValueError, match="expected"):
        ro.rollout_errors(rc.LOG, rc.SETS[0], "pacejka", 3, **KW)
    with pytest.raises(ValueError, match="unknown tyre kind"):
        ro.rollout_errors(rc.LOG, rc.SETS[0], "mlp", 3, **KW)
    r = ro.rollout_errors(rc.LOG, rc.SETS[0], "linear", 3, **KW)  # default: every admissible row
    assert r.pred is None and (r.count == rc.T - 3).all() and r.mean.shape == (1, 3, 6)
