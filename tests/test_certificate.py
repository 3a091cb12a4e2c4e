"""Every returned point certified by the oracle NLP, on the host builds of the solver source (tests/kkt_certificate.py;
tests/test_gpu_certificate.py holds the gfx950 build to the same checks).

Three parts: (1) ``g_opti``, the torch restatement the stationarity residual is differentiated through, equals
``MPCProblem.opti_rows`` row for row; (2) the host builds' outputs pass the certificate at the host's own bars, and
the deviations measured here are the constants ``HOST_DEV`` / ``HOST_STAT`` the device bars are derived from
(the bars they give are within a factor 2 of what this run would give); (3) planted faults in a correct
output set are each flagged at the device's (wider) bars, and the unmodified set passes there.

The emulated wave costs ~10 ms per iteration, so the cases are a few short instances each: instances 8..15 of the
tail recording's C4 set (the shard's first eight; not its 500-iteration solves) in fp32 and four of them
in fp64 at the reference's options, C2 (kin, status 0), C3 (lane rows), C5 (tyres), a batch with state0 throttle /
steer NaN and a u_init, and a mixed-horizon batch through mrh_solve_batch_horizons.
"""
import numpy as np
import pytest
import torch

import horizon_cases as hc
import host_twin as ht
import kkt_certificate as kc

CASES = {
    "C4-fp32": lambda: kc.tail_case("C4", "fp32", "reference", range(8, 16)),
    "C4-fp64": lambda: kc.tail_case("C4", "fp64", "reference", [8, 9, 10, 12]),
    "C2": lambda: kc.config_case("C2", 8),
    "C3-lane": lambda: kc.take_case(kc.config_case("C3", 3), [0, 2]),
    "C5-tyres": lambda: kc.tail_case("C5", "fp32", "reference", range(4)),
    "nan-state0-u_init": lambda: kc.nan_state0_case(8),
    "horizons": lambda: kc.horizons_case((1, 2, 16, 63)),
}
_runs = {}


def host_run(name, scalar=False):
    """(case, outputs) of a host build, solved once per session and never modified."""
    key = (name, scalar)
    if key not in _runs:
        case = CASES[name]()
        c = ht.config(case["N"], case["model"], case["precision"], case["lane"], case["Ts"],
                      **kc.OPTIONS[case["options"]])
        if case["horizon"] is not None:
            out = hc.host_solve(c, case["batch"], case["horizon"], scalar=scalar, duals=not scalar,
                                tyres=case["tyres"])
        else:
            out = ht.solve(c, case["batch"], tyres=case["tyres"], scalar=scalar, duals=not scalar)
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _runs[key] = (case, out)
    return _runs[key]


# ------------------------------------------------------------------------------------------ (1) g_opti
@pytest.mark.parametrize("N,thr,steer", [(1, 0.2, -0.1), (3, None, 0.1), (7, 0.3, None), (5, None, None)])
def test_g_opti_equals_opti_rows(N, thr, steer):
    b = kc.config_case("C2", 1)["batch"]
    inst = kc.wl.instance_dicts(b)[0]
    w = kc.problem(inst, "dyn", N, 0.05, b["runtime"][:, 0]).initial_guess()
    w = w + np.random.default_rng(N).normal(0.0, 0.05, w.size)
    inst["state0"]["throttle"], inst["state0"]["steer"] = thr, steer
    prob = kc.problem(inst, "dyn", N, 0.05, b["runtime"][:, 0])
    g, lo, hi = prob.opti_rows(w)
    mine = kc.g_opti(prob, torch.as_tensor(w)).numpy()
    assert len(g) == 13 * N + 9 - (thr is None) - (steer is None)
    assert np.isfinite(g).all() and np.array_equal(mine, g)


# ------------------------------------------------------------------- (2) the host builds and the yardsticks
@pytest.mark.parametrize("scalar", [False, True], ids=["wave", "scalar"])
@pytest.mark.parametrize("name", list(CASES))
def test_host_build_is_certified(name, scalar):
    """At the host's own bars, max(2 x recorded host deviation, floor) (2 x: the recorded maxima are this build's
    on one CPU; see test_recorded_host_deviations_are_the_measured_ones).  The scalar build exports no lam_g:
    primal checks only."""
    case, out = host_run(name, scalar)
    bad = [(i, st, f) for i, (_c, st, f) in enumerate(kc.certify_batch(case, out, factor=2.0)) if f]
    assert not bad, bad
    if name in ("C2", "nan-state0-u_init", "horizons"):
        assert (out["status"] == 0).all(), out["status"]


def test_recorded_host_deviations_are_the_measured_ones():
    """HOST_DEV / HOST_STAT (the yardsticks of the device bars) against what the host builds give here."""
    dev = {p: {q: 0.0 for q in kc.QUANTITIES} for p in kc.HOST_DEV}
    stat = {k: 0.0 for k in kc.HOST_STAT}
    n_c = 0
    for name in CASES:
        for scalar in (False, True):
            case, out = host_run(name, scalar)
            for cert, status, _f in kc.certify_batch(case, out, factor=1.0):
                assert cert.finite
                for q, v in cert.primal_deviations().items():
                    dev[case["precision"]][q] = max(dev[case["precision"]][q], v)
                if not scalar and kc.in_class_c(status, float(cert.col["kkt"]), kc.OPTIONS[case["options"]]["tol"]):
                    key = (case["precision"], case["options"])
                    stat[key] = max(stat[key], cert.dual()["stat_rel"])
                    n_c += 1
    print("measured host deviations (units):", dev)
    print("measured host relative stationarity:", stat, "instances in (c):", n_c)
    # what matters of a yardstick is the bar it gives, max(8 x deviation, floor): compared there, within a factor 2
    # either way (the host libm's variants between CPUs move a maximum over a few dozen instances by less)
    for p in dev:
        for q, v in dev[p].items():
            a, b = max(v, kc.FLOOR[p] / kc.DEVICE_FACTOR), max(kc.HOST_DEV[p][q], kc.FLOOR[p] / kc.DEVICE_FACTOR)
            assert a <= 2.0 * b and b <= 2.0 * a, (p, q, v, kc.HOST_DEV[p][q])
    for k, v in stat.items():
        fl = kc.STAT_FLOOR[k[0]] / kc.DEVICE_FACTOR
        a, b = max(v, fl), max(kc.HOST_STAT[k], fl)
        assert a <= 2.0 * b and b <= 2.0 * a, (k, v, kc.HOST_STAT[k])
    assert n_c >= 30


# ------------------------------------------------------------------------------------------ (3) planted faults
def _c2_column(i):
    case, out = host_run("C2")
    b = case["batch"]
    prob = kc.problem(kc.wl.instance_dicts(b)[i], case["model"], case["N"], case["Ts"], b["runtime"][:, i])
    col = {k: np.array(v) for k, v in kc.column(out, i).items()}
    return case, prob, col


def _fails(case, prob, col):
    return kc.certify(prob, col, case["precision"], case["options"], kc.OPTIONS[case["options"]]["tol"])[1]


def _pick_instance():
    """The C2 instance whose i = 0 wrap rate rows and i = 1 rate rows differ most in their multipliers."""
    case, out = host_run("C2")
    b0 = 7 + 7 * case["N"]
    d = np.abs(out["lam_g"][b0 + 4:b0 + 6] - out["lam_g"][b0 + 10:b0 + 12]).max(axis=0)
    return int(np.argmax(d))


def _swap(col, a, b):
    lam = col["lam_g"]
    lam[[a, b]] = lam[[b, a]]


def _fault_swap_rows(case, prob, col):
    _swap(col, 7 + 3, 7 + 7 * case["N"] + 2)  # a dynamics row and a steer box row


def _fault_wrap_rows(case, prob, col):
    b0 = 7 + 7 * case["N"]
    _swap(col, b0 + 4, b0 + 10)
    _swap(col, b0 + 5, b0 + 11)


def _fault_negate_dynamics(case, prob, col):
    col["lam_g"][7 + 7 * 2 + 3] *= -1.0


def _fault_move_control(case, prob, col):
    col["U"][1, 3] += 1e-3


def _fault_scale_obj(case, prob, col):
    col["obj"] = col["obj"] * (1.0 + 1e-4)


def _fault_exchange_errors(case, prob, col):
    col["eC"], col["eL"] = col["eL"].copy(), col["eC"].copy()


FAULTS = {"two lam_g rows swapped": _fault_swap_rows, "i = 0 wrap rate rows exchanged with i = 1": _fault_wrap_rows,
          "one dynamics multiplier negated": _fault_negate_dynamics, "U[1, 3] moved by 1e-3": _fault_move_control,
          "obj scaled by 1 + 1e-4": _fault_scale_obj, "eC and eL exchanged": _fault_exchange_errors}


def test_unmodified_outputs_pass_at_the_device_bars():
    for i in range(8):
        case, prob, col = _c2_column(i)
        assert _fails(case, prob, col) == [], i


@pytest.mark.parametrize("fault", list(FAULTS))
def test_planted_fault_is_flagged(fault):
    case, prob, col = _c2_column(_pick_instance())
    assert _fails(case, prob, col) == []
    FAULTS[fault](case, prob, col)
    fails = _fails(case, prob, col)
    print(fault, "->", fails)
    assert fails, fault


def test_constr_viol_without_its_bound_rows_is_flagged():
    """constr_viol replaced by the equality part alone, at a point whose largest violation is a bound row: the
    returned point with S_N pushed 1e-3 past the Delta-S row's upper bound (S_N enters no equality row), its obj
    and constr_viol re-stated for that point by the oracle.  That set passes; the same set with the equality part
    for constr_viol does not."""
    case, prob, col = _c2_column(0)
    N = case["N"]
    col["S"][N] = col["S"][N - 1] + case["Ts"] * prob.fp.v_max + 1e-3
    at = kc.Certificate(prob, col, case["precision"])
    assert at.viol_bound > 100 * at.viol_eq and abs(at.viol_bound - 1e-3) < 1e-9
    col["obj"], col["constr_viol"] = np.float64(at.obj_ref), np.float64(at.viol_ref)
    assert kc.Certificate(prob, col, case["precision"]).primal_failures() == []
    col["constr_viol"] = np.float64(at.viol_eq)
    fails = kc.Certificate(prob, col, case["precision"]).primal_failures()
    assert len(fails) == 1 and fails[0].startswith("viol"), fails


def test_nan_rows_of_lam_g_are_counted():
    """A state0 row that should be NaN but holds a number (or the reverse) fails the certificate's row count."""
    case, out = host_run("nan-state0-u_init")
    b = case["batch"]
    for i, n_nan in ((0, 2), (4, 1), (7, 0)):
        prob = kc.problem(kc.wl.instance_dicts(b)[i], case["model"], case["N"], case["Ts"], b["runtime"][:, i],
                          u_init=b["u_init"][:, :, i])
        col = {k: np.array(v) for k, v in kc.column(out, i).items()}
        assert int(np.isnan(col["lam_g"]).sum()) == n_nan
        kc.Certificate(prob, col, "fp64").lam()
        col["lam_g"][-1] = 0.0 if n_nan == 2 else np.nan
        with pytest.raises(AssertionError, match="NaN rows"):
            kc.Certificate(prob, col, "fp64").lam()
