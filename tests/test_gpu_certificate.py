"""Every point the gfx950 build returns, certified by the oracle NLP (tests/kkt_certificate.py): the outputs a caller
gets back -- constr_viol, obj, eC, eL, lam_g and what the status claims -- re-derived in fp64 from the returned X, U, S
alone, at every exit of the solve and at both precisions.  The library only (BatchSolver.solve(b, duals=True)), one
launch per case; inputs from mpcracing.workload, references from oracle/.

Per instance:
 (a) every exit with finite outputs: constr_viol, obj, eC, eL are the oracle's at the returned point;
 (b) status 0 / 1: the oracle's violation and the one-sided complementarity of lam_g meet IPOPT's thresholds
     (1e-4 / 1e-2), with the allowance max|lam| (viol_ref + relax) and the precision's bar;
 (c) status 0, 1 and status 3 with kkt <= tol (the original problem's iterate at the claimed tolerance): no
     wrong-signed multiplier on a one-sided row and the relative stationarity of grad f + J^T lam_g within the bar;
 (d) status 2 and exits inside the restoration phase: primal checks only (include/mpcracing.h says what lam_g holds
     there); the NaN rows of lam_g are checked at every exit.
Bars: max(8 x the host builds' deviation, floor), the constants of tests/kkt_certificate.py (measured on the CPU by
tests/test_certificate.py; DESIGN.md §4 lists them with the gfx950 maxima this test prints).  Coverage is asserted:
C4 fp32 puts >= 20 instances through (c) and reaches statuses 1, 2 and 3; C3 puts >= 24 status-0 instances through
(c), C2 >= 24 instances.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import kkt_certificate as kc  # noqa: E402

CASES = {
    "C4-fp32": lambda: kc.tail_case("C4", "fp32", "reference"),
    "C4-fp64": lambda: kc.tail_case("C4", "fp64", "reference"),
    "C5": lambda: kc.tail_case("C5", "fp32", "reference"),
    "C3": lambda: kc.tail_case("C3", "fp64", "default"),
    "C2": lambda: kc.config_case("C2", 32),
    "nan-state0-u_init": lambda: kc.nan_state0_case(8),
    "horizons": lambda: kc.horizons_case(),
}
# name -> (least number of instances through (c), statuses that must occur, least status-0 instances through (c))
COVERAGE = {"C4-fp32": (20, (1, 2, 3), 0), "C2": (24, (), 0), "C3": (24, (0,), 24)}


def _solve(case):
    from mpcracing.batch import BatchSolver
    b = case["batch"]
    B = int(b["s0"].shape[0])
    s = BatchSolver(case["N"], case["model"], case["precision"], case["lane"], case["Ts"], max_batch=B,
                    tyres=case["tyres"], **kc.OPTIONS[case["options"]])
    if case["horizon"] is not None:
        b = dict(b, horizon=case["horizon"])
    return {k: v.cpu().numpy() for k, v in s.solve(b, duals=True).items()}


@pytest.mark.parametrize("name", list(CASES))
def test_gpu_outputs_are_certified(name):
    case = CASES[name]()
    out = _solve(case)
    tol = kc.OPTIONS[case["options"]]["tol"]
    res = kc.certify_batch(case, out)
    status = np.array([st for _c, st, _f in res])
    in_c = np.array([c.finite and kc.in_class_c(st, float(c.col["kkt"]), tol) for c, st, _f in res])
    # the figures, before anything is asserted
    dev = {q: 0.0 for q in kc.QUANTITIES}
    err = {q: 0.0 for q in kc.QUANTITIES}
    stat = wrong = compl = 0.0
    for (c, st, _f), cc in zip(res, in_c):
        if not c.finite:
            continue
        d, e = c.primal_deviations(), c.primal_errors()
        for q in dev:
            if np.isfinite(d[q]):
                dev[q], err[q] = max(dev[q], d[q]), max(err[q], e[q])
        if cc:
            du = c.dual(13 * case["N"] + 9)
            stat, wrong = max(stat, du["stat_rel"]), max(wrong, du["wrong_sign"] / du["norm"])
            if st in (0, 1):
                compl = max(compl, du["compl"])
    c0 = res[0][0]
    print(f"\n{name} {case['precision']} {case['options']}: statuses {np.bincount(status, minlength=5).tolist()} "
          f"finite {sum(c.finite for c, _s, _f in res)} in (c) {int(in_c.sum())}")
    print("  gfx950 max deviations (units): " + " ".join(f"{q} {dev[q]:.3g} (abs {err[q]:.3g})" for q in dev))
    print("  bars (units): " + " ".join(
        f"{q} {max(kc.DEVICE_FACTOR * kc.HOST_DEV[case['precision']][q], kc.FLOOR[case['precision']]):.3g}"
        for q in dev))
    print(f"  gfx950 max relative stationarity {stat:.3g} (bar {c0.stat_bar(case['options']):.3g}) "
          f"wrong sign / norm {wrong:.3g} complementarity at status 0 / 1 {compl:.3g}")
    bad = [(i, st, f) for i, (_c, st, f) in enumerate(res) if f]
    for row in bad:
        print("  FAIL", row)
    assert not bad, bad
    claimed = np.isin(status, (0, 1))
    assert all(c.finite for (c, _s, _f), cl in zip(res, claimed) if cl)
    if name in COVERAGE:
        n_c, statuses, n_c0 = COVERAGE[name]
        assert int(in_c.sum()) >= n_c, (name, int(in_c.sum()))
        assert all((status == s).any() for s in statuses), (name, np.bincount(status).tolist())
        assert int((in_c & (status == 0)).sum()) >= n_c0, (name, int((in_c & (status == 0)).sum()))
    if name in ("nan-state0-u_init", "horizons"):
        assert (status == 0).all(), status
