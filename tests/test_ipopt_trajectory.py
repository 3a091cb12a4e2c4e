"""Iteration-level parity of the solver's IPOPT rules with the dense IPOPT restatement (oracle/ipopt.py).

The product solves the stage-wise restatement of the reference's NLP with a Riccati recursion
(csrc/mr_solver.h, the host build of the same source as the kernel); the oracle solves the NLP in the
reference's own variables (control/MPC.py:62-64) with a full-space KKT matrix and LDL inertia.  IPOPT's
iterates are determined by the step, the inertia correction delta_w (applied to the reference's variables,
mr_solver.h delta_var), the fraction-to-boundary rule and the filter line search, so the two must produce
the same per-iteration primal step size alpha, shift delta, constraint violation theta and barrier
parameter mu -- checked here over the first iterations of
  * a C2 instance (kinematic, no inertia correction), and
  * C3 instance 374 (dynamic model + hard lane rows; delta > 0 from the second iteration on, growing past
    1e2 within these iterations -- the instance the round-2 product left at max_iter).
The oracle runs under ``ipopt.PRODUCT``: IPOPT 3.14's rules (oracle/ipopt.py ``IPOPT``) less the few the
product does not restate (soft restoration, tiny-step termination, the restoration phase's own
watchdog / SOC / least-squares multipliers) -- none of which is reached in these iterations.
Tolerances: alpha, theta 1e-6 relative (different linear algebra, same arithmetic; theta also 1e-10
absolute: near feasibility it is roundoff of the defects), delta and mu exact to 1e-12 (they are products
of IPOPT's constants).

Below the two live-oracle tests, the same comparison runs against the oracle's committed log
(tests/golden/ipopt_trace_golden.npz, generator make_ipopt_trace_golden.py; bars in tests/ipopt_trace_cases.py)
for both host builds -- the scalar solver and the emulated wavefront, the kernel's own source -- over the
kinematic, dynamic + lane rows, blended and blended + Pacejka models: five 14-iteration prefixes and six whole
solves at tol 1e-10 (iterations, status, objective, and for the wave build lam_g -- the scalar build exports
none).  tests/test_gpu_ipopt_trajectory.py holds the gfx950 build to the same fixture.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "mpc-racing_amd"))

import host_twin as ht  # noqa: E402
import ipopt_trace_cases as itc  # noqa: E402
from mpcracing import workload as wl  # noqa: E402


@pytest.mark.parametrize("name,i,K", [("C2", 5, 9), ("C3", 374, 14)])
def test_iterates_match_dense_ipopt(name, i, K):
    from oracle.ipopt import PRODUCT, solve_ipopt
    from oracle.nlp import MPCProblem
    cfg = wl.CONFIGS[name]
    b = wl.make_batch(name, limit=i + 1)
    sub = {k: (v[..., i:i + 1].copy() if v is not None else None) for k, v in b.items()}
    c = ht.config(cfg["N"], cfg["model"], "fp64", cfg["lane"], cfg["Ts"], tol=1e-8, acceptable_iter=15,
                  acceptable_tol=1e-6)
    tr = ht.solve(c, sub, nthreads=1, scalar=True, trace_instance=0, trace_cap=520)["trace"]
    inst = wl.instance_dicts(b)[i]
    p = MPCProblem(inst["state0"], inst["s0"], inst["cx"], inst["cy"], inst["max_error"], N=cfg["N"],
                   Ts=cfg["Ts"], model=cfg["model"], lane_bounds=cfg["lane"])
    r = solve_ipopt(p, tol=1e-8, max_iter=K, acceptable_tol=1e-6, acceptable_iter=15, log=True, rules=PRODUCT)
    rows = r.log[:K]
    assert len(rows) >= min(K, 8)
    for j, (_it, _kkt, mu, alpha, delta, th, _ph, in_resto) in enumerate(rows):
        assert not in_resto
        np.testing.assert_allclose(tr[j, 2], alpha, rtol=1e-6, err_msg=f"{name} {i} iteration {j}: alpha")
        np.testing.assert_allclose(tr[j, 4], delta, rtol=1e-12, err_msg=f"{name} {i} iteration {j}: delta")
        np.testing.assert_allclose(tr[j, 5], th, rtol=1e-6, atol=1e-10, err_msg=f"{name} {i} iteration {j}: theta")
        np.testing.assert_allclose(tr[j, 1], mu, rtol=1e-12, err_msg=f"{name} {i} iteration {j}: mu")
    if name == "C3":
        assert max(row[4] for row in rows) > 1e2  # the inertia correction is exercised


@pytest.mark.parametrize("i", [1, 10])
def test_whole_solve_matches_dense_ipopt(i):
    """Over a whole C2 solve (kinematic, tol 1e-8): the same optimality error at every iteration (IPOPT's
    scaled stationarity / primal / complementarity measure on the reference's NLP, mr_solver.h
    MR_KKT_RESTATED), hence the same barrier-parameter updates, the same termination iteration and the
    same objective.  (Instance 1 ended one iteration later than IPOPT while the error was measured on the
    restatement.)"""
    from oracle.ipopt import PRODUCT, solve_ipopt
    from oracle.nlp import MPCProblem
    cfg = wl.CONFIGS["C2"]
    b = wl.make_batch("C2", limit=i + 1)
    sub = {k: (v[..., i:i + 1].copy() if v is not None else None) for k, v in b.items()}
    c = ht.config(cfg["N"], cfg["model"], "fp64", cfg["lane"], cfg["Ts"], tol=1e-8, acceptable_iter=15,
                  acceptable_tol=1e-6)
    o = ht.solve(c, sub, nthreads=1, scalar=True, trace_instance=0, trace_cap=520)
    inst = wl.instance_dicts(b)[i]
    p = MPCProblem(inst["state0"], inst["s0"], inst["cx"], inst["cy"], inst["max_error"], N=cfg["N"],
                   Ts=cfg["Ts"], model=cfg["model"], lane_bounds=cfg["lane"])
    r = solve_ipopt(p, tol=1e-8, max_iter=500, acceptable_tol=1e-6, acceptable_iter=15, log=True, rules=PRODUCT)
    assert r.status == 0 and int(o["status"][0]) == 0
    assert int(o["iters"][0]) == r.iters
    for j, row in enumerate(r.log):
        np.testing.assert_allclose(o["trace"][j, 0], row[1], rtol=1e-6, err_msg=f"iteration {j}: kkt")
        np.testing.assert_allclose(o["trace"][j, 1], row[2], rtol=1e-12, err_msg=f"iteration {j}: mu")
    np.testing.assert_allclose(o["obj"][0], r.obj, rtol=1e-10)


# ---- the oracle's committed log (tests/golden/ipopt_trace_golden.npz) against both host builds ----

_solves = {}


def _host(case, scalar):
    """One host solve per (case, build), shared by the tests below."""
    if (case, scalar) not in _solves:
        _solves[case, scalar] = itc.GEN.host_trace(case, scalar)
    return _solves[case, scalar]


def test_ipopt_trace_fixture():
    """The fixture itself: its inputs are what mpcracing.workload makes today, every case keeps its promised
    number of comparable rows, and the inertia correction is exercised (delta > 1e2 in C3_374, >= 100 in C5_0:
    without those the shift's growth rule would go unchecked)."""
    arrays, index = itc.fixture()
    G = itc.GEN
    assert sorted(index) == sorted(G.CASES)
    assert os.path.getsize(G.NPZ) + os.path.getsize(G.INDEX) < 100 * 1024
    for case, (name, i, kind) in G.CASES.items():
        e = index[case]
        assert (e["config"], e["instance"], e["kind"], e["options"]) == (name, i, kind, G.OPTIONS[kind])
        sub = G.case_inputs(case)
        for k in G.IN_KEYS:
            if sub[k] is None:
                assert f"{case}/in_{k}" not in arrays, (case, k)
            else:
                assert np.array_equal(arrays[f"{case}/in_{k}"], sub[k], equal_nan=True), (case, k)
        log = arrays[f"{case}/log"]
        assert log.shape == (e["rows"], 7) and np.isfinite(log).all()
        need = G.MIN_N_CMP.get(case, G.MIN_N_CMP[kind])
        assert e["whole"] == (e["status"] == 0 and e["n_cmp"] == e["rows"] == e["iters"])
        assert e["whole"] if need is None else need <= e["n_cmp"] <= e["rows"]
        assert not log[:e["n_cmp"], itc.LOG_COL["in_resto"]].any()
        assert max(e["host_worst_dev"][c] for c in ("alpha", "theta", "kkt")) <= G.N_CMP_RTOL
        if kind == "whole":
            assert e["status"] == 0 and arrays[f"{case}/lam_g"].shape == (13 * G.case_config(case)["N"] + 9 -
                                                                          2 * (case == "C1dyn_nan"),)
        if kind == "fp32":
            assert arrays[f"{case}/marker"].shape == (G.K_FP32,)
            assert arrays[f"{case}/fp32_dev"].shape == (len(G.FP32_COLS),)
    d = itc.LOG_COL["delta"]
    assert arrays["C3_374/log"][:index["C3_374"]["n_cmp"], d].max() > 1e2
    assert arrays["C5_0/log"][:, d].max() >= 100.0
    assert np.isnan(arrays["C1dyn_nan/in_state0"][6:]).all()


@pytest.mark.parametrize("scalar", [True, False], ids=["scalar", "wave"])
@pytest.mark.parametrize("case", itc.cases("prefix", "whole"))
def test_host_build_iterates_match_oracle_log(case, scalar):
    """alpha, theta, kkt to 1e-6, mu and delta to 1e-12 over the case's n_cmp rows; a whole solve that is compared
    to its end also stops at the oracle's iteration with its status and (to 1e-10) its objective."""
    label = "scalar" if scalar else "wave"
    o = _host(case, scalar)
    itc.check_rows(case, o["trace"], label)
    itc.check_whole(case, o["status"][0], o["iters"][0], o["obj"][0], label)


@pytest.mark.parametrize("case", itc.cases("whole"))
def test_wave_lam_g_matches_oracle_log(case):
    """The emulated wave's exported lam_g against the oracle's multipliers in Opti row order; C1dyn_nan: the two
    state0 rows absent (NaN), the other 13N+7 matching."""
    o = _host(case, False)
    assert o["status"][0] == 0
    lam = o["lam_g"][:, 0]
    assert np.isnan(lam[-2:]).all() == (case == "C1dyn_nan") and not np.isnan(lam[:-2]).any()
    itc.check_lam_g(case, lam, "wave")
