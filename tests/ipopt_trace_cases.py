"""Shared by tests/test_ipopt_trajectory.py and tests/test_gpu_ipopt_trajectory.py: the committed log of the
dense IPOPT oracle (tests/golden/ipopt_trace_golden.npz / .json, generator make_ipopt_trace_golden.py) and the
bars a solver build's iteration trace is held to against it.

Bars (the issue's, from the existing live-oracle tests): alpha, theta and kkt to 1e-6 relative (two linear
algebras, the same arithmetic), theta with 1e-10 absolute on top (near feasibility it is roundoff of the defects);
mu and delta to 1e-12 relative (products of IPOPT's constants).  Only the first ``n_cmp`` rows of a case are
compared -- the generator set n_cmp where both host builds are still within 1e-8 of the oracle, 100 times inside
the bar.  lam_g: tests/test_duals.py's bar, 1e-7 of max |lam_g|.
"""
import importlib.util
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_ipopt_trace_golden",
                                                  os.path.join(GOLDEN, "make_ipopt_trace_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _generator()
TRACE_COL, LOG_COL = GEN.TRACE_COL, GEN.LOG_COL
RTOL = dict(alpha=1e-6, theta=1e-6, kkt=1e-6, mu=1e-12, delta=1e-12)
THETA_ATOL = 1e-10

_cache = {}


def fixture():
    """(arrays keyed "<case>/<name>", index keyed by case); loaded once and never modified."""
    if not _cache:
        with np.load(GEN.NPZ) as z:
            arrays = {k: z[k] for k in z.files}
        for v in arrays.values():
            v.setflags(write=False)
        with open(GEN.INDEX) as f:
            _cache["f"] = (arrays, json.load(f))
    return _cache["f"]


def cases(*kinds):
    return [c for c, (_n, _i, kind) in GEN.CASES.items() if kind in kinds]


def check_rows(case, trace, label, fx=None):
    """The first n_cmp rows of ``trace`` [rows][8] (mr_outputs.trace) against the oracle's log, at the bars
    above.  Returns the worst relative deviation per column (theta: after its absolute allowance).  ``fx``: another
    fixture of the same layout as (arrays, index) -- tests/config_grid_cases.py -- instead of this module's."""
    arrays, index = fx or fixture()
    log, n = arrays[f"{case}/log"], index[case]["n_cmp"]
    assert n >= 1 and not log[:n, LOG_COL["in_resto"]].any()
    assert (trace[:n, TRACE_COL["marker"]] > -200.0).all(), f"{label} {case}: restoration rows within n_cmp"
    worst = {}
    for col, rtol in RTOL.items():
        mine, ref = trace[:n, TRACE_COL[col]], log[:n, LOG_COL[col]]
        worst[col] = float(GEN.rel_dev(mine, ref, THETA_ATOL if col == "theta" else 0.0).max())
    print(f"{label} {case}: {n} rows, worst relative deviation " +
          " ".join(f"{c} {v:.1e}" for c, v in worst.items()))
    for col, rtol in RTOL.items():
        mine, ref = trace[:n, TRACE_COL[col]], log[:n, LOG_COL[col]]
        np.testing.assert_allclose(mine, ref, rtol=rtol, atol=THETA_ATOL if col == "theta" else 0.0,
                                   err_msg=f"{label} {case}: {col} (rows are iterations)")
    return worst


def check_whole(case, status, iters, obj, label, fx=None):
    """A whole-solve case compared to its last row: the same termination iteration, status and objective."""
    _arrays, index = fx or fixture()
    e = index[case]
    if not e["whole"]:
        return
    assert e["n_cmp"] == e["rows"] == e["iters"]
    assert (int(status), int(iters)) == (e["status"], e["iters"]), f"{label} {case}: status / iterations"
    np.testing.assert_allclose(obj, e["obj"], rtol=1e-10, err_msg=f"{label} {case}: objective")


def check_lam_g(case, mine, label, fx=None):
    """tests/test_duals.py::_check: every present row within 1e-7 of max |lam_g|; absent rows are NaN."""
    arrays, _index = fx or fixture()
    lg = arrays[f"{case}/lam_g"]
    ok = ~np.isnan(mine)
    assert ok.sum() == len(lg), f"{label} {case}: {int(ok.sum())} rows present, {len(lg)} expected"
    err = np.abs(lg - mine[ok]).max()
    print(f"{label} {case}: lam_g error {err / np.abs(lg).max():.1e} of max |lam_g|")
    assert err <= 1e-7 * np.abs(lg).max(), f"{label} {case}: lam_g off by {err}"
