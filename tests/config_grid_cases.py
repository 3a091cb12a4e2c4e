"""Shared by tests/test_config_grid.py and tests/test_gpu_config_grid.py: the committed log of the dense IPOPT
oracle over the grid of horizons, models, lane rows and controller / runtime / vehicle parameters
(tests/golden/config_grid_golden.npz / .json, generator make_config_grid_golden.py) and the checks a solver build
is held to against it.

The row, whole-solve and lam_g checks and their bars are tests/ipopt_trace_cases.py's, applied to this fixture
(alpha, theta, kkt to 1e-6 relative, theta with 1e-10 absolute on top; mu and delta to 1e-12; iterations, status
and the objective to 1e-10 where a solve is compared to its end; lam_g to 1e-7 of its largest entry).  check_point
adds the final point of a whole solve: X, U, S, eC, eL to 1e-6 absolute except U[0, N-1] and vx_N, which only the
barrier fixes (tests/test_gpu_golden.py).
"""
import importlib.util
import os

import numpy as np

import ipopt_trace_cases as itc

GOLDEN = itc.GOLDEN


def _generator():
    spec = importlib.util.spec_from_file_location("make_config_grid_golden",
                                                  os.path.join(GOLDEN, "make_config_grid_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _generator()
TRACE_COL, LOG_COL = GEN.TRACE_COL, GEN.LOG_COL
POINT_ATOL = 1e-6

_cache = {}


def fixture():
    """(arrays keyed "<case>/<name>", index keyed by case); loaded once and never modified."""
    if not _cache:
        arrays, index = GEN.load_fixture()
        for v in arrays.values():
            v.setflags(write=False)
        _cache["f"] = (arrays, index)
    return _cache["f"]


def cases(*kinds, mix=False):
    """Case names of the given kinds; the mixed batch's columns only with ``mix``."""
    return [c for c, s in GEN.CASES.items() if s["kind"] in kinds and (mix or s["mix"] is None)]


def check_rows(case, trace, label):
    return itc.check_rows(case, trace, label, fixture())


def check_whole(case, status, iters, obj, label):
    itc.check_whole(case, status, iters, obj, label, fixture())


def check_lam_g(case, mine, label):
    itc.check_lam_g(case, mine, label, fixture())


def check_point(case, o, label, i=0, device=False):
    """The final point of instance ``i`` of the outputs ``o`` against the oracle's; returns the worst difference.

    Status.  A host build ends with the oracle's status in every whole case, also where rounding separates the
    iterates late.  So does the gfx950 build (``device``), with one allowance: where the oracle itself left by the
    acceptable exit (status 1: dyn_N20_Ts0.1_par_whole stalls at the mu floor, its scaled error 1e-11 under tol but
    IPOPT's unscaled tests unmet, and a failed line search ends it after 69 iterations, 75 in the host wave build),
    the device build, which rounds differently (FMA), may find a step there and stay until max_iter (status 2 after
    500 iterations, measured).  It must then still sit at an acceptable point: its final error within
    acceptable_tol of the case's options, besides the final point and lam_g checked as everywhere."""
    arrays, _index = fixture()
    N = GEN.CASES[case]["N"]
    ref = GEN.unpack_sol(arrays[f"{case}/sol"], N)
    status, want = int(o["status"][i]), _index[case]["status"]
    print(f"{label} {case}: status {status} after {int(o['iters'][i])} iterations, final error {o['kkt'][i]:.1e} "
          f"(oracle {want} after {_index[case]['iters']})")
    if device and want == 1 and status == 2:
        assert o["kkt"][i] <= GEN.OPTIONS["whole"]["acceptable_tol"], f"{label} {case}: error {o['kkt'][i]}"
    else:
        assert status == want, f"{label} {case}: status {status}, oracle {want}"
    worst = {}
    for k, r in ref.items():
        d = np.abs(np.asarray(o[k][..., i], np.float64) - r)
        if k == "U":
            d[0, N - 1] = 0.0
        if k == "X":
            d[3, N] = 0.0
        worst[k] = float(d.max())
    print(f"{label} {case}: final point, worst difference " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= POINT_ATOL, f"{label} {case}: {k} off by {v}"
    return worst


def fp32_reference(case):
    """(log rows, markers, host fp32 deviation per column of FP32_COLS) of an fp32 case."""
    arrays, _index = fixture()
    v = arrays[f"{case}/fp32"]
    K = GEN.K_FP32
    return arrays[f"{case}/log"], v[:K], v[K:]


def fp32_dev(case, trace):
    """Worst relative deviation of the first K_FP32 rows of ``trace`` from the oracle per column of FP32_COLS."""
    log, _marker, _host = fp32_reference(case)
    K = GEN.K_FP32
    return {c: float(GEN.T.rel_dev(trace[:K, TRACE_COL[c]], log[:K, LOG_COL[c]]).max()) for c in GEN.FP32_COLS}
