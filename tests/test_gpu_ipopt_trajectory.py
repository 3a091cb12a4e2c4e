"""The gfx950 build's iterates and multipliers against the dense IPOPT oracle's committed log.

tests/test_ipopt_trajectory.py holds both host builds of the solver source to tests/golden/ipopt_trace_golden.npz
(generator make_ipopt_trace_golden.py, bars in tests/ipopt_trace_cases.py); this file holds libmpcracing.so to the
same fixture through BatchSolver.solve(trace_instance=, trace_cap=, duals=).  An interior-point method corrects
itself, so a device Riccati factorisation, MFMA fragment layout, DPP reduction or fraction-to-boundary reduction
that is slightly off still reaches the optimum a few iterations later and passes every final-point test; it
cannot keep alpha, theta and kkt of every iteration within 1e-6 of the oracle, nor mu and delta exact.  The
device halves of mr_wave_prims.h exist only in this build.  No oracle solve runs here: the fixture is read only.

* fp64 trace, every prefix and whole-solve case (kinematic, dynamic + lane rows, blended, blended + Pacejka,
  config 1 dynamic with and without state0 controls): the bars of ipopt_trace_cases.check_rows over the case's
  n_cmp rows, and iterations / status / objective where a whole solve is compared to its end.
* fp64 lam_g of every whole-solve case (tests/test_duals.py's bar); C1dyn_nan: its two state0 rows NaN.
* trace addressing: instance 7 of a C4 batch of 200, traced under dispatch_order 0, 1 and 2, in fp32 and fp64.
* fp32, first 8 rows of C4_0 and C5_0 at the reference's options: markers and delta's zero pattern equal, every
  numeric column within max(8 x the host fp32 build's recorded deviation from the oracle, 1e-5) relative.  The
  factor 8 is for what the device build has and the IEEE host build has not: FMA contraction and the few-ulp
  hardware reciprocal, square root and transcendentals.

The wave kernel keeps the last MR_TRACE_RESERVED rows of a trace buffer (2; 4 in a cycle-counter build) out of
the iteration rows' reach: TRACE_CAP leaves the longest solve here (86 iterations + the final record) clear of
them, and RESERVED = 4 rows are never compared.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import ipopt_trace_cases as itc  # noqa: E402
from mpcracing import workload as wl  # noqa: E402
from mpcracing.batch import BatchSolver, solver_for_config  # noqa: E402

G = itc.GEN
TRACE_CAP = 128
RESERVED = 4
ROWS = TRACE_CAP - RESERVED

_solves = {}


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _gpu(case, precision="fp64"):
    """One B = 1 GPU solve per (case, precision), shared by the tests below."""
    if (case, precision) not in _solves:
        cfg = G.case_config(case)
        s = BatchSolver(cfg["N"], cfg["model"], precision, cfg["lane"], cfg["Ts"], max_batch=1,
                        tyres=G.case_tyres(case), **G.OPTIONS[G.CASES[case][2]])
        o = _np(s.solve(G.case_inputs(case), trace_instance=0, trace_cap=TRACE_CAP, duals=True))
        assert 0 <= o["iters"][0] < ROWS, "iteration rows would reach the reserved rows: raise TRACE_CAP"
        _solves[case, precision] = o
    return _solves[case, precision]


@pytest.mark.parametrize("case", itc.cases("prefix", "whole"))
def test_gpu_fp64_iterates_match_oracle_log(case):
    o = _gpu(case)
    itc.check_rows(case, o["trace"][:ROWS], "gfx950")
    itc.check_whole(case, o["status"][0], o["iters"][0], o["obj"][0], "gfx950")


@pytest.mark.parametrize("case", itc.cases("whole"))
def test_gpu_fp64_lam_g_matches_oracle_log(case):
    o = _gpu(case)
    assert o["status"][0] == 0
    lam = o["lam_g"][:, 0]
    assert np.isnan(lam[-2:]).all() == (case == "C1dyn_nan") and not np.isnan(lam[:-2]).any()
    itc.check_lam_g(case, lam, "gfx950")


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_trace_addressing(precision):
    """The trace follows the instance, not the workgroup: instance 7 of 200 traced under every dispatch order
    gives the rows and outputs of its solve alone, bit for bit; nothing else of the zeroed buffer is written
    (the reserved rows aside); and a trace_instance that names no instance (-1, B) leaves the buffer zero."""
    B, i = 200, 7
    b = wl.make_batch("C4", limit=B)
    one = {k: (np.ascontiguousarray(v[..., i:i + 1]) if v is not None else None) for k, v in b.items()}
    ref = _np(solver_for_config("C4", 1, precision=precision).solve(one, trace_instance=0, trace_cap=TRACE_CAP,
                                                                    duals=True))
    n = int(ref["iters"][0])
    assert 0 < n < ROWS - 1 and ref["trace"][n, 7] == 1000.0 + ref["status"][0]
    assert (ref["trace"][:n, 1] > 0).all() and not ref["trace"][n + 1:ROWS].any()
    hint = np.random.default_rng(11).integers(0, 400, B).astype(np.int32)
    for order in (0, 1, 2):
        s = solver_for_config("C4", B, precision=precision, dispatch_order=order)
        bb = dict(b, order_hint=hint) if order == 2 else b
        o = _np(s.solve(bb, trace_instance=i, trace_cap=TRACE_CAP, duals=True))
        assert np.array_equal(o["trace"][:ROWS].view(np.uint64), ref["trace"][:ROWS].view(np.uint64)), order
        for k, v in ref.items():
            if k != "trace":
                mine = np.ascontiguousarray(o[k][..., i:i + 1])
                assert mine.dtype == v.dtype and np.array_equal(mine.view(np.uint8), v.view(np.uint8)), (order, k)
        for none in (-1, B):
            z = _np(s.solve(bb, trace_instance=none, trace_cap=TRACE_CAP))
            assert not z["trace"].view(np.uint64).any(), (order, none)
            assert np.array_equal(z["iters"], o["iters"]), (order, none)


@pytest.mark.parametrize("case", itc.cases("fp32"))
def test_gpu_fp32_first_rows_match_oracle_log(case):
    """Markers (the host fp64 wave build's on the oracle's trajectory, see the generator) and delta's zero pattern
    equal; kkt, mu, alpha, delta, theta, phi within max(8 x host fp32 deviation, 1e-5) relative of the oracle.

    Measured on an MI355X (worst relative deviation from the oracle over the 8 rows; host fp32 build in brackets):
      C4_0_ref  kkt 2.1e-6 (1.5e-6)  mu 1.5e-8 (1.5e-8)  alpha 4.9e-6 (3.9e-6)  delta 0 (0)
                theta 4.5e-5 (3.8e-5)  phi 1.3e-4 (1.3e-4)
      C5_0_ref  kkt 1.7e-6 (1.8e-6)  mu 1.5e-8 (1.5e-8)  alpha 2.8e-5 (8.5e-6)  delta 2.7e-7 (5.3e-8)
                theta 4.8e-4 (4.5e-4)  phi 2.3e-6 (2.8e-6)
    The device build is at most 3.3 x the host build's deviation (alpha of C5_0_ref, bar 6.8e-5) where the bar is
    8 x, and 5.2 x on delta of C5_0_ref, where the 1e-5 floor is the bar: the factor 8 was not widened."""
    arrays, _index = itc.fixture()
    log, marker, host_dev = arrays[f"{case}/log"], arrays[f"{case}/marker"], arrays[f"{case}/fp32_dev"]
    K = G.K_FP32
    o = _gpu(case, "fp32")
    assert o["iters"][0] >= K
    tr = o["trace"][:K]
    dev = {c: float(G.rel_dev(tr[:, itc.TRACE_COL[c]], log[:K, itc.LOG_COL[c]]).max()) for c in G.FP32_COLS}
    bar = {c: max(8.0 * float(h), 1e-5) for c, h in zip(G.FP32_COLS, host_dev)}
    print(f"gfx950 fp32 {case}: markers {tr[:, 7].astype(int).tolist()}")
    for c in G.FP32_COLS:
        print(f"gfx950 fp32 {case}: {c:6s} deviation {dev[c]:.2e}  host fp32 {host_dev[G.FP32_COLS.index(c)]:.2e}"
              f"  bar {bar[c]:.2e}")
    assert np.array_equal(tr[:, itc.TRACE_COL["marker"]], marker[:K])
    assert np.array_equal(tr[:, itc.TRACE_COL["delta"]] == 0.0, log[:K, itc.LOG_COL["delta"]] == 0.0)
    for c in G.FP32_COLS:
        assert dev[c] <= bar[c], (case, c, dev[c], bar[c])
