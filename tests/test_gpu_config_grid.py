"""The gfx950 build against the dense IPOPT oracle's committed log over the configuration grid.

tests/test_config_grid.py holds both host builds of the solver source to tests/golden/config_grid_golden.npz
(generator make_config_grid_golden.py, checks in tests/config_grid_cases.py); this file holds libmpcracing.so to the
same fixture through BatchSolver(N, model, precision, lane, Ts, max_batch, tyres=, **overrides).solve(
trace_instance=, trace_cap=, duals=).  The kernel maps stage k to lane k, forms its MFMA operands per group of 16
lanes and keeps special slots above stage N; its per-stage and per-instance constants (bounds, weights, the runtime
row, the vehicle block) reach the line search and the SOC tries through registers and LDS.  The horizons here fill,
just miss and just cross every 16-lane group up to N = 63, and every constant differs from its default and from its
neighbours, so a stage mapped to the wrong lane, a folded constant or a runtime row read at another instance's
column moves alpha, theta or kkt of some iteration by far more than the 1e-6 they are held to.  No oracle solve
runs here: the fixture is read only.

* fp64 rows of every prefix / whole case and of every column of the mixed batches (bars of
  ipopt_trace_cases.check_rows over n_cmp rows); whole solves: iterations / status / objective where compared to
  the end, the final point to 1e-6 (U[0, N-1], vx_N excepted) and, without lane rows, lam_g.
* mixed batch under dispatch_order 0 and 1: instance j of the batch of five runtime columns is the B = 1 solve of
  column j bit for bit.
* fp32, first 8 rows at the reference's options: markers and delta's zero pattern equal, every column within
  max(8 x the host fp32 build's recorded deviation, 1e-5) relative of the oracle.
One solver handle per configuration, cached in the module; every solve is B <= 5.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import config_grid_cases as cg  # noqa: E402
from mpcracing.batch import BatchSolver  # noqa: E402

G = cg.GEN
TRACE_CAP = 520  # max_iter (500) + the final record clear of the reserved rows
RESERVED = 4     # rows the kernel keeps out of the iteration rows' reach (tests/test_gpu_ipopt_trajectory.py)
ROWS = TRACE_CAP - RESERVED

_handles = {}
_solves = {}


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _handle(case, precision="fp64", order=0):
    s = G.CASES[case]
    key = (s["N"], s["model"], precision, s["lane"], s["Ts"], s["kind"], s["par"], s["veh"], order)
    if key not in _handles:
        _handles[key] = BatchSolver(s["N"], s["model"], precision, s["lane"], s["Ts"], max_batch=5,
                                    tyres=G.case_tyres(case), dispatch_order=order, **G.OPTIONS[s["kind"]],
                                    **G.case_overrides(case))
    return _handles[key]


def _solve(case, precision="fp64", order=0, batch=None, trace_instance=0):
    o = _np(_handle(case, precision, order).solve(batch if batch is not None else G.case_inputs(case),
                                                  trace_instance=trace_instance, trace_cap=TRACE_CAP, duals=True))
    assert (0 <= o["iters"]).all() and (o["iters"] < ROWS).all(), "iteration rows would reach the reserved rows"
    return o


def _gpu(case, precision="fp64"):
    """One B = 1 GPU solve per (case, precision), shared by the tests below."""
    if (case, precision) not in _solves:
        _solves[case, precision] = _solve(case, precision)
    return _solves[case, precision]


@pytest.mark.parametrize("case", cg.cases("prefix", "whole", mix=True))
def test_gpu_fp64_iterates_match_oracle_log(case):
    o = _gpu(case)
    cg.check_rows(case, o["trace"][:ROWS], "gfx950")
    if G.CASES[case]["kind"] == "whole":
        cg.check_whole(case, o["status"][0], o["iters"][0], o["obj"][0], "gfx950")
        cg.check_point(case, o, "gfx950", device=True)


@pytest.mark.parametrize("case", [c for c in cg.cases("whole") if not G.CASES[c]["lane"]])
def test_gpu_fp64_lam_g_matches_oracle_log(case):
    lam = _gpu(case)["lam_g"][:, 0]
    assert not np.isnan(lam).any()
    cg.check_lam_g(case, lam, "gfx950")


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("group", sorted(G.MIX_GROUPS))
def test_gpu_mixed_runtime_batch(group, order):
    """Five different runtime columns (and NaN state0 controls in two) in one batch, under both dispatch orders:
    instance j is the B = 1 solve of column j bit for bit, and meets the oracle's rows of that column."""
    cols = G.MIX_GROUPS[group]
    batch = G.stack_inputs(cols)
    for j, case in enumerate(cols):
        one = _gpu(case)
        o = _solve(case, order=order, batch=batch, trace_instance=j)
        assert np.array_equal(o["trace"][:ROWS].view(np.uint64), one["trace"][:ROWS].view(np.uint64)), (group, j)
        for k, v in one.items():
            if k != "trace":
                mine = np.ascontiguousarray(o[k][..., j:j + 1])
                assert mine.dtype == v.dtype and np.array_equal(mine.view(np.uint8), v.view(np.uint8)), (group, j, k)
        cg.check_rows(case, o["trace"][:ROWS], f"gfx950 order {order} batch[{j}]")


@pytest.mark.parametrize("case", cg.cases("fp32"))
def test_gpu_fp32_first_rows_match_oracle_log(case):
    """Markers (the host fp64 wave build's on the oracle's trajectory) and delta's zero pattern equal; kkt, mu,
    alpha, delta, theta, phi within max(8 x host fp32 deviation, 1e-5) relative of the oracle."""
    log, marker, host_dev = cg.fp32_reference(case)
    K = G.K_FP32
    o = _gpu(case, "fp32")
    assert o["iters"][0] >= K
    tr = o["trace"][:K]
    dev = cg.fp32_dev(case, tr)
    bar = {c: max(8.0 * float(h), 1e-5) for c, h in zip(G.FP32_COLS, host_dev)}
    print(f"gfx950 fp32 {case}: markers {tr[:, 7].astype(int).tolist()}")
    for c, h in zip(G.FP32_COLS, host_dev):
        print(f"gfx950 fp32 {case}: {c:6s} deviation {dev[c]:.2e}  host fp32 {h:.2e}  bar {bar[c]:.2e}")
    assert np.array_equal(tr[:, cg.TRACE_COL["marker"]], marker)
    assert np.array_equal(tr[:, cg.TRACE_COL["delta"]] == 0.0, log[:K, cg.LOG_COL["delta"]] == 0.0)
    for c in G.FP32_COLS:
        assert dev[c] <= bar[c], (case, c, dev[c], bar[c])
