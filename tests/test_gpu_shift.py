"""The gfx950 build against the dense IPOPT oracle where the inertia shift is large at once.

tests/test_shift.py holds both host builds to tests/golden/shift_golden.npz (generator make_shift_golden.py: slow C3
cars under braking that accept delta = 100 in their first iteration, rows selected by the scalar build alone); this
file holds libmpcracing.so in fp64 to the same rows at the same bars (tests/ipopt_trace_cases.py: alpha, theta, kkt to
1e-6 relative, mu and delta to 1e-12).  The device build runs the wave algorithm of the host emulation with FMA
contraction on top; the other oracle files cannot see a loss of accuracy that only the wave path has, because their
rows were selected where both host builds agree with the oracle.

Every case is a B = 1 solve of at most 12 iterations at N = 40 with trace_instance = 0.  One more test solves the
twelve lane-row instances as one batch and traces instance 79 under dispatch_order 0 and 1: the trace follows the
instance, bit for bit, as tests/test_gpu_ipopt_trajectory.py::test_trace_addressing has it.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import shift_cases as sc  # noqa: E402
from mpcracing.batch import BatchSolver  # noqa: E402

G = sc.GEN
TRACE_CAP = 32  # 12 iteration rows + the final record, clear of the reserved rows
RESERVED = 4    # rows the kernel keeps out of the iteration rows' reach (tests/test_gpu_ipopt_trajectory.py)
ROWS = TRACE_CAP - RESERVED

_handles = {}
_solves = {}


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _handle(lane, max_batch=1, order=0):
    key = (lane, max_batch, order)
    if key not in _handles:
        cfg = dict(G.case_config(next(iter(G.CASES))), lane=lane)
        _handles[key] = BatchSolver(cfg["N"], cfg["model"], "fp64", lane, cfg["Ts"], max_batch=max_batch,
                                    dispatch_order=order, **G.OPT)
    return _handles[key]


def _gpu(case):
    """One B = 1 GPU solve per case, shared by the tests below."""
    if case not in _solves:
        o = _np(_handle(G.CASES[case]["lane"]).solve(G.case_inputs(case), trace_instance=0, trace_cap=TRACE_CAP,
                                                     duals=True))
        assert 0 <= o["iters"][0] <= G.K_SHIFT < ROWS
        _solves[case] = o
    return _solves[case]


@pytest.mark.parametrize("case", sc.cases("shift", "control"))
def test_gpu_fp64_iterates_match_oracle_log(case):
    sc.check_rows(case, _gpu(case)["trace"][:ROWS], "gfx950")


def test_gpu_shift_batch_trace_addressing():
    """The twelve lane-row instances as one batch: instance 79's trace and outputs under dispatch_order 0 and 1 are
    those of its B = 1 solve, bit for bit."""
    inst = list(G.SHIFT)
    j = inst.index(79)
    batch = G.take(G.batch(), inst)
    one = _gpu("C3_79")
    n = int(one["iters"][0])
    assert n == G.K_SHIFT and one["trace"][n, 7] == 1000.0 + one["status"][0]
    assert (one["trace"][:n, 1] > 0).all() and not one["trace"][n + 1:ROWS].any()
    for order in (0, 1):
        o = _np(_handle(True, len(inst), order).solve(batch, trace_instance=j, trace_cap=TRACE_CAP, duals=True))
        assert np.array_equal(o["trace"][:ROWS].view(np.uint64), one["trace"][:ROWS].view(np.uint64)), order
        for k, v in one.items():
            if k != "trace":
                mine = np.ascontiguousarray(o[k][..., j:j + 1])
                assert mine.dtype == v.dtype and np.array_equal(mine.view(np.uint8), v.view(np.uint8)), (order, k)
