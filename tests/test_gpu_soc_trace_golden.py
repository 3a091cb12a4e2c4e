"""The lean second-order correction (mr_wave.h: soc_backward's constants staged in LDS, the forward recursion on
two lane groups, the dual side of the direction finished by soc_commit) changes no arithmetic: the full iteration
trace, every output array and lam_g of six single-instance solves stay bitwise equal to the recording made with
the library of the commit before it (tests/golden/soc_trace_parent.npz, generator
tests/golden/make_soc_trace_golden.py).  The trace pins the dual step size and the dual steps of an accepted
correction in the iteration they are taken, not only through the final outputs."""
import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_soc_trace_golden",
                                                  os.path.join(GOLDEN, "make_soc_trace_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _generator()


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "soc_trace_parent.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case", list(GEN.CASES))
def test_trace_and_outputs_bitwise_equal_to_parent(case, golden):
    out = GEN.solve_case(case)
    keys = sorted(k.split("/", 1)[1] for k in golden if k.startswith(case + "/"))
    assert keys == sorted(out) and "trace" in keys and "lam_g" in keys and len(keys) == 12
    if case in GEN.C3_MIN_ACCEPTED:
        assert GEN.accepted_corrections(out) >= GEN.C3_MIN_ACCEPTED[case]
    tr, gt = out["trace"], golden[f"{case}/trace"]
    assert tr.shape == gt.shape == (GEN.TRACE_CAP, 8)
    rows = np.nonzero(np.any(tr.view(np.uint64) != gt.view(np.uint64), axis=1))[0]
    assert rows.size == 0, ("first differing trace rows", rows[:8], tr[rows[:2]], gt[rows[:2]])
    for k in keys:
        g = golden[f"{case}/{k}"]
        assert out[k].dtype == g.dtype and out[k].shape == g.shape, k
        assert np.array_equal(out[k].view(np.uint8), g.view(np.uint8)), k
