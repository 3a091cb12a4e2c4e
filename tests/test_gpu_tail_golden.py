"""The line search's restructure (compile-time modes, filter overflow entries loaded once per line search) changes
no arithmetic: every output of three small solves stays bitwise equal to the recording made with the library of
the commit before it (tests/golden/tail_parent.npz, generator tests/golden/make_tail_golden.py).

C4 fp32: the shard's long solves (second-order corrections, backtracking resumed down to alpha_min, watchdog steps,
a filter beyond its LDS entries) plus instances 0..55; C5 fp32 (N = 60); C3 fp64 (lane rows, the restoration
phase's line search)."""
import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_tail_golden", os.path.join(GOLDEN, "make_tail_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "tail_parent.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case", ["C4", "C5", "C3"])
def test_outputs_bitwise_equal_to_parent(case, golden):
    gen = _generator()
    idx, out = gen.solve_case(case)
    assert np.array_equal(idx, golden[f"{case}/idx"])
    keys = sorted(k.split("/", 1)[1] for k in golden if k.startswith(case + "/") and not k.endswith("/idx"))
    assert keys == sorted(out) and len(keys) == 10
    for k in keys:
        g = golden[f"{case}/{k}"]
        assert out[k].dtype == g.dtype and out[k].shape == g.shape, k
        # bitwise: NaNs (none expected) would have to match too
        assert np.array_equal(out[k].view(np.uint8), g.view(np.uint8)), (
            k, np.nonzero(np.any((out[k] != g).reshape(-1, len(idx)), axis=0))[0][:16])
