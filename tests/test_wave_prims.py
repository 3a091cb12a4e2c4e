"""The host fibre emulation of the wave primitives (csrc/mr_wave_prims.h, `#else` branch) against a
numpy restatement written from the header's prose (tests/wave_prims_ref.py).

Every CPU solver test runs the kernel's SPMD source on this emulation, so its lane maps, its reduction
order and its MFMA chain are checked here directly: moves, WBuf and pick6 bit for bit (integer views),
reductions bit for bit against the restated six-level butterfly and against math.fsum within
6 eps sum|v|, the MFMA exactly on integer-valued matrices, within 4 eps (|C| + |A| |B|) on random ones and
(f32) bit for bit against a k-ordered fma chain.  tests/test_gpu_wave_prims.py holds the device to the
same restatement and to this emulation.
"""
import numpy as np
import pytest

import wave_prims_cases as wc
import wave_prims_ref as R


CASES = [("f32", False), ("f64", False), ("i32", False), ("f32", True), ("f64", True)]  # (type, one NaN per workgroup)


@pytest.mark.parametrize("kind,nan", CASES)
def test_host_prims_match_restatement(kind, nan):
    x = wc.prims_inputs(kind, nan)
    wc.check_prims(wc.host_prims(x), x, "host")


def test_inputs_exercise_association():
    """The sum inputs would catch a different association: the restated butterfly and a left-to-right sum differ."""
    for kind in ("f32", "f64"):
        v = wc.prims_inputs(kind)[1, 0]
        seq = v.dtype.type(0)
        for t in v:
            seq = v.dtype.type(seq + t)
        assert R.butterfly(v, R.op_sum)[0] != seq


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_host_mfma(kind):
    A, B, C = wc.mfma_inputs(kind)
    D = wc.host_mfma(A, B, C)
    wc.check_mfma(D, A, B, C, "host")
    if kind == "f32":
        exp = wc.fma_chain_expected(A, B, C)
        assert (R.bits(D) == R.bits(exp)).all(), np.argwhere(R.bits(D) != R.bits(exp))[:8].tolist()


def test_restated_fma_is_single_rounding():
    """fma32 differs from multiply-then-add where the product's low bits matter."""
    a, b, c = np.float32(1 + 2 ** -12), np.float32(1 + 2 ** -12), np.float32(-1)
    assert float(R.fma32(a, b, c)) == 2 ** -11 + 2 ** -24
    assert float(np.float32(a * b) + c) != 2 ** -11 + 2 ** -24
