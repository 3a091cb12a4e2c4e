"""The gfx950 wave primitives (csrc/mr_wave_prims.h, device branch) against the numpy restatement
(tests/wave_prims_ref.py) and against the host fibre emulation that every CPU solver test runs on.

The probe (csrc/mr_probe.hip, the product's compiler flags) launches three 64-lane workgroups with
different data, as mr_wave_kernel is launched, so a result cannot leak between blocks unnoticed.
DPP rotates, readlane broadcasts, the permlane swaps of the butterfly and of wtranspose4, the buffer
accessors and pick6 are compared bit for bit; wsum / wmax / wmin bit for bit with the restated butterfly
and with the emulation, on all 64 lanes; the MFMA lane maps with identity-pattern matrices, exactly on
integer-valued ones, f32 bit for bit with a k-ordered fmaf chain, f64 within 4 eps (|C| + |A| |B|).

Measured on an MI355X (profiles/f32_accuracy.json "wave_prims"): every move and reduction bit-identical to the
restatement and to the emulation; with one NaN, wmax / wmin give NaN on 1 of 64 lanes (not lane-uniform), as the
restated butterfly does; the f64 MFMA was bitwise equal to the emulation as well, at most 0.24 of the bound away
from the exact product.
"""
import json
import os

import numpy as np
import pytest

import wave_prims_cases as wc
import wave_prims_ref as R

pytestmark = pytest.mark.gpu

CASES = [("f32", False), ("f64", False), ("i32", False), ("f32", True), ("f64", True)]  # (type, one NaN per workgroup)


@pytest.mark.parametrize("kind,nan", CASES)
def test_device_prims_match_restatement_and_host(kind, nan):
    x = wc.prims_inputs(kind, nan)
    dev = wc.device_prims(x)
    wc.check_prims(dev, x, "device")
    host = wc.host_prims(x)
    _, have = R.prims_expected(x[0], 0)
    for g in range(3):
        for s in np.flatnonzero(have):
            if nan and s == R.SLOT["sum"]:
                continue  # NaN on every lane on both sides (check_prims); the payload of a computed NaN is not pinned
            assert (R.bits(dev[g, s]) == R.bits(host[g, s])).all(), (kind, g, int(s))


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_wmax_with_one_nan_follows_the_butterfly(kind):
    """b > a ? b : a keeps a NaN only on the lanes whose own value it is at some level: the result is not
    lane-uniform, and the device gives lane by lane what the restated butterfly gives."""
    x = wc.prims_inputs(kind, True)
    dev = wc.device_prims(x)
    for g in range(3):
        for name, op in (("max", R.op_max), ("min", R.op_min)):
            exp = R.butterfly(x[g, 0], op)
            assert (R.bits(dev[g, R.SLOT[name]]) == R.bits(exp)).all(), (kind, g, name)
            print(kind, "workgroup", g, "w" + name, "with one NaN: NaN on", int(np.isnan(exp).sum()), "of 64 lanes")


def test_device_mfma_f32_is_the_fma_chain():
    A, B, C = wc.mfma_inputs("f32")
    D = wc.device_mfma(A, B, C)
    wc.check_mfma(D, A, B, C, "device")
    exp = wc.fma_chain_expected(A, B, C)
    assert (R.bits(D) == R.bits(exp)).all(), np.argwhere(R.bits(D) != R.bits(exp))[:8].tolist()
    assert (R.bits(D) == R.bits(wc.host_mfma(A, B, C))).all()


def test_device_mfma_f64():
    A, B, C = wc.mfma_inputs("f64")
    D = wc.device_mfma(A, B, C)
    res = wc.check_mfma(D, A, B, C, "device")
    H = wc.host_mfma(A, B, C)
    res["bitwise_equal_to_host_emulation"] = bool((R.bits(D) == R.bits(H)).all())
    res["max_abs_diff_to_host_emulation"] = float(np.abs(D - H).max())
    print("f64 MFMA:", json.dumps(res))
    out = os.environ.get("MR_F32_ACCURACY_OUT")
    if out:
        with open(os.path.join(out, "wave_mfma_f64.json"), "w") as f:
            json.dump(res, f)
