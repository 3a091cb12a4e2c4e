"""Shared by tests/test_shift.py and tests/test_gpu_shift.py: the committed log of the dense IPOPT oracle on C3
instances that accept a large inertia shift at once (tests/golden/shift_golden.npz / .json, generator
make_shift_golden.py), whose compared rows the scalar build alone selected.

The row check and its bars are tests/ipopt_trace_cases.py's, applied to this fixture: alpha, theta, kkt to 1e-6
relative, theta with 1e-10 absolute on top; mu and delta to 1e-12.
"""
import importlib.util
import os

import ipopt_trace_cases as itc

GOLDEN = itc.GOLDEN


def _generator():
    spec = importlib.util.spec_from_file_location("make_shift_golden", os.path.join(GOLDEN, "make_shift_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _generator()
TRACE_COL, LOG_COL = GEN.TRACE_COL, GEN.LOG_COL

_cache = {}


def fixture():
    """(arrays keyed "<case>/<name>", index keyed by case); loaded once and never modified."""
    if not _cache:
        arrays, index = GEN.load_fixture()
        for v in arrays.values():
            v.setflags(write=False)
        _cache["f"] = (arrays, index)
    return _cache["f"]


def cases(*kinds):
    return [c for c, s in GEN.CASES.items() if s["kind"] in kinds]


def check_rows(case, trace, label):
    return itc.check_rows(case, trace, label, fixture())
