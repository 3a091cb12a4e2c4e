"""The line search with its modes at compile time and the filter's overflow entries loaded once per line search
(mr_wave.h line_search<RESTO, SOCDIR, MODE>) takes the same decisions as the untouched scalar solver
(mr_solver.h Solver): the emulated wave against the scalar build, fp64, at the C4 options of
test_host_twin.py::test_second_order_corrections_wave_matches_scalar.  The trace's marker column (7) must be
equal exactly, columns 0..6 (kkt, mu, alpha, delta, theta, phi, ...) to rtol 1e-6 / atol 1e-12.

Worst error of the build before the restructure, as a fraction of that tolerance: case 1 0.018, case 2 0.074,
case 3 0.0012."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import host_twin as ht
from mpcracing import abi, workload as wl

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _traces(i, max_iter):
    """(scalar trace, wave trace) of C4 instance i over its iterations."""
    cfg = wl.CONFIGS["C4"]
    b = wl.make_batch("C4", limit=i + 1)
    sub = {k: (v[..., i:i + 1].copy() if v is not None else None) for k, v in b.items()}
    c = ht.config(cfg["N"], cfg["model"], "fp64", cfg["lane"], cfg["Ts"], tol=1e-4, acceptable_iter=15,
                  acceptable_tol=1e-2, max_iter=max_iter)
    a = ht.solve(c, sub, nthreads=1, scalar=True, trace_instance=0, trace_cap=max_iter + 50)
    w = ht.solve(c, sub, nthreads=1, scalar=False, trace_instance=0, trace_cap=max_iter + 50)
    n = int(a["iters"][0])
    assert int(w["iters"][0]) == n and int(w["status"][0]) == int(a["status"][0])
    return a["trace"][:n], w["trace"][:n]


def _check(ta, tw):
    np.testing.assert_array_equal(ta[:, 7], tw[:, 7])
    np.testing.assert_allclose(tw[:, :7], ta[:, :7], rtol=1e-6, atol=1e-12)


def test_long_backtracks_then_watchdog_step():
    """Instance 312, 80 iterations: backtracks of 5-11 halvings at iterations 66-72 (the resumed backtracking,
    LS_NOSOC: no capture code), then a watchdog step (marker -101 at iteration 73; LS_WD).  Beyond about 86
    iterations this instance exceeds 1e-6 before the restructure too."""
    ta, tw = _traces(312, 80)
    m = ta[:, 7]
    assert m[73] == -101
    assert ((m[66:73] % 100 >= 5) & (m[66:73] % 100 <= 11)).all(), m[66:73]
    _check(ta, tw)


def test_accepted_corrections_and_shortened_steps():
    """Instance 3049, 150 iterations: 31 accepted second-order corrections (marker >= 100; the SOC trial,
    LS_WD | LS_CAP along the SOC direction) and 56 shortened steps (a marker with backtracks)."""
    ta, tw = _traces(3049, 150)
    m = ta[:, 7]
    assert (m >= 100).sum() == 31
    assert ((m > 0) & (m < 100)).sum() == 56
    _check(ta, tw)


_CHILD = r"""
import json, sys
sys.path[:0] = [{repo!r}, {repo!r} + "/mpc-racing_amd", {repo!r} + "/tests"]
import numpy as np
import test_ls_restructure as t
ta, tw = t._traces(4765, 150)
t._check(ta, tw)
print(json.dumps({{"iters": len(ta), "soc": int((ta[:, 7] >= 100).sum())}}))
"""


@pytest.mark.slow
def test_filter_overflow_path(tmp_path):
    """Instance 4765, 150 iterations, on a host build with -DMR_FMAX=2: the filter's LDS bank holds two entries,
    so from the third entry on every acceptance test runs on the overflow entries (held in registers for the
    line search).  The variant is built into tmp_path with build.py's g++ line and run in a child process
    (MR_HOST_TWIN_LIB)."""
    lib = str(tmp_path / "libmpcracing_host_fmax2.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-fopenmp", "-DMR_FMAX=2",
                    "-o", lib, os.path.join(abi.CSRC, "mpcracing_host.cpp")], check=True)
    env = dict(os.environ, MR_HOST_TWIN_LIB=lib)
    r = subprocess.run([sys.executable, "-c", _CHILD.format(repo=REPO)], env=env, check=True, capture_output=True,
                       text=True)
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["iters"] > 2 and res["soc"] >= 5  # (more than two filter entries: the overflow path is exercised)
