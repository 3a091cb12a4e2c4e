"""Scalar-against-wave census of the host builds on C3 where the inertia shift is large (CPU only).

Two figures, printed as one JSON object (profiles/shift_accuracy.json keeps them before and after the symmetric
cost-to-go tile of mr_wave.h):
  whole     iterations and status of the whole fp64 solves (tol 1e-8, acceptable 1e-6 over 15, max_iter 500) of the
            instances of tests/golden/make_shift_golden.py, scalar Solver against the emulated wave
  rows      over C3 instances 0..95, the share whose step length alpha of iterations 0..5 differs between the two
            builds by more than 1e-6 relative, and the largest difference (with the instance)

Usage: python mpc-racing_amd/tools/shift_census.py [--lib libmpcracing_host.so]     (about a minute, 16 processes)
"""
import argparse
import json
import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(REPO, "mpc-racing_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

WHOLE = (79, 67, 62, 57, 33, 2754, 6258, 3734, 5287, 6101, 7151, 3022)
OPT = dict(tol=1e-8, acceptable_tol=1e-6, acceptable_iter=15)
_b = {}


def _sub(i):
    from mpcracing import workload as wl
    if "b" not in _b:
        _b["b"] = wl.make_batch("C3", limit=max(WHOLE) + 1)
    return {k: (np.ascontiguousarray(v[..., i:i + 1]) if v is not None else None) for k, v in _b["b"].items()}


def _pair(arg):
    import host_twin as ht
    from mpcracing import workload as wl
    i, max_iter = arg
    cfg = wl.CONFIGS["C3"]
    c = ht.config(cfg["N"], cfg["model"], "fp64", cfg["lane"], cfg["Ts"], max_iter=max_iter, **OPT)
    return i, [ht.solve(c, _sub(i), nthreads=1, scalar=s, trace_instance=0, trace_cap=max_iter + 8) for s in (True, False)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another host build of the source (MR_HOST_TWIN_LIB)")
    a = ap.parse_args()
    if a.lib:
        os.environ["MR_HOST_TWIN_LIB"] = os.path.abspath(a.lib)
    with Pool(16) as pool:
        whole = pool.map(_pair, [(i, 500) for i in WHOLE], chunksize=1)
        rows = pool.map(_pair, [(i, 6) for i in range(96)], chunksize=1)
    out = dict(whole={}, rows={})
    for i, (s, w) in whole:
        out["whole"][str(i)] = dict(scalar=[int(s["iters"][0]), int(s["status"][0])],
                                    wave=[int(w["iters"][0]), int(w["status"][0])])
    worst, n_over = (0.0, -1), 0
    for i, (s, w) in rows:
        a_s, a_w = s["trace"][:6, 2], w["trace"][:6, 2]
        d = float(np.max(np.abs(a_w - a_s) / np.abs(a_s)))
        n_over += d > 1e-6
        worst = max(worst, (d, i))
    out["rows"] = dict(instances=96, over_1e_6=int(n_over), share=n_over / 96.0, worst=worst[0], worst_instance=worst[1])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
