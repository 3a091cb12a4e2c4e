"""Time the tyre fit (mr_tyre_fit): R = 1 and R = 1024 training runs on the GPU, and the host build of the
same source on 16 threads.  Writes profiles/tyrefit_bench.json.  No pass / fail bar.

The setup is the reference's (learning/train.py): Pacejka tyres, Adam, lr 1e-3, 25 epochs, minibatches of
64, factor 0.5, patience 2.  Rows: --train / --val csv files in the reference's column layout, or by
default the 200 fixture rows of tests/golden/tyrefit_golden.npz tiled to --rows (the fit's cost depends on
the number of rows, not on their values).  GPU times are host clocks around calls that end in a device
synchronise, after a warm-up call of the same shape; the median of --repeat calls is reported with the
spread.  The CPU leg runs --cpu-runs runs (one emulated wavefront per run, 16 OpenMP threads).

Usage: python mpc-racing_amd/tools/tyrefit_bench.py [--rows 6405] [--repeat 5]
"""
import argparse
import datetime
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(REPO, "mpc-racing_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train")
    ap.add_argument("--val")
    ap.add_argument("--rows", type=int, default=6405)  # the reference's largest training set
    ap.add_argument("--epochs", type=int, default=25)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--runs", type=int, default=1024)
    ap.add_argument("--cpu-runs", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tyrefit_bench.json"))
    a = ap.parse_args()
    import torch
    from mpcracing import abi
    from mpcracing import tyrefit as tf
    if not torch.cuda.is_available():
        raise SystemExit("tyrefit_bench.py needs the GPU (no fallback: a CPU time says nothing about it)")
    if a.train:
        train, val = tf.load_rows(a.train), tf.load_rows(a.val or a.train)
    else:
        rows = np.load(os.path.join(REPO, "tests", "golden", "tyrefit_golden.npz"))["rows"]
        train = np.tile(rows, (-(-a.rows // len(rows)), 1))[:a.rows]
        val = train[:max(1, a.rows // 6)]
    n = len(train)
    steps = a.epochs * (-(-n // 64))
    res = {"date": datetime.date.today().isoformat(), "binary": os.path.relpath(abi.PRODUCT_LIB, REPO),
           "device": torch.cuda.get_device_name(0), "n_train": n, "n_val": len(val), "epochs": a.epochs,
           "steps_per_run": steps, "kind": "pacejka", "optimizer": "adam", "lr": 1e-3, "repeat": a.repeat}

    def gpu(R):
        perm = tf.make_perm(1337, a.epochs, n)  # shared shuffle: the runs differ in lr (as a sweep would)
        kw = dict(kind="pacejka", runs=R, lr=1e-3 * (1 + np.arange(R) % 8), epochs=a.epochs, perm=perm)
        tf.fit_tyres(train, val, **kw)  # warm-up of this shape
        ts = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            r = tf.fit_tyres(train, val, **kw)  # ends in torch.cuda.synchronize
            ts.append(time.perf_counter() - t0)
        assert (r.flag == 0).all()
        return {"runs": R, "median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)),
                "includes": "host-to-device copies of rows / perm, the perm check, the fit kernel, copies back",
                "us_per_step": float(np.median(ts)) / steps * 1e6}
    res["gpu_R1"], res["gpu_R"] = gpu(1), gpu(a.runs)
    res["ratio_R_over_R1"] = res["gpu_R"]["median_s"] / res["gpu_R1"]["median_s"]
    res["runs_per_s_gpu"] = a.runs / res["gpu_R"]["median_s"]
    perm = tf.make_perm(1337, a.epochs, n)
    t0 = time.perf_counter()
    tf.fit_tyres(train, val, kind="pacejka", runs=a.cpu_runs, lr=1e-3, epochs=a.epochs, perm=perm, host_twin=True)
    dt = time.perf_counter() - t0
    res["cpu_host_build_16_threads"] = {"runs": a.cpu_runs, "seconds": dt, "runs_per_s": a.cpu_runs / dt,
                                        "note": "emulated wavefront (64 fibers per run): a test harness, not a tuned CPU code"}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
