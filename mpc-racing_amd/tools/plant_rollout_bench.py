"""Time the plant rollouts (mr_plant_rollout): 1 024 parameter sets x every start row of a log of 6 405 rows x
H = 40 on the GPU for each of the three plant models, and one plantfit.identify run.  Writes
profiles/plant_rollout_bench.json.  No pass / fail bar.

Log, starts, H and the number of sets are those of tools/rollout_bench.py (the fixture log of
tests/golden/rollout_golden.npz tiled to --rows, or --log steps.csv), so the two records are comparable.
Parameter sets: the defaults with Cf, Cr, m and Iz of each set perturbed by 1 %.  GPU times are host clocks
around library calls on device-resident arrays (each call checks the starts, allocates its partials, launches
and synchronises), after a warm-up call of the same shape; the median of --repeat calls is reported with the
spread.  The identify run searches (Cf, Cr) of the dynamic model over --grid^2 sets per round for --rounds
rounds, through the Python interface (its arrays travel to the device in every round).

Usage: python mpc-racing_amd/tools/plant_rollout_bench.py
"""
import argparse
import ctypes
import datetime
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(REPO, "mpc-racing_amd"))

MODELS = ["kin", "dyn", "blend"]


def make_work(a):
    from mpcracing import rollout as ro
    if a.log:
        log = ro.load_log(a.log)
    else:
        fix = np.load(os.path.join(REPO, "tests", "golden", "rollout_golden.npz"))["log"]
        log = np.tile(fix, (1, -(-a.rows // fix.shape[1])))[:, :a.rows]
    rng = np.random.default_rng(11)
    params = np.tile(ro.plant_params(), (a.sets, 1))
    for k in ("Cf", "Cr", "m", "Iz"):
        j = ro.PLANT_FIELDS.index(k)
        params[1:, j] *= 1 + 0.01 * rng.standard_normal(a.sets - 1)
    starts = np.arange(log.shape[1] - a.horizon, dtype=np.int32)
    return np.ascontiguousarray(log), params, starts


def time_gpu(a, model):
    """median / min / max seconds of mr_plant_rollout on device-resident arrays"""
    import torch
    from mpcracing import abi
    log, params, starts = make_work(a)
    lib = abi.load_product()
    dev = torch.device("cuda", 0)
    d = [torch.as_tensor(x).to(dev).contiguous() for x in (log, starts, params)]
    P, H, T, n = a.sets, a.horizon, log.shape[1], len(starts)
    stats = torch.empty((P, H, 6, 4), dtype=torch.float64, device=dev)
    count = torch.empty((P, H), dtype=torch.int32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call():
        rc = lib.mr_plant_rollout(abi.MR_PLANT[model], T, p(d[0]), n, p(d[1]), H, P, p(d[2]), None, p(stats), p(count),
                                  None, st)
        if rc != 0:
            raise RuntimeError(lib.mr_last_error().decode())
    call()  # warm-up of this shape
    torch.cuda.synchronize(dev)
    ts = []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        call()  # ends in a stream synchronise
        ts.append(time.perf_counter() - t0)
    c = count.cpu().numpy()
    steps = P * n * H
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)),
            "model_steps_per_s": steps / float(np.median(ts)), "count_min": int(c.min()), "count_max": int(c.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log")
    ap.add_argument("--rows", type=int, default=6405)  # as tools/rollout_bench.py
    ap.add_argument("--sets", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=40)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--grid", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "plant_rollout_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("plant_rollout_bench.py needs the GPU (no fallback: a CPU time says nothing about it)")
    from mpcracing import plantfit
    from mpcracing import rollout as ro
    log, _, starts = make_work(a)
    n = len(starts)
    res = {"date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "sets": a.sets,
           "T": log.shape[1], "n_start": n, "horizon": a.horizon, "waves": a.sets * (-(-n // 64)),
           "model_steps": a.sets * n * a.horizon, "repeat": a.repeat,
           "includes": "start check, partials allocation, rollout and finishing kernels, synchronise; arrays "
                       "already on the device",
           "gpu": {m: time_gpu(a, m) for m in MODELS}}
    free = {"Cf": (30000.0, 150000.0), "Cr": (30000.0, 150000.0)}
    plantfit.identify(log, "dyn", free, a.horizon, grid=a.grid, rounds=1)  # warm-up of the round's shape
    t0 = time.perf_counter()
    r = plantfit.identify(log, "dyn", free, a.horizon, grid=a.grid, rounds=a.rounds)
    dt = time.perf_counter() - t0
    res["identify"] = {"model": "dyn", "free": {k: list(v) for k, v in free.items()}, "grid": a.grid,
                       "rounds": a.rounds, "sets_per_round": a.grid ** 2, "rollouts": a.rounds * a.grid ** 2 * n,
                       "seconds": dt, "values": r.values, "cost": r.cost,
                       "cost_at_defaults": float(ro.plant_rollout_errors(log, "dyn", horizon=a.horizon)
                                                 .position_cost()[0]),
                       "best_cost_per_round": [h["best_cost"] for h in r.history],
                       "includes": "per round: host-to-device copies of the log and the sets, one mr_plant_rollout "
                                   "call, the statistics back"}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
