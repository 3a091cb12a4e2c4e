"""Developer tool: what the primal warm start does to a batched closed loop on the GPU.

  python mpc-racing_amd/tools/warm_start_bench.py [--B 4096] [--ticks 40] [--pairs 3] [--out FILE]
                                                  [--only cold|warm]

The configuration of tools/closed_loop_bench.py (B vehicles spread along Shanghai, dynamic-model MPC, N = 15, blended
plant, control from tick 1, dispatch by the previous tick's iterations) at the reference's IPOPT options (tol 1e-4,
acceptable_tol 1e-2 over 15, control/MPC.py:152-161), in fp64 and fp32.  Per precision, ``pairs`` times in one
process: the loop without warm start (ClosedLoop's default, the baseline), then ClosedLoop(warm_start="primal"),
alternating, each from the same start states.  Two ticks run before the timed window (the global projections of
tick 0 and the first controlled tick, which is cold in both loops); every timed tick lies between two device events
on the loop's stream and nothing synchronises inside the window.

Writes profiles/warm_start_bench.json: per precision and variant, per timed tick the mean and max iterations, the
status histogram and the ms per tick (the median over the pairs; iterations and statuses are the same in every pair),
the totals of every pair, and for the warm loop the share of vehicle ticks that started from the guess.
``--only`` runs one variant (for a kernel trace of its own, e.g. under rocprofv3 --kernel-trace --stats).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(REPO, "mpc-racing_amd"))
from mpcracing.closed_loop import ClosedLoop  # noqa: E402
from mpcracing.geometry import DeviceTrack  # noqa: E402

REFERENCE_OPTIONS = dict(tol=1e-4, acceptable_tol=1e-2, acceptable_iter=15)


def one_run(loop, x0, ticks):
    """(ms per tick [ticks], records) of ``ticks`` timed ticks after the two warm-up ticks."""
    loop.reset(x0)
    loop.run(2)
    torch.cuda.synchronize(loop.dev)
    st = torch.cuda.current_stream(loop.dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(ticks + 1)]
    recs = []
    ev[0].record(st)
    for k in range(ticks):
        recs.append(loop.tick(st))
        ev[k + 1].record(st)
    torch.cuda.synchronize(loop.dev)
    return np.array([ev[k].elapsed_time(ev[k + 1]) for k in range(ticks)]), recs


def summarise(runs, warm):
    ms = np.stack([m for m, _r in runs])  # [pairs][ticks]
    recs = runs[0][1]
    it = np.stack([r["iters"].cpu().numpy() for r in recs])
    stt = np.stack([r["status"].cpu().numpy() for r in recs])
    for _m, other in runs[1:]:  # the solves do not depend on the run
        assert all(torch.equal(a["iters"], b["iters"]) and torch.equal(a["status"], b["status"])
                   for a, b in zip(recs, other))
    out = {"per_tick": {"iters_mean": it.mean(axis=1).tolist(), "iters_max": it.max(axis=1).tolist(),
                        "status_hist": [np.bincount(s, minlength=5).tolist() for s in stt],
                        "ms": np.median(ms, axis=0).tolist()},
           "pairs_total_ms": ms.sum(axis=1).tolist(), "total_ms_median": float(np.median(ms.sum(axis=1))),
           "ms_per_tick_median": float(np.median(ms)), "ms_per_tick_max": float(np.median(ms, axis=0).max()),
           "iters_mean": float(it.mean()), "iters_max": int(it.max()),
           "status_hist": np.bincount(stt.ravel(), minlength=5).tolist(),
           "instances_at_max_iter_per_tick": (it >= 500).sum(axis=1).tolist(),
           "abs_error_p50": float(np.median(np.abs(recs[-1]["error"].cpu().numpy()))),
           "abs_error_max": float(np.abs(recs[-1]["error"].cpu().numpy()).max())}
    if warm:
        used = np.stack([r["warm_used"].cpu().numpy() for r in recs])
        out["warm_used_share"] = float(used.mean())
        out["per_tick"]["warm_used"] = used.sum(axis=1).tolist()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--only", choices=("cold", "warm"), default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "warm_start_bench.json"))
    a = ap.parse_args()
    tr = DeviceTrack("shanghai_intl_circuit")
    s0 = (np.arange(a.B) + 0.5) * tr.length / a.B
    x0 = ClosedLoop.start_states(tr, s0, v0=15.0)
    res = {"B": a.B, "ticks": a.ticks, "pairs": a.pairs, "N": 15, "options": REFERENCE_OPTIONS,
           "device": torch.cuda.get_device_name(0)}
    for prec in ("fp64", "fp32"):
        variants = {"cold": None, "warm": "primal"}
        if a.only:
            variants = {a.only: variants[a.only]}
        loops = {k: ClosedLoop(tr, B=a.B, N=15, plant="blend", precision=prec, start_control_at=1, warm_start=w,
                               **REFERENCE_OPTIONS) for k, w in variants.items()}
        runs = {k: [] for k in variants}
        for _pair in range(a.pairs):
            for k in variants:
                runs[k].append(one_run(loops[k], x0, a.ticks))
        res[prec] = {k: summarise(runs[k], k == "warm") for k in variants}
        if not a.only:
            res[prec]["speedup_total_median"] = res[prec]["cold"]["total_ms_median"] / res[prec]["warm"]["total_ms_median"]
        print(prec, json.dumps({k: {q: v[q] for q in ("total_ms_median", "pairs_total_ms", "ms_per_tick_median",
                                                      "ms_per_tick_max", "iters_mean", "iters_max", "status_hist")}
                                for k, v in res[prec].items() if isinstance(v, dict)}), flush=True)
        del loops
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
