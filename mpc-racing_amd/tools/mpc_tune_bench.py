"""Time the MPC's segment drives on the reference GA's sizes (GA/mpcGA.py:7-10: 100 individuals x 5 checkpoints =
500 vehicles), N = 15, 240 ticks, fp64, Shanghai, the blended plant.  Writes profiles/mpc_tune_bench.json.

(a) ga.evaluate_population (ClosedLoop: every vehicle solved on every tick, torch glue between the launches, the
    crossing times on the host) against mpc.segment_times at the same arguments (library launches only, a finished
    vehicle neither solved nor stepped), and mpc.segment_times with poll_every=16 (the loop ends once every vehicle
    has finished).  The three alternate in one process.
(b) One generation of mpc.tune_weights on the same vehicles (runtime vectors from genes, reset, drive, breeding).

Times are host clocks around whole calls, set-up and results back included, each ending in a device synchronise:
the median of --repeat rounds after a warm-up round.  skipped_solves_share: the share of the (vehicle, tick)
solves of evaluate_population that segment_times leaves out.  The only bar: segment_times is not slower than
evaluate_population (exit status 1 otherwise).

The five segments are 100 m each from 100 m on: from 15 m/s a vehicle covers one in roughly half of the 12 s, and
none comes near the start line's +-2 m window, where the reference's rule projects globally.

Usage: python mpc-racing_amd/tools/mpc_tune_bench.py
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


def stats(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--population", type=int, default=100)
    ap.add_argument("--segments", type=int, default=5)
    ap.add_argument("--segment-length", type=float, default=100.0)
    ap.add_argument("--ticks", type=int, default=240)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--poll-every", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mpc_tune_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mpc_tune_bench.py needs the GPU (no fallback: a CPU time says nothing about it)")
    from mpcracing import ga, mpc
    from mpcracing.geometry import DeviceTrack
    track = DeviceTrack("shanghai_intl_circuit")
    P, K, T, N = a.population, a.segments, a.ticks, 15
    rng = np.random.default_rng(7)
    genes = rng.uniform(0, 1, (P, 5))
    default = np.array(mpc.RUNTIME_DEFAULTS)
    lo, hi = 0.5 * default, 1.5 * default
    pop = lo + genes * (hi - lo)
    bounds = 100.0 + a.segment_length * np.arange(K + 1)
    names = ["alpha_c", "q_v_y", "n", "beta_delta"]
    cols = [mpc.RUNTIME_FIELDS.index(k) for k in names]
    ranges = {k: (lo[c], hi[c]) for k, c in zip(names, cols)}
    runs = {
        "evaluate_population": lambda: ga.evaluate_population(track, pop, bounds, T, N=N)[0],
        "segment_times": lambda: mpc.segment_times(track, pop, bounds, T, N=N),
        "segment_times_poll": lambda: mpc.segment_times(track, pop, bounds, T, N=N, poll_every=a.poll_every),
        # two islands: mr_ga_breed takes at most 64 individuals per island
        "tune_weights_generation": lambda: mpc.tune_weights(track, bounds, 1, ranges, islands=2, population=P // 2,
                                                            pairs=P // 8, genes=names,
                                                            init=genes[:P // 2 * 2, cols].reshape(2, P // 2, 4),
                                                            ticks=T, N=N),
    }
    ts, out = {k: [] for k in runs}, {}
    for r in range(a.repeat + 1):  # round 0 is the warm-up; the variants alternate within a round
        for k, fn in runs.items():
            t0 = time.perf_counter()
            out[k] = fn()
            torch.cuda.synchronize(track.device)
            if r:
                ts[k].append(time.perf_counter() - t0)
            print(r, k, f"{time.perf_counter() - t0:.3f} s", flush=True)
    t_ref = out["evaluate_population"]
    t_seg, done, _ = out["segment_times"]
    t_poll, done_poll, _ = out["segment_times_poll"]
    # a vehicle that finishes at tick k (ticks_done = k + 1) was solved on ticks 1 .. k - 1; one that does not, on
    # ticks 1 .. T - 1, as every vehicle of evaluate_population
    finished = np.isfinite(t_seg) | (done < T)
    solved = np.where(finished, np.maximum(done - 2, 0), T - 1)
    med = {k: stats(v) for k, v in ts.items()}
    res = {"date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0),
           "track": "shanghai_intl_circuit", "plant": "blend", "mpc_model": "dyn", "precision": "fp64", "N": N,
           "individuals": P, "segments": K, "vehicles": P * K, "ticks": T, "repeat": a.repeat,
           "bounds": bounds.tolist(),
           "includes": "whole calls on a host clock (solver and buffers created, results back), each ending in a "
                       "device synchronise; the variants alternate within a round; the median after one warm-up round",
           "timing": med,
           "speedup_segment_times": med["evaluate_population"]["median_s"] / med["segment_times"]["median_s"],
           "speedup_segment_times_poll": med["evaluate_population"]["median_s"] / med["segment_times_poll"]["median_s"],
           "poll_every": a.poll_every,
           "library_calls_per_tick": {"segment_times": 4, "segment_times_primal": 5,
                                      "note": "mr_agent_sense, mr_mpcseg_inputs, (mr_warm_shift,) the solve, "
                                              "mr_mpcseg_apply; the solve call enqueues its dispatch-order kernels "
                                              "and the wave kernel; no torch op between them"},
           "times_equal_bitwise": bool(np.array_equal(t_seg, t_ref)),
           "times_equal_bitwise_poll": bool(np.array_equal(t_poll, t_ref)),
           "segments_finished": int(np.isfinite(t_seg).sum()),
           "ticks_share": float(np.mean(done / T)),
           "skipped_solves_share": float(1.0 - solved.sum() / (P * K * (T - 1))),
           "last_finish_tick": int(done[np.isfinite(t_seg)].max()) if np.isfinite(t_seg).any() else None,
           "tune_weights_best_reward": out["tune_weights_generation"].best_reward.tolist()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
    if med["segment_times"]["median_s"] > med["evaluate_population"]["median_s"]:
        raise SystemExit("segment_times is slower than evaluate_population")


if __name__ == "__main__":
    main()
