"""Time the gain-tuning GA's two forms on the shape of pid_drive_bench.py's evaluate_gains run: 256 individuals x 20
segments = 5 120 vehicles, 240 ticks, Shanghai, the blended plant.  Writes profiles/pid_tune_bench.json.  No pass /
fail bar.

(a) One generation's fitness: pid.segment_times (one mr_pid_segment_times launch, times and ticks_done back)
    against pid.evaluate_gains at the same arguments (one mr_pid_drive launch that keeps the progress row, the row
    back, the crossing times in a Python loop over the vehicles).
(b) Ten generations: pid.tune_gains (4 islands x 64 individuals, 4 pairs; 20 launches on one stream, one
    synchronise) against the same ten generations as a host loop of pid.evaluate_gains + ga.breed.

Both sides of a pair run in the same session; times are host clocks around whole calls, each ending in a device
synchronise, the median of --repeat calls after a warm-up call.  ticks_share is the mean of ticks_done / ticks: the
share of the ticks that the early exit leaves to drive; wave_ticks_share is the same with every wavefront counted
to its slowest lane, which is what the device runs.

The segment bounds run from 10 m to 600 m before the end of the lap: no vehicle comes within the +-2 m window of
the start line, neither while it is timed nor in the ticks evaluate_gains drives on after the crossing (240 ticks
are at most 12 s).  Otherwise the reference's rule sends such a vehicle to the global projection, which costs 57
ms a tick and would decide both sides of the comparison.

Usage: python mpc-racing_amd/tools/pid_tune_bench.py
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


def timed(fn, repeat):
    out, ts = None, []
    for k in range(repeat + 1):  # the first call is the warm-up
        t0 = time.perf_counter()
        out = fn()
        if k:
            ts.append(time.perf_counter() - t0)
    return out, {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts))}


def wave_share(done, T):
    """The share of the ticks that the wavefronts run: a wave ends with its slowest lane, and lane j of the launch
    drives gains row j % G on segment j // G (pid_segment_kernel), so the 64 lanes of a wave share a segment."""
    G, K = done.shape
    lanes = done.T.reshape(-1)  # lane order: segment by segment
    return float(np.mean([lanes[w:w + 64].max() for w in range(0, G * K, 64)]) / T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--islands", type=int, default=4)
    ap.add_argument("--population", type=int, default=64)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--segments", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=240)
    ap.add_argument("--generations", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pid_tune_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pid_tune_bench.py needs the GPU (no fallback: a CPU time says nothing about it)")
    from mpcracing import ga, pid
    from mpcracing.geometry import DeviceTrack
    track = DeviceTrack("shanghai_intl_circuit")
    dev = track.device
    I, P, K, T, G = a.islands, a.population, a.segments, a.ticks, a.generations
    default4 = np.array(pid.GAIN_DEFAULTS[2:6])
    rng = np.random.default_rng(5)
    pop = default4 * (1 + 0.2 * rng.uniform(-1, 1, (I * P, 4)))
    lo, hi = 0.5 * default4, 1.5 * default4
    bounds = np.linspace(10.0, track.length - 600.0, K + 1)

    def sync(x):
        torch.cuda.synchronize(dev)
        return x

    # (a) one generation's fitness
    (t_fused, done), fused = timed(lambda: sync(pid.segment_times(track, pop, bounds, T)), a.repeat)
    (t_log, _), logged = timed(lambda: sync(pid.evaluate_gains(track, pop, bounds, T)), a.repeat)

    # (b) ten generations
    def host_loop():
        genes, avg = pop.reshape(I, P, 4), np.full((I, K), T * 0.05 / 2)
        for g in range(G):
            t, _ = pid.evaluate_gains(track, genes.reshape(I * P, 4), bounds, T)
            out = ga.breed(genes, t.reshape(I, P, K), avg, pairs=a.pairs, lo=lo, hi=hi, seed=5, generation=g)
            genes, avg = out.genes, out.avg
        return sync(genes)

    def device_loop():
        return sync(pid.tune_gains(track, bounds, G, islands=I, population=P, pairs=a.pairs, seed=5,
                                   init=pop.reshape(I, P, 4), lo=lo, hi=hi, ticks=T))

    res_dev, tuned = timed(device_loop, a.repeat)
    genes_host, looped = timed(host_loop, a.repeat)
    res = {"date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0),
           "track": "shanghai_intl_circuit", "model": "blend", "individuals": I * P, "islands": I, "segments": K,
           "vehicles": I * P * K, "ticks": T, "repeat": a.repeat,
           "bounds": "linspace(10, L - 600, segments + 1): no vehicle comes within the +-2 m projection window of the "
                     "start line on either side of a comparison (the global projection there costs 57 ms a tick and "
                     "would decide both sides)",
           "includes": "whole calls on a host clock, host-to-device copies and results back included, each ending in "
                       "a device synchronise; the median after one warm-up call",
           "fitness": {"segment_times": fused, "evaluate_gains": logged,
                       "speedup": logged["median_s"] / fused["median_s"],
                       "times_equal_bitwise": bool(np.array_equal(t_fused, t_log)),
                       "segments_finished": int(np.isfinite(t_fused).sum()),
                       "ticks_share": float(np.mean(done / T)), "wave_ticks_share": wave_share(done, T)},
           "generations": {"count": G, "pairs": a.pairs, "tune_gains": tuned, "host_loop": looped,
                           "speedup": looped["median_s"] / tuned["median_s"],
                           "launches": 2 * G,
                           "populations_equal_bitwise": bool(np.array_equal(res_dev.population, genes_host)),
                           "ticks_share_last_generation": float(np.mean(res_dev.ticks_done / T)),
                           "best_reward_first_last": [res_dev.best_reward[0].tolist(),
                                                      res_dev.best_reward[-1].tolist()]}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
