"""Time the PID agent's drives: T = 400 ticks of n = 64, 4 096 and 65 536 vehicles on Shanghai with the blended
plant, (a) fused, one mr_pid_drive launch, with the full log and with only the progress row, and (b) step-wise,
T times mr_pid_control + mr_plant_step_params launched from Python.  One pid.evaluate_gains run (256 individuals
x 20 segments) and a probe of single ticks (tick_probe) go beside it.  Writes profiles/pid_drive_bench.json.  No pass / fail bar.

Vehicles start on the centerline at evenly spread progress with 15 m/s and the default gains and parameters
(shared: G = P = 1).  Times are host clocks around whole calls on device-resident arrays, ending in a device
synchronise, after a warm-up call of the same shape; the median of --repeat calls is reported with the spread.
State and memory are restored on the device before every call, outside the clock.  The step-wise form includes
what a Python loop needs between the two launches: the two small torch kernels that build the plant's command
(cmd_throttle - cmd_brake, cmd_steer) from the agent's output; it keeps no log.

Usage: python mpc-racing_amd/tools/pid_drive_bench.py
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


def stats(ts, n, T):
    med = float(np.median(ts))
    return {"median_s": med, "min_s": float(min(ts)), "max_s": float(max(ts)), "vehicle_ticks_per_s": n * T / med,
            "us_per_tick": 1e6 * med / T}


def bench_size(a, track, n):
    import torch
    from mpcracing import abi, pid
    from mpcracing import rollout as ro
    from mpcracing.closed_loop import ClosedLoop
    lib, dev, T, dt = track.lib, track.device, a.ticks, 0.05
    s0 = np.linspace(5.0, track.length - 5.0, n)
    x0 = torch.as_tensor(ClosedLoop.start_states(track, s0, v0=15.0)).to(dev).contiguous()
    mem0 = torch.zeros((4, n), dtype=torch.float64, device=dev)
    mem0[0] = torch.as_tensor(s0).to(dev)
    mem0[3] = float("nan")
    g = torch.as_tensor(pid.gains()[None]).to(dev).contiguous()
    q = torch.as_tensor(ro.plant_params()[None]).to(dev).contiguous()
    state, mem = x0.clone(), mem0.clone()
    done = torch.empty(n, dtype=torch.int32, device=dev)
    out = torch.empty((8, n), dtype=torch.float64, device=dev)
    cmd = torch.empty((2, n), dtype=torch.float64, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    model = abi.MR_PLANT["blend"]

    def check(rc):
        if rc != 0:
            raise RuntimeError(lib.mr_last_error().decode())

    def fused(mask, log):
        check(lib.mr_pid_drive(track.h, model, n, T, dt, p(state), p(mem), 1, p(g), 1, p(q), mask, p(log), p(done), st))

    def stepwise():
        for _ in range(T):
            check(lib.mr_pid_control(track.h, n, p(state), p(mem), 1, p(g), dt, p(out), st))
            torch.sub(out[2], out[4], out=cmd[0])
            cmd[1].copy_(out[3])
            check(lib.mr_plant_step_params(model, n, p(state), p(cmd), dt, 1, p(q), p(state), st))

    def timed(fn):
        ts = []
        for k in range(a.repeat + 1):  # the first call is the warm-up of this shape
            state.copy_(x0)
            mem.copy_(mem0)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            if k:
                ts.append(time.perf_counter() - t0)
        return stats(ts, n, T)

    res = {"n": n, "waves": -(-n // 64)}
    res["stepwise"] = timed(stepwise)
    final = state.clone()
    log1 = torch.empty((1, T, n), dtype=torch.float64, device=dev)
    res["fused_progress_only"] = timed(lambda: fused(1 << pid.LOG_ROWS.index("progress"), log1))
    res["fused_equals_stepwise_bitwise"] = bool(torch.equal(final, state))
    res["ticks_done_min"] = int(done.min())
    del log1
    log = torch.empty((abi.MR_PID_NLOG, T, n), dtype=torch.float64, device=dev)
    res["fused_full_log"] = timed(lambda: fused((1 << abi.MR_PID_NLOG) - 1, log))
    res["full_log_bytes"] = log.numel() * 8
    return res


def tick_probe(a, track):
    """What one tick costs and what it depends on: single mr_pid_control launches (median of 20 after a
    warm-up, each ended by a synchronise) for vehicles spread over the lap but away from the start line, the
    same with ONE vehicle whose +-2 m bounds straddle the start line (the reference's rule sends it to the
    global projection), and 64 vehicles spread over the lap against 64 within 2 m of each other."""
    import torch
    from mpcracing import pid
    from mpcracing.closed_loop import ClosedLoop
    lib, dev, L = track.lib, track.device, track.length
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    g = torch.as_tensor(pid.gains()[None]).to(dev).contiguous()

    def one(s0):
        n = len(s0)
        x = torch.as_tensor(ClosedLoop.start_states(track, s0, v0=15.0)).to(dev).contiguous()
        mem0 = torch.zeros((4, n), dtype=torch.float64, device=dev)
        mem0[0] = torch.as_tensor(s0).to(dev)
        mem0[3] = float("nan")
        mem, out = mem0.clone(), torch.empty((8, n), dtype=torch.float64, device=dev)
        ts = []
        for k in range(21):
            mem.copy_(mem0)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            if lib.mr_pid_control(track.h, n, p(x), p(mem), 1, p(g), 0.05, p(out), st) != 0:
                raise RuntimeError(lib.mr_last_error().decode())
            torch.cuda.synchronize(dev)
            if k:
                ts.append(time.perf_counter() - t0)
        return {"n": n, "median_us": 1e6 * float(np.median(ts)), "min_us": 1e6 * min(ts), "max_us": 1e6 * max(ts)}

    res = {}
    for n in (64, 4096, 65536):
        s0 = np.linspace(100.0, L - 100.0, n)
        res[f"spread_{n}"] = one(s0)
        s1 = s0.copy()
        s1[-1] = L - 1.0
        res[f"spread_{n}_one_at_start_line"] = one(s1)
    res["neighbours_64"] = one(np.linspace(700.0, 702.0, 64))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 4096, 65536])
    ap.add_argument("--ticks", type=int, default=400)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--individuals", type=int, default=256)
    ap.add_argument("--segments", type=int, default=20)
    ap.add_argument("--ga-ticks", type=int, default=240)
    ap.add_argument("--only-probe", action="store_true", help="write the tick probe alone")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pid_drive_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pid_drive_bench.py needs the GPU (no fallback: a CPU time says nothing about it)")
    from mpcracing import pid
    from mpcracing.geometry import DeviceTrack
    track = DeviceTrack("shanghai_intl_circuit")
    if a.only_probe:
        res = {"tick_probe": tick_probe(a, track)}
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res, indent=1))
        return
    res = {"date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0),
           "track": "shanghai_intl_circuit", "model": "blend", "ticks": a.ticks, "repeat": a.repeat,
           "includes": "whole calls on device-resident arrays up to a device synchronise; step-wise: per tick "
                       "mr_pid_control, two torch kernels for the command, mr_plant_step_params",
           "sizes": [bench_size(a, track, n) for n in a.sizes], "tick_probe": tick_probe(a, track)}
    rng = np.random.default_rng(5)
    pop = np.array([0.1, 0.1, 0.82954, 1.21341]) * (1 + 0.2 * rng.uniform(-1, 1, (a.individuals, 4)))
    bounds = np.linspace(0.0, track.length, a.segments + 1)
    pid.evaluate_gains(track, pop, bounds, a.ga_ticks)  # warm-up of the shape
    t0 = time.perf_counter()
    times, _ = pid.evaluate_gains(track, pop, bounds, a.ga_ticks)
    res["evaluate_gains"] = {"individuals": a.individuals, "segments": a.segments, "vehicles": times.size,
                             "ticks": a.ga_ticks, "seconds": time.perf_counter() - t0,
                             "segments_finished": int(np.isfinite(times).sum()),
                             "includes": "start states, host-to-device copies, one mr_pid_drive launch that keeps the "
                                         "progress row, the row back, the crossing times on the host"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
