"""The weight-tuning GA of the reference (GA/mpcGA.py) on the device: segment drives that stop at the line.

``GA/mpcGA.py`` tunes the five ``RuntimeControllerParameters`` over segments of the lap, with a random number
where the segment time should come from driving (mpcGA.py:43).  ``ga.evaluate_population`` drives the vehicles
through ``ClosedLoop`` -- every vehicle for every tick, with torch glue between the launches and the crossing
times found on the host afterwards.  Here the same drive is library launches only:

* ``segment_times``: per tick ``mr_agent_sense``, ``mr_mpcseg_inputs`` (csrc/mr_mpcseg.h: the crossing test of
  ``ga.crossing_times`` and the solve's inputs), with ``warm_start="primal"`` ``mr_warm_shift``, the solve
  (``BatchSolver.launch`` with a horizon per vehicle) and ``mr_mpcseg_apply`` (command, plant step, the agent's
  memory).  A vehicle that has crossed its segment's end gets horizon 0, which the solve skips, and is not
  stepped again: the times are those of ``evaluate_population`` bit for bit, its state is the one it crossed
  with.  Two output sets alternate, so the previous tick's solution is read in place; nothing synchronises
  unless ``poll_every`` asks for it.
* ``tune_weights``: the GA itself, as ``pid.tune_gains`` is for the PID gains -- per generation one
  ``mr_mpcseg_runtime`` launch (genes in [0, 1] to runtime vectors), the drive, one ``mr_ga_breed`` launch.

No CPU fallback: without a GPU or the built library the calls raise.
"""
import ctypes
import math

import numpy as np
import torch

from . import abi, ga, rollout
from .batch import BatchSolver
from .closed_loop import ClosedLoop
from .geometry import DeviceTrack, _ptr
from .pid import TuneResult
from .track import CAR_WIDTH
from .tyrefit import _Device

RUNTIME_FIELDS = ["alpha_c", "d_max", "q_v_y", "n", "beta_delta"]
RUNTIME_DEFAULTS = [1000.0, 0.85, 50.0, 2.0, 5000.0]  # control/ControllerParameters.py:26-32
D_MAX_CLASS_ATTRIBUTE = 0.85  # what the reference's NLP reads whatever the runtime vector says (MPC.py:50)


class _SegmentDrive:
    """The buffers and the tick loop of ``segment_times`` for n_ind individuals on the K segments of ``bounds``:
    vehicle ind * K + k starts on the centerline at bounds[k] with speed v0 (``ClosedLoop.start_states``) and is
    MPC-controlled from tick 1 on (tick 0 applies (0.5, 0.0), agent.py:283), as ``ga.evaluate_population`` sets
    its ``ClosedLoop`` up.  ``run`` only enqueues."""

    def __init__(self, track, n_ind, bounds, v0, N, precision, plant, plant_params, dt, horizon, horizon_lookahead,
                 horizon_min, warm_start, device, solver_kw):
        if not torch.cuda.is_available():
            raise RuntimeError("mpcracing.mpc needs a ROCm GPU (torch.cuda.is_available() is False)")
        solver_kw = dict(solver_kw)
        self.track = track if isinstance(track, DeviceTrack) else DeviceTrack(track, device=device)
        self.lib, self.dev = self.track.lib, self.track.device
        bounds = np.asarray(bounds, np.float64)
        if bounds.ndim != 1 or len(bounds) < 2:
            raise ValueError("bounds: expected [K + 1] with K >= 1")
        self.K, self.N = len(bounds) - 1, int(N)
        self.n = n = int(n_ind) * self.K
        self.dt, self.Ts = float(dt), float(solver_kw.pop("Ts", 0.05))
        self.model_id, q = rollout._plant_args(plant, plant_params)
        if q.shape[0] not in (1, n):
            raise ValueError(f"plant_params: expected one vector or n = {n}, got {q.shape[0]}")
        f = dict(dtype=torch.float64, device=self.dev)
        i32 = dict(dtype=torch.int32, device=self.dev)
        self.q = torch.as_tensor(q, **f).contiguous() if plant_params is not None else None
        # horizon: None, "speed" (the rule on the device, mr_mpcseg_inputs) or an int array [n]
        self.hz_lookahead, self.hz_min, self.hz_in = 0.0, 1, None
        if isinstance(horizon, str):
            if horizon != "speed":
                raise ValueError('horizon: None, "speed" or an int array [P * K]')
            if not 1 <= int(horizon_min) <= self.N:
                raise ValueError(f"horizon_min must be in 1..N = {self.N}")
            if not float(horizon_lookahead) > 0:
                raise ValueError("horizon_lookahead must be > 0")
            self.hz_lookahead, self.hz_min = float(horizon_lookahead), int(horizon_min)
        elif horizon is not None:
            hz = np.asarray(horizon.cpu() if isinstance(horizon, torch.Tensor) else horizon)
            if hz.shape != (n,) or hz.dtype.kind not in "iu" or hz.min() < 1 or hz.max() > self.N:
                raise ValueError(f"horizon: an int array [{n}] with entries in 1..N = {self.N}")
            self.hz_in = torch.as_tensor(hz.astype(np.int32), device=self.dev).contiguous()
        if warm_start not in (None, "primal"):
            raise ValueError('warm_start: None or "primal"')
        self.warm_start = warm_start
        solver_kw.setdefault("dispatch_order", 2)  # ClosedLoop's default; results do not depend on it
        self.solver = BatchSolver(self.N, solver_kw.pop("mpc_model", "dyn"), precision, False, self.Ts, max_batch=n,
                                  device=self.dev.index, **solver_kw)
        # the read-only side: start states, segment bounds, the memory a drive starts from
        x0 = ClosedLoop.start_states(self.track, np.tile(bounds[:-1], int(n_ind)), v0=v0)
        self.start = torch.as_tensor(x0, **f).contiguous()
        self.s_start = torch.as_tensor(bounds[:-1].copy(), **f)
        self.s_end = torch.as_tensor(bounds[1:].copy(), **f)
        mem0 = np.zeros((abi.MR_MPCSEG_NMEM, n))
        mem0[0] = mem0[1] = np.nan  # old_yaw, prev_progress: the agent's None (ClosedLoop.reset)
        self.mem0 = torch.as_tensor(mem0, **f)
        # what a drive writes
        self.state, self.mem = torch.empty((6, n), **f), torch.empty((abi.MR_MPCSEG_NMEM, n), **f)
        self.done = torch.empty(n, **i32)
        self.progress, self.error, self.max_error = (torch.empty(n, **f) for _ in range(3))
        self.cx, self.cy = torch.empty((5, n), **f), torch.empty((5, n), **f)
        self.state0 = torch.empty((8, n), **f)
        self.u_init = torch.empty((2, self.N, n), **f)
        self.hz = [torch.empty(n, **i32) for _ in range(2)]
        self.sol = [self.solver.alloc_outputs(n) for _ in range(2)]
        if warm_start:
            self.warm = self.solver.alloc_warm(n)
            for s in self.sol:
                s["warm_used"] = torch.empty(n, **i32)

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(f"libmpcracing error {rc}: {self.lib.mr_last_error().decode()}")

    def reset(self, times, ticks_done, ticks):
        """The start of a drive, stream-ordered: every vehicle at its segment's first point, nothing finished."""
        self.state.copy_(self.start)
        self.mem.copy_(self.mem0)
        self.done.zero_()
        times.fill_(math.inf)
        ticks_done.fill_(int(ticks))

    def run(self, runtime, ticks, times, ticks_done, poll_every=None):
        """``ticks`` ticks on torch's current stream with runtime [5][n] (device); times [n] and ticks_done [n]
        (device) take the results.  Per tick four library calls (five with the primal warm start), from tick 1 on;
        tick 0 has no solve."""
        n, K, N, lib = self.n, self.K, self.N, self.lib
        st = torch.cuda.current_stream(self.dev)
        sp = ctypes.c_void_p(st.cuda_stream)
        L = self.track.length
        for t in range(int(ticks)):
            cur, prev = self.sol[t % 2], self.sol[(t - 1) % 2]
            hz_cur, hz_prev = self.hz[t % 2], self.hz[(t - 1) % 2]
            have_prev = t >= 2  # tick 0 is not controlled, tick 1 is the first solve
            warm = have_prev and self.warm_start is not None
            gather = have_prev and not warm
            self._check(lib.mr_agent_sense(self.track.h, n, _ptr(self.state[0]), _ptr(self.state[1]),
                                           _ptr(self.mem[1]), 5.0, 45.0, CAR_WIDTH / 2, _ptr(self.progress),
                                           _ptr(self.error), _ptr(self.cx), _ptr(self.cy), _ptr(self.max_error), sp))
            self._check(lib.mr_mpcseg_inputs(n, K, N, t, self.dt, L, _ptr(self.state), _ptr(self.progress),
                                             _ptr(self.mem), _ptr(self.s_start), _ptr(self.s_end),
                                             _ptr(prev["U"]) if gather else None, _ptr(hz_prev) if gather else None,
                                             _ptr(self.hz_in) if self.hz_in is not None else None, self.hz_lookahead,
                                             self.Ts, self.hz_min, _ptr(self.state0),
                                             _ptr(self.u_init) if gather else None, _ptr(hz_cur), _ptr(self.done),
                                             _ptr(times), _ptr(ticks_done), sp))
            if t >= 1:
                dev_in = dict(state0=self.state0, s0=self.progress, cx=self.cx, cy=self.cy, max_error=self.max_error,
                              runtime=runtime, u_init=self.u_init if gather else None, horizon=hz_cur,
                              order_hint=prev["iters"] if have_prev else None)
                if warm:
                    w = self.solver.warm_shift(prev, self.state0, self.progress, hz_prev, hz_cur, out=self.warm,
                                               stream=st)
                    dev_in.update(u_init=w["u_init"], x_init=w["x_init"], s_init=w["s_init"], warm_use=w["warm_use"])
                self.solver.launch(dev_in, cur, stream=st)
            self._check(lib.mr_mpcseg_apply(self.model_id, n, K, N, self.dt, L, _ptr(self.state), _ptr(self.mem),
                                            _ptr(self.progress), _ptr(self.s_start), _ptr(self.done),
                                            _ptr(cur["U"]) if t >= 1 else None,
                                            self.q.shape[0] if self.q is not None else 0,
                                            _ptr(self.q) if self.q is not None else None, sp))
            if poll_every and (t + 1) % int(poll_every) == 0 and bool(self.done.all()):
                break


def segment_times(track, population, bounds, ticks, v0=15.0, N=15, precision="fp64", plant="blend", plant_params=None,
                  dt=0.05, d_max_class_attribute=True, horizon=None, horizon_lookahead=20.0, horizon_min=5,
                  warm_start=None, poll_every=None, device=0, **solver_kw):
    """The segment times of ``ga.evaluate_population`` (bit for bit, inf included) without its records: P
    individuals ([P][5] runtime vectors) on K segments (bounds [K+1]), every tick library launches only, a
    vehicle's solves and plant steps ending at the tick at which it crosses its segment's end.

    plant_params: the plant's constants, [MR_PLANT_NPAR] or one vector per vehicle (``rollout.plant_params``).
    horizon, horizon_lookahead, horizon_min, warm_start, d_max_class_attribute: as ``evaluate_population``.
    poll_every=m: every m ticks the host reads whether every vehicle has finished and ends the loop if so (a
    synchronise each time); default: ``ticks`` ticks are enqueued with no synchronise before the end.
    Returns (times [P][K]; ticks_done [P][K], the ticks driven with the crossing tick included, ``ticks`` for a
    vehicle that never crosses; final_state [6][P*K], a finished vehicle's being the state it crossed with)."""
    pop = np.asarray(population, dtype=np.float64).reshape(-1, 5)
    P = pop.shape[0]
    if int(ticks) < 1:
        raise ValueError("ticks < 1")
    sd = _SegmentDrive(track, P, bounds, v0, N, precision, plant, plant_params, dt, horizon, horizon_lookahead, horizon_min,
                warm_start, device, solver_kw)
    rt = np.repeat(pop, sd.K, axis=0).T.copy()  # [5][P*K], vehicle = individual * K + segment
    if d_max_class_attribute:
        rt[1] = D_MAX_CLASS_ATTRIBUTE
    with torch.cuda.device(sd.dev):
        runtime = torch.as_tensor(rt, dtype=torch.float64, device=sd.dev).contiguous()
        times = torch.empty(sd.n, dtype=torch.float64, device=sd.dev)
        ticks_done = torch.empty(sd.n, dtype=torch.int32, device=sd.dev)
        sd.reset(times, ticks_done, ticks)
        sd.run(runtime, ticks, times, ticks_done, poll_every)
        torch.cuda.synchronize(sd.dev)
    return (times.cpu().numpy().reshape(P, sd.K), ticks_done.cpu().numpy().reshape(P, sd.K),
            sd.state.cpu().numpy())


def tune_weights(track, bounds, generations, ranges, islands=1, population=10, pairs=1, seed=0,
                 genes=("alpha_c", "q_v_y", "n", "beta_delta"), init=None, avg0=None, keep_times=False, ticks=240,
                 v0=15.0, N=15, precision="fp64", plant="blend", plant_params=None, dt=0.05,
                 d_max_class_attribute=True, horizon=None, horizon_lookahead=20.0, horizon_min=5, warm_start=None,
                 poll_every=None, kT=4.0, lambda_T=0.3, mutation_rate=0.4, device=0, **solver_kw):
    """The reference's weight-tuning GA (GA/mpcGA.py) with the fitness it never had: ``islands`` independent
    populations of ``population`` runtime vectors over ``generations`` generations, every (individual, segment)
    pair one vehicle of ``segment_times``' drive.  Everything stays on the device: per generation one
    ``mr_mpcseg_runtime`` launch (genes to runtime vectors), a stream-ordered reset, the tick loop and one
    ``mr_ga_breed`` launch on the gene rows; one synchronise at the end unless ``poll_every`` is set.

    genes: the tuned ``RUNTIME_FIELDS``; ranges: {name: (lo, hi)} for each of them.  A gene lives in [0, 1]
    (mpcGA.py:17) and stands for lo + gene * (hi - lo); the breeding clips to [0, 1].  The other parameters keep
    the ``RuntimeControllerParameters`` defaults (a range of zero width).  init [I][P][D] (or [P][D] for every
    island), default uniform [0, 1) from the stream (seed, island, generation 2**32 - 1); avg0: the segments'
    initial average times, a scalar, [K] or [I][K], default ticks * dt / 2.  Generation g draws from the stream
    (seed, island, g).  The drive's arguments are ``segment_times``'.  Returns a ``pid.TuneResult`` with
    ``weights`` [I][P][5] (the runtime vectors of the final population; with ``d_max_class_attribute`` the NLP
    reads 0.85 whatever their d_max) in place of ``gains``."""
    I, P, G = int(islands), int(population), int(generations)
    if G < 1 or I < 1:
        raise ValueError("generations and islands must be at least 1")
    if int(ticks) < 1:
        raise ValueError("ticks < 1")
    if not 2 <= P <= abi.MR_GA_P_MAX or not 1 <= int(pairs) <= P // 2 or len(bounds) - 1 > abi.MR_GA_K_MAX:
        raise ValueError(f"mr_ga_breed: 2 <= population <= {abi.MR_GA_P_MAX} per island, 1 <= pairs <= population / 2, "
                         f"at most {abi.MR_GA_K_MAX} segments")
    names = list(genes)
    unknown = [k for k in names if k not in RUNTIME_FIELDS]
    if unknown or len(set(names)) != len(names):
        raise ValueError(f"genes: distinct names of {RUNTIME_FIELDS} expected, got {names}")
    if sorted(ranges) != sorted(names):
        raise ValueError(f"ranges: one (lo, hi) for each of {names} expected, got {sorted(ranges)}")
    D = len(names)
    cols = [RUNTIME_FIELDS.index(k) for k in names]
    lo5, hi5 = np.array(RUNTIME_DEFAULTS), np.array(RUNTIME_DEFAULTS)
    for k, c in zip(names, cols):
        lo5[c], hi5[c] = (float(v) for v in ranges[k])
    if init is None:
        pop = np.stack([ga.random(seed, i, ga.INIT_GENERATION, 0, P * D).reshape(P, D) for i in range(I)])
    else:
        pop = np.array(np.broadcast_to(np.asarray(init, np.float64), (I, P, D)))
    full = np.zeros((I * P, 5))
    full[:, cols] = pop.reshape(I * P, D)
    sd = _SegmentDrive(track, I * P, bounds, v0, N, precision, plant, plant_params, dt, horizon, horizon_lookahead,
                horizon_min, warm_start, device, solver_kw)
    K, n = sd.K, sd.n
    avg = np.array(np.broadcast_to(np.asarray(ticks * dt / 2 if avg0 is None else avg0, np.float64), (I, K)))
    d_max = D_MAX_CLASS_ATTRIBUTE if d_max_class_attribute else math.nan
    with torch.cuda.device(sd.dev):
        be = _Device(sd.dev.index)
        d_g, d_avg, d_lo, d_hi = be.put(full), be.put(avg), be.put(lo5), be.put(hi5)
        d_b = be.put(np.stack([np.zeros(D), np.ones(D)]))
        d_rt = be.empty((5, n))
        d_t = be.empty((G if keep_times else 1, n))
        d_done, d_r = be.empty((n,), np.int32), be.empty((I, P))
        d_br, d_bi, d_bg = be.empty((G, I)), be.empty((G, I), np.int32), be.empty((G, I, D))
        col = (ctypes.c_int32 * D)(*cols)
        for g in range(G):
            t = d_t[g if keep_times else 0]
            be.call("mpcseg_runtime", I * P, K, be.ptr(d_g), be.ptr(d_lo), be.ptr(d_hi), d_max, be.ptr(d_rt),
                    sync=False)
            sd.reset(t, d_done, ticks)
            sd.run(d_rt, ticks, t, d_done, poll_every)
            ga.breed_launch(be, False, (I, P, K, D, int(pairs)), d_g, 5, col, t, d_avg, d_b,
                            (kT, lambda_T, mutation_rate), seed, 0, g, d_r, d_br[g], d_bi[g], d_bg[g])
        torch.cuda.synchronize(sd.dev)
    out = np.array(be.get(d_g)).reshape(I, P, 5)
    return TuneResult(population=out[:, :, cols].copy(), weights=lo5 + out * (hi5 - lo5),
                      best_reward=np.array(be.get(d_br)), best_index=np.array(be.get(d_bi)),
                      best_genes=np.array(be.get(d_bg)), avg=np.array(be.get(d_avg)), rewards=np.array(be.get(d_r)),
                      ticks_done=np.array(be.get(d_done)).reshape(I, P, K),
                      times=np.array(be.get(d_t)).reshape(G, I, P, K) if keep_times else None, genes=names)
