"""The reference's PID agent on the GPU: whole drives in one launch, gains per vehicle.

``agent_pid.py`` is the reference's second controller and the one that drove every log it learns from: pure
pursuit plus PD on the centerline error for the steering, a curvature-based speed target with PD throttle, a
brake floor of 0.5.  ``control`` is one ``Agent.run_step`` for a batch of vehicles (``mr_pid_control``);
``drive`` keeps every vehicle on the device for a whole drive against the ``models/`` plant (``mr_pid_drive``,
csrc/mr_pid.h: one lane per vehicle, state, memory and gains in registers, one launch per 4096 ticks) and
returns the drive as logs that ``rollout.load_log`` / ``rollout_errors`` / ``plantfit`` take;
``evaluate_gains`` is the fitness of the gain-tuning GA (GA/pdGA.py:48-55): segment times of a population of
gain vectors, every (individual, segment) pair one vehicle of one drive.  ``segment_times`` gives the same times
without the log, taken as the vehicles drive (``mr_pid_segment_times``: a vehicle's drive ends at its crossing), and
``tune_gains`` is the GA itself: per generation that launch and one ``mr_ga_breed`` (csrc/mr_ga.h, ``ga.breed``),
all generations on one stream with one synchronise.

``host_twin=True`` runs the g++ build of the same source instead (TEST-ONLY, explicit; there is no fallback:
without it a missing GPU or library is an error).
"""
import ctypes
import os

import numpy as np

from . import abi, rollout, runlog
from .tyrefit import _Device, _Host

GAIN_FIELDS = ["k", "zeta", "kP_steer", "kD_steer", "kP_throttle", "kD_throttle", "lookahead",
               "vel_lookahead_factor"]
GAIN_DEFAULTS = [1.1, 15.0, 0.1, 0.1, 0.82954, 1.21341, 3.0, 40.0]  # agent_pid.py:47-58 (mr_pid_gains_default)
OUT_ROWS = ["progress", "error", "cmd_throttle", "cmd_steer", "cmd_brake", "target_vel", "kappa", "yawdot_fd"]
LOG_ROWS = ["X", "Y", "yaw", "vx", "vy", "yawdot", "yawdot_fd", "progress", "error", "cmd_throttle", "cmd_steer",
            "cmd_brake", "target_vel", "kappa"]
T_MAX = 4096  # ticks per mr_pid_drive call
assert len(GAIN_FIELDS) == len(GAIN_DEFAULTS) == abi.MR_PID_NGAIN and len(LOG_ROWS) == abi.MR_PID_NLOG


def gains(**overrides):
    """[MR_PID_NGAIN]: the agent's default gains with ``overrides`` by name (``GAIN_FIELDS``); an unknown name
    raises."""
    unknown = [k for k in overrides if k not in GAIN_FIELDS]
    if unknown:
        raise ValueError(f"unknown gain(s) {unknown}; the fields are {GAIN_FIELDS}")
    g = np.array(GAIN_DEFAULTS, np.float64)
    for k, v in overrides.items():
        g[GAIN_FIELDS.index(k)] = float(v)
    return g


class _HostTrack:
    """TEST-ONLY: the centerline tables as a host blob (the arguments of the host build's track functions)."""

    def __init__(self, tables):
        t, cx, cy, L, el, er = tables
        self.lib = abi.load_host_twin()
        t, cx, cy = (np.ascontiguousarray(a, np.float64) for a in (t, cx, cy))
        el = np.zeros(0) if el is None else np.ascontiguousarray(el, np.float64)
        er = np.zeros(0) if er is None else np.ascontiguousarray(er, np.float64)
        self.nt, self.nr, self.length = len(t), len(el), float(L)
        self.blob = np.zeros(self.lib.mrh_track_blob_size(self.nt, self.nr))
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        self.lib.mrh_track_build(p(t), self.nt, p(cx), p(cy), len(cx), p(el) if self.nr else None,
                                 p(er) if self.nr else None, self.nr, p(self.blob))

    def args(self):
        return [self.blob.ctypes.data_as(ctypes.c_void_p), self.nt, self.length, self.nr]

    # the two queries of ClosedLoop.start_states, as CPU tensors
    def eval(self, s):
        import torch
        s = np.ascontiguousarray(s, np.float64)
        out, span = np.zeros((6, len(s))), np.zeros(len(s), np.int32)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        self.lib.mrh_track_eval(*self.args(), len(s), p(s), p(out), p(span))
        return torch.from_numpy(out), torch.from_numpy(span)

    def frame(self, s):
        import torch
        s = np.ascontiguousarray(s, np.float64)
        yaw, kap, nx, ny, mk = (np.zeros(len(s)) for _ in range(5))
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        self.lib.mrh_track_frame(*self.args(), len(s), p(s), p(yaw), p(kap), p(nx), p(ny), 45.0, p(mk))
        return dict(yaw=torch.from_numpy(yaw), nx=torch.from_numpy(nx), ny=torch.from_numpy(ny))


def _track(track, host_twin, device):
    """``track``: a ``DeviceTrack``, a ``mpcracing.track.Track``, a track name, or tables (t, cx, cy, L, err_left,
    err_right) as ``DeviceTrack(tables=...)`` takes them (lane tables may be None: the agent never reads them)."""
    if isinstance(track, _HostTrack) or (not host_twin and hasattr(track, "h")):
        return track
    tables = track if isinstance(track, (tuple, list)) else None
    if host_twin:
        if tables is None:
            from .track import Track
            tr = track if isinstance(track, Track) else Track(track)
            tables = (tr.spline_x.t, tr.spline_x.c, tr.spline_y.c, tr.length, tr.err_left, tr.err_right)
        return _HostTrack(tables)
    from .geometry import DeviceTrack
    return DeviceTrack(device=device, tables=tables) if tables is not None else DeviceTrack(track, device=device)


def _backend(tr, host_twin):
    return _Host() if host_twin else _Device(tr.device.index)


def _gains(g, n):
    g = gains() if g is None else np.asarray(g, np.float64)
    g = np.ascontiguousarray(np.atleast_2d(g))
    if g.ndim != 2 or g.shape[1] != abi.MR_PID_NGAIN or g.shape[0] not in (1, n):
        raise ValueError(f"gains: expected [{abi.MR_PID_NGAIN}] or [n = {n}][{abi.MR_PID_NGAIN}], got {g.shape}")
    return g


def control(track, state, mem, gains, dt, host_twin=False, device=0):
    """One ``Agent.run_step`` (agent_pid.py:157-237) of n vehicles: state [6][n] = (X, Y, yaw, vx, vy, yawdot),
    mem [4][n] = (prev_progress, last_error, last_throttle_error, old_yaw) with NaN for the reference's None,
    gains [8] or [n][8].  Returns (out [8][n] (``OUT_ROWS``), the updated mem [4][n]), numpy."""
    tr = _track(track, host_twin, device)
    state = np.ascontiguousarray(state, np.float64).reshape(6, -1)
    n = state.shape[1]
    mem = np.array(mem, np.float64).reshape(abi.MR_PID_NMEM, n)
    g = _gains(gains, n)
    be = _backend(tr, host_twin)
    d = [be.put(state), be.put(mem), be.put(g)]
    out = be.empty((abi.MR_PID_NOUT, n))
    be.call("pid_control", n, be.ptr(d[0]), be.ptr(d[1]), g.shape[0], be.ptr(d[2]), float(dt), be.ptr(out), track=tr)
    return be.get(out), np.array(be.get(d[1]))


class PidResult:
    """A drive of n vehicles: ``rows`` name -> [T][n] (the kept ``LOG_ROWS``; NaN from the tick at which a
    vehicle stopped), the final ``state`` [6][n] and ``mem`` [4][n] (a stopped vehicle's: those its last tick
    started from), ``ticks_done`` [n], ``dt``."""

    def __init__(self, rows, state, mem, ticks_done, dt):
        self.rows, self.state, self.mem, self.ticks_done, self.dt = rows, state, mem, ticks_done, dt

    def _need(self, names):
        missing = [r for r in names if r not in self.rows]
        if missing:
            raise ValueError(f"the drive kept no {missing} rows (drive(rows=...))")

    def log(self, i, yawdot="agent"):
        """[9][T] (``rollout.LOG_ROWS``) of vehicle ``i``, as ``rollout.load_log`` gives it for a logged run:
        throttle = cmd_throttle - cmd_brake, ts = dt, the yaw through ``rollout.unwrap``; the yaw rate is the
        agent's finite difference (``"agent"``: what the reference's Logger records, NaN at the first tick) or
        the plant's state (``"plant"``)."""
        if yawdot not in ("agent", "plant"):
            raise ValueError("yawdot is 'agent' or 'plant'")
        yd = "yawdot_fd" if yawdot == "agent" else "yawdot"
        self._need(["X", "Y", "yaw", "vx", "vy", yd, "cmd_throttle", "cmd_steer", "cmd_brake"])
        r = {k: v[:, i] for k, v in self.rows.items()}
        return np.stack([r["X"], r["Y"], rollout.unwrap(r["yaw"]), r["vx"], r["vy"], r[yd],
                         r["cmd_throttle"] - r["cmd_brake"], r["cmd_steer"], np.full(len(r["X"]), float(self.dt))])

    def write_run(self, run_dir, i=0, yawdot="agent"):
        """``<run_dir>/steps.csv`` of vehicle ``i`` in the reference's Logger column order
        (``runlog.MEMBER_NAMES``), which ``rollout.load_log`` reads back; the lane-boundary points are ``None``."""
        yd = "yawdot_fd" if yawdot == "agent" else "yawdot"
        self._need(["X", "Y", "yaw", "vx", "vy", yd, "progress", "error", "cmd_throttle", "cmd_steer", "cmd_brake"])
        os.makedirs(run_dir, exist_ok=True)
        T = len(self.rows["X"])
        with open(os.path.join(run_dir, "steps.csv"), "w") as f:
            f.write(",".join(runlog.MEMBER_NAMES) + "\n")
            for t in range(T):
                rec = {k: v[t] for k, v in self.rows.items()}
                rec["yawdot"] = self.rows[yd][t]
                rec["step"] = t
                f.write(runlog.steps_line(rec, i, self.dt))


def _mask(rows):
    rows = LOG_ROWS if rows is None else list(rows)
    unknown = [r for r in rows if r not in LOG_ROWS]
    if unknown:
        raise ValueError(f"unknown row(s) {unknown}; the rows are {LOG_ROWS}")
    kept = [r for r in LOG_ROWS if r in rows]  # packed in row order
    return kept, sum(1 << LOG_ROWS.index(r) for r in kept)


def drive(track, state0, ticks, gains=None, model="blend", params=None, dt=0.05, progress0=None, rows=None,
          host_twin=False, device=0, mem0=None):
    """``ticks`` ticks of the PID agent against the ``model`` plant ("kin", "dyn", "blend") from state0 [6][n].
    gains [8] or [n][8] (default: ``gains()``), params [MR_PLANT_NPAR] or [n][...] (``rollout.plant_params``).
    The agent's memory starts as (progress0 or NaN, 0, 0, NaN) -- NaN progress: the first projection is the
    global one -- or as ``mem0`` [4][n] (``PidResult.mem`` of an earlier drive, to continue it).  rows: the
    ``LOG_ROWS`` to keep (default: all; [] for none).  One ``mr_pid_drive`` call per 4096 ticks.  Returns a
    PidResult."""
    tr = _track(track, host_twin, device)
    state = np.array(state0, np.float64).reshape(6, -1)
    n, T = state.shape[1], int(ticks)
    if T < 1:
        raise ValueError("ticks < 1")
    if mem0 is not None:
        mem = np.array(mem0, np.float64).reshape(abi.MR_PID_NMEM, n)
    else:
        mem = np.zeros((abi.MR_PID_NMEM, n))
        mem[0] = np.nan if progress0 is None else np.broadcast_to(np.asarray(progress0, np.float64), (n,))
        mem[3] = np.nan
    g = _gains(gains, n)
    model_id, q = rollout._plant_args(model, params)
    if q.shape[0] not in (1, n):
        raise ValueError(f"params: expected one vector or n = {n}, got {q.shape[0]}")
    kept, mask = _mask(rows)
    be = _backend(tr, host_twin)
    d_state, d_mem, d_g, d_q = be.put(state), be.put(mem), be.put(g), be.put(q)
    done = np.zeros(n, np.int64)
    chunks = []
    for t0 in range(0, T, T_MAX):
        Tc = min(T_MAX, T - t0)
        log = be.empty((len(kept), Tc, n)) if kept else None
        td = be.empty((n,), np.int32)
        be.call("pid_drive", model_id, n, Tc, float(dt), be.ptr(d_state), be.ptr(d_mem), g.shape[0], be.ptr(d_g),
                q.shape[0], be.ptr(d_q), mask, be.ptr(log) if kept else None, be.ptr(td), track=tr)
        td = be.get(td)
        done += np.where(done == t0, td, 0)  # a stopped vehicle stays stopped in the later calls
        chunks.append(be.get(log) if kept else None)
    out = {}
    if kept:
        full = np.concatenate(chunks, axis=1)
        out = {name: full[j] for j, name in enumerate(kept)}
    return PidResult(out, np.array(be.get(d_state)), np.array(be.get(d_mem)), done.astype(np.int32), float(dt))


def evaluate_gains(track, population, bounds, ticks, v0=15.0, model="blend", params=None, dt=0.05,
                   host_twin=False, device=0):
    """Segment times [P][K] of P gain vectors on K segments (bounds [K+1]): the fitness of GA/pdGA.py:48-55.
    population [P][4] = (kP_steer, kD_steer, kP_throttle, kD_throttle) (pdGA.py:5; the other gains default)
    or [P][8].  Vehicle individual * K + segment starts on the centerline at its segment's first point with
    speed v0 (``ClosedLoop.start_states``) and is driven for ``ticks`` ticks in one drive that keeps only the
    progress row; its time is the first crossing of the segment's end (``ga.crossing_times``, inf if not
    reached).  Returns (times, the PidResult)."""
    from .closed_loop import ClosedLoop
    from .ga import crossing_times
    pop = _full_gains(population)
    P, K = pop.shape[0], len(bounds) - 1
    starts = np.asarray(bounds[:-1], np.float64)
    ends = np.asarray(bounds[1:], np.float64)
    tr = _track(track, host_twin, device)
    s0 = np.tile(starts, P)
    x0 = ClosedLoop.start_states(tr, s0, v0=v0)
    res = drive(tr, x0, ticks, gains=np.repeat(pop, K, axis=0), model=model, params=params, dt=dt, progress0=s0,
                rows=["progress"], host_twin=host_twin, device=device)
    t = crossing_times(res.rows["progress"], s0, np.tile(ends, P), tr.length, dt)
    return t.reshape(P, K), res


def _full_gains(population):
    """[G][8]: gain vectors given whole, or as the GA's four (kP_steer, kD_steer, kP_throttle, kD_throttle) in
    the default gains"""
    pop = np.atleast_2d(np.asarray(population, np.float64))
    if pop.shape[1] == 4:
        full = np.tile(gains(), (pop.shape[0], 1))
        full[:, 2:6] = pop
        pop = full
    elif pop.shape[1] != abi.MR_PID_NGAIN:
        raise ValueError(f"gains: expected [G][4] or [G][{abi.MR_PID_NGAIN}], got {pop.shape}")
    return np.ascontiguousarray(pop)


class _SegmentDrive:
    """The read-only side of ``mr_pid_segment_times`` on a backend: the segments' start states, bounds and the
    plant parameters, put there once; ``launch`` only enqueues."""

    def __init__(self, track, bounds, n_gain, v0, model, params, dt, host_twin, device):
        from .closed_loop import ClosedLoop
        self.tr = _track(track, host_twin, device)
        self.host_twin = host_twin
        bounds = np.asarray(bounds, np.float64)
        if bounds.ndim != 1 or len(bounds) < 2:
            raise ValueError("bounds: expected [K + 1] with K >= 1")
        self.K = len(bounds) - 1
        self.n = int(n_gain) * self.K
        self.model_id, q = rollout._plant_args(model, params)
        if q.shape[0] not in (1, self.n):
            raise ValueError(f"params: expected one vector or n = {self.n}, got {q.shape[0]}")
        self.P, self.dt = q.shape[0], float(dt)
        self.be = be = _backend(self.tr, host_twin)
        x0 = ClosedLoop.start_states(self.tr, bounds[:-1], v0=v0)
        self.start, self.s_start, self.s_end, self.q = be.put(x0), be.put(bounds[:-1]), be.put(bounds[1:]), be.put(q)

    def launch(self, d_gains, ticks, d_times, d_done):
        be = self.be
        p = lambda a: None if a is None else be.ptr(a)  # noqa: E731
        be.call("pid_segment_times", self.model_id, self.n, self.K, int(ticks), self.dt, p(self.start),
                p(self.s_start), p(self.s_end), p(d_gains), self.P, p(self.q), p(d_times), p(d_done), track=self.tr,
                sync=False)

    def sync(self):
        if not self.host_twin:
            self.be.torch.cuda.synchronize(self.be.dev)


def segment_times(track, gains, bounds, ticks, v0=15.0, model="blend", params=None, dt=0.05, host_twin=False,
                  device=0):
    """The times of ``evaluate_gains`` (bit for bit) without its log: G gain vectors ([G][4] or [G][8], as there)
    on K segments (bounds [K+1]) in one ``mr_pid_segment_times`` launch that takes each vehicle's crossing time
    from its progress as it drives and ends a vehicle's drive there (csrc/mr_pid.h pid_segment_vehicle).
    1 <= ticks <= 4096.  Returns (times [G][K], inf where the segment's end is not reached; ticks_done [G][K],
    the ticks driven, the crossing tick included)."""
    g = _full_gains(gains)
    sd = _SegmentDrive(track, bounds, g.shape[0], v0, model, params, dt, host_twin, device)
    be = sd.be
    d_g, t, done = be.put(g), be.empty((sd.n,)), be.empty((sd.n,), np.int32)
    sd.launch(d_g, ticks, t, done)
    sd.sync()
    return np.array(be.get(t)).reshape(-1, sd.K), np.array(be.get(done)).reshape(-1, sd.K)


class TuneResult:
    """A GA run of ``tune_gains``: ``population`` [I][P][D] (the final genes) and ``gains`` [I][P][8] (the gain
    vectors they make); per generation and island ``best_reward`` [G][I], ``best_index`` [G][I] and ``best_genes``
    [G][I][D] (the best individual of the generation as it was scored); ``avg`` [I][K] the final running averages;
    ``rewards`` [I][P] and ``ticks_done`` [I][P][K] of the last generation; ``times`` [G][I][P][K] with
    ``keep_times`` (else None); ``genes`` the gene names."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def tune_gains(track, bounds, generations, islands=1, population=10, pairs=1, seed=0,
               genes=("kP_steer", "kD_steer", "kP_throttle", "kD_throttle"), init=None, lo=None, hi=None, avg0=None,
               keep_times=False, ticks=240, v0=15.0, model="blend", params=None, dt=0.05, kT=4.0, lambda_T=0.3,
               mutation_rate=0.4, host_twin=False, device=0):
    """The reference's gain-tuning GA (GA/pdGA.py) with the fitness it never had: ``islands`` independent
    populations of ``population`` gain vectors over ``generations`` generations, every (individual, segment) pair
    one vehicle.  Everything stays on the device: per generation one ``mr_pid_segment_times`` launch (the segment
    times of all islands) and one ``mr_ga_breed`` launch (rewards, selection, crossover, mutation and replacement,
    one wavefront per island, on the gain rows themselves), 2 * generations launches on one stream and one
    synchronise at the end.

    genes: the tuned ``GAIN_FIELDS`` (the others keep their defaults); init [I][P][D] (or [P][D] for every
    island), default uniform [0, 1) from the stream (seed, island, generation 2**32 - 1) (pdGA.py:23); lo, hi: gene
    bounds (scalars or [D]); avg0: the segments' initial average times, a scalar, [K] or [I][K], default
    ticks * dt / 2 (the reference's lap_time / num_checkpoints of TrackSegments can be passed here).  Generation g
    draws from the stream (seed, island, g).  Returns a TuneResult."""
    from . import ga
    I, P, G = int(islands), int(population), int(generations)
    if G < 1 or I < 1:
        raise ValueError("generations and islands must be at least 1")
    names = list(genes)
    unknown = [k for k in names if k not in GAIN_FIELDS]
    if unknown or len(set(names)) != len(names):
        raise ValueError(f"genes: distinct names of {GAIN_FIELDS} expected, got {names}")
    D = len(names)
    cols = [GAIN_FIELDS.index(k) for k in names]
    if init is None:
        pop = np.stack([ga.random(seed, i, ga.INIT_GENERATION, 0, P * D, host_twin=host_twin).reshape(P, D)
                        for i in range(I)])
    else:
        pop = np.array(np.broadcast_to(np.asarray(init, np.float64), (I, P, D)))
    full = np.tile(gains(), (I * P, 1))
    full[:, cols] = pop.reshape(I * P, D)
    sd = _SegmentDrive(track, bounds, I * P, v0, model, params, dt, host_twin, device)
    K, be = sd.K, sd.be
    avg = np.array(np.broadcast_to(np.asarray(ticks * dt / 2 if avg0 is None else avg0, np.float64), (I, K)))
    b = ga._bounds(lo, hi, D)
    d_g, d_avg = be.put(full), be.put(avg)
    d_b = be.put(b) if b is not None else None
    d_t = be.empty((G if keep_times else 1, I * P * K))
    d_done, d_r = be.empty((I * P * K,), np.int32), be.empty((I, P))
    d_br, d_bi, d_bg = be.empty((G, I)), be.empty((G, I), np.int32), be.empty((G, I, D))
    col = (ctypes.c_int32 * D)(*cols)
    for g in range(G):
        t = d_t[g if keep_times else 0]
        sd.launch(d_g, ticks, t, d_done)
        ga.breed_launch(be, host_twin, (I, P, K, D, int(pairs)), d_g, abi.MR_PID_NGAIN, col, t, d_avg, d_b,
                        (kT, lambda_T, mutation_rate), seed, 0, g, d_r, d_br[g], d_bi[g], d_bg[g])
    sd.sync()
    out = np.array(be.get(d_g)).reshape(I, P, abi.MR_PID_NGAIN)
    return TuneResult(population=out[:, :, cols].copy(), gains=out, best_reward=np.array(be.get(d_br)),
                      best_index=np.array(be.get(d_bi)), best_genes=np.array(be.get(d_bg)),
                      avg=np.array(be.get(d_avg)), rewards=np.array(be.get(d_r)),
                      ticks_done=np.array(be.get(d_done)).reshape(I, P, K),
                      times=np.array(be.get(d_t)).reshape(G, I, P, K) if keep_times else None, genes=names)
