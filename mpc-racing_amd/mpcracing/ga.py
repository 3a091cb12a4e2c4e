"""Batched fitness evaluation of controller-parameter populations.

The reference's GA (GA/mpcGA.py:16-62) scores each individual -- a RuntimeControllerParameters
vector (alpha_c, d_max, q_v_y, n, beta_delta) -- by its time over a track segment
(splines/TrackSegments.py:7-35 splits the lap into ``num_checkpoints`` equal-time segments),
rewards it with ``exp(-kT (segment_time - average_time))`` and updates the segment's running
average ``lambda_T * segment_time + (1 - lambda_T) * average_time`` (mpcGA.py:18-23).  The
reference's loop has a random placeholder where the segment time should come from driving;
here every (individual, segment) pair is one vehicle of a batched closed loop
(mpcracing.ClosedLoop): population x segments vehicles start at their segment's first point,
are MPC-controlled from the first tick, and the segment time is the first tick at which their
progress passes the segment end (linear interpolation inside the tick; ``inf`` if not reached).
"""
import numpy as np
import torch

from .closed_loop import ClosedLoop

KT, KC, LAMBDA_T = 4.0, 0.5, 0.3  # GA/mpcGA.py:11-13


def compute_reward(segment_time, average_time):
    return np.exp(-KT * (segment_time - average_time))   # mpcGA.py:18-20


def compute_avg_time(segment_time, average_time):
    return LAMBDA_T * segment_time + (1 - LAMBDA_T) * average_time   # mpcGA.py:22-23


def segment_times(records, s_start, s_end, length, dt):
    """First crossing time of s_end [B] by the progress records (track wrap handled)."""
    prog = np.stack([r["progress"].cpu().numpy() for r in records])          # [T][B]
    return crossing_times(prog, s_start, s_end, length, dt)


def crossing_times(prog, s_start, s_end, length, dt):
    """``segment_times`` on the progress array [T][B] itself."""
    travelled = np.mod(prog - s_start[None, :], length)                      # distance along the lap
    # the first ticks may sit slightly behind the start (projection): treat > L/2 as negative
    travelled = np.where(travelled > 0.5 * length, travelled - length, travelled)
    need = np.mod(s_end - s_start, length)
    B = prog.shape[1]
    out = np.full(B, np.inf)
    for b in range(B):
        hit = np.nonzero(travelled[:, b] >= need[b])[0]
        if len(hit) and hit[0] > 0:
            k = hit[0]
            a, c = travelled[k - 1, b], travelled[k, b]
            out[b] = dt * ((k - 1) + (need[b] - a) / (c - a))
    return out


def evaluate_population(track, population, bounds, ticks, v0=15.0, N=15, precision="fp64", plant="blend",
                        dt=0.05, d_max_class_attribute=True, horizon=None, horizon_lookahead=20.0, horizon_min=5,
                        warm_start=None, **solver_kw):
    """Segment times [P][K] of P individuals ([P][5] runtime vectors) on K segments (bounds [K+1]).

    d_max_class_attribute: the reference's NLP ignores the runtime d_max (MPC.py:50 reads the
    class attribute 0.85); True reproduces that.
    horizon, horizon_lookahead, horizon_min: ClosedLoop's (None, "speed" or an int array [P*K], vehicle =
    individual * K + segment).
    warm_start: ClosedLoop's (None, or "primal": each tick starts from the previous solution, shifted)."""
    pop = np.asarray(population, dtype=np.float64).reshape(-1, 5)
    P, K = pop.shape[0], len(bounds) - 1
    starts = np.asarray(bounds[:-1], dtype=np.float64)
    ends = np.asarray(bounds[1:], dtype=np.float64)
    rt = np.repeat(pop, K, axis=0).T.copy()             # [5][P*K], vehicle = individual * K + segment
    if d_max_class_attribute:
        rt[1] = 0.85
    s0 = np.tile(starts, P)
    loop = ClosedLoop(track, B=P * K, N=N, plant=plant, precision=precision, dt=dt, start_control_at=1,
                      runtime=rt, horizon=horizon, horizon_lookahead=horizon_lookahead, horizon_min=horizon_min,
                      warm_start=warm_start, **solver_kw)
    x0 = ClosedLoop.start_states(loop.track, s0, v0=v0)
    loop.reset(x0)
    recs = loop.run(ticks)
    torch.cuda.synchronize(loop.dev)
    t = segment_times(recs, s0, np.tile(ends, P), loop.track.length, dt)
    return t.reshape(P, K), recs


def rewards(times, avg_times):
    """Per-individual reward sum and the updated segment averages, in the order of mpcGA.py:40-56
    (individual i on its segment, averages updated as the individuals are scored)."""
    avg = np.array(avg_times, dtype=np.float64)
    P, K = times.shape
    r = np.zeros(P)
    for i in range(P):
        for k in range(K):
            a = avg[k]
            avg[k] = compute_avg_time(times[i, k], a)
            r[i] += compute_reward(times[i, k], a)
    return r, avg


MUTATION_RATE = 0.4  # GA/pdGA.py:9
INIT_GENERATION = 2 ** 32 - 1  # the stream's generation that draws an initial population (pdGA.py:23)


def random(seed, island, generation, first, count, raw=False, host_twin=False):
    """Draws first .. first + count - 1 of the GA's stream (``mr_ga_random``; needs no GPU): what
    ``numpy.random.Philox(key=[seed, island], counter=[0, 0, generation, 0])`` gives as ``random_raw`` (``raw``) or
    through ``Generator.random()`` (the doubles (raw >> 11) * 2**-53)."""
    import ctypes
    from . import abi
    out = np.zeros(int(count), np.uint64)
    if host_twin:
        rc = abi.load_host_twin().mrh_ga_random(seed, island, generation, first, int(count), out.ctypes.data)
    else:
        lib = abi._bind_product(ctypes.CDLL(abi.PRODUCT_LIB))  # host code only: no device is touched
        rc = lib.mr_ga_random(seed, island, generation, first, int(count), out.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"mr_ga_random failed ({rc})")
    return out if raw else (out >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


class BreedResult:
    """One generation: the new ``genes`` [I][P][D], the rewards ``r`` [I][P] and the updated averages ``avg``
    [I][K]; per island the best reward ``best_r``, its index ``best_idx`` and its genes before the replacement
    ``best_genes`` [I][D]."""

    def __init__(self, genes, r, avg, best_r, best_idx, best_genes):
        self.genes, self.r, self.avg = genes, r, avg
        self.best_r, self.best_idx, self.best_genes = best_r, best_idx, best_genes


def _bounds(lo, hi, D):
    """[2][D] with NaN for no bound, or None when neither is given"""
    if lo is None and hi is None:
        return None
    b = np.full((2, D), np.nan)
    if lo is not None:
        b[0] = np.broadcast_to(np.asarray(lo, np.float64), (D,))
    if hi is not None:
        b[1] = np.broadcast_to(np.asarray(hi, np.float64), (D,))
    return b


def breed_launch(be, host_twin, dims, genes, ld, col, times, avg, bounds, consts, seed, island0, generation, r, best_r,
                 best_idx, best_genes):
    """``mr_ga_breed`` (or the host build's) on arrays of backend ``be``; no synchronise.  dims = (islands, P, K, D,
    pairs), col a ctypes int32 array or None, bounds the device array [2][D] or None, consts = (kT, lambda_T,
    mutation_rate)."""
    n_island, P, K, D, pairs = dims
    lo = be.ptr(bounds[0]) if bounds is not None else None
    hi = be.ptr(bounds[1]) if bounds is not None else None
    p = lambda a: None if a is None else be.ptr(a)  # noqa: E731
    be.call("ga_breed", n_island, P, K, D, pairs, p(genes), ld, col, p(times), p(avg), lo, hi,
            *[float(c) for c in consts], int(seed), int(island0), int(generation), p(r), p(best_r), p(best_idx),
            p(best_genes), sync=False)


def breed(genes, times, avg, pairs=1, lo=None, hi=None, kT=KT, lambda_T=LAMBDA_T, mutation_rate=MUTATION_RATE, seed=0,
          island0=0, generation=0, host_twin=False, device=0):
    """One generation of the reference's GA step (GA/pdGA.py:57-91 with the rewards of GA/mpcGA.py:40-56) for I
    islands in one launch (``mr_ga_breed``, csrc/mr_ga.h: one wavefront per island): genes [I][P][D] (or [P][D]),
    times [I][P][K] (non-finite: segment not finished), avg [I][K]; ``pairs`` pairs of parents by roulette
    selection, one-point crossover, mutation, clip to ``lo`` / ``hi`` (scalars or [D], NaN or None for none), the
    children replacing the lowest rewards.  The draws are those of ``random(seed, island0 + island, generation,
    ...)``.  Returns a BreedResult (numpy; the inputs are not changed).  ``host_twin=True`` runs the host build
    (TEST-ONLY)."""
    from .tyrefit import _Device, _Host
    genes = np.asarray(genes, np.float64)
    single = genes.ndim == 2
    genes = genes.reshape((-1,) + genes.shape[-2:])
    n_island, P, D = genes.shape
    times = np.asarray(times, np.float64).reshape(n_island, P, -1)
    K = times.shape[2]
    avg = np.asarray(avg, np.float64).reshape(n_island, K)
    b = _bounds(lo, hi, D)
    be = _Host() if host_twin else _Device(device)
    d_genes, d_times, d_avg = be.put(np.array(genes)), be.put(times), be.put(np.array(avg))
    d_b = be.put(b) if b is not None else None
    r, best_r, best_genes = be.empty((n_island, P)), be.empty((n_island,)), be.empty((n_island, D))
    best_idx = be.empty((n_island,), np.int32)
    breed_launch(be, host_twin, (n_island, P, K, D, int(pairs)), d_genes, D, None, d_times, d_avg, d_b,
                 (kT, lambda_T, mutation_rate), seed, island0, generation, r, best_r, best_idx, best_genes)
    if not host_twin:
        be.torch.cuda.synchronize(be.dev)
    out = [np.array(be.get(a)) for a in (d_genes, r, d_avg, best_r, best_idx, best_genes)]
    if single:
        out = [a[0] for a in out]
    return BreedResult(*out)


# splines/TrackSegments.py:7-35, the drop-in module (host quadrature, reference formulas)
from splines.TrackSegments import TrackSegments  # noqa: E402,F401
