"""Which plant constants reproduce a logged drive: a deterministic grid search over rollouts.

script/optimize_coeffs.py searches ``dt`` or ``(Cf, Cr)`` of a models/ plant with ``scipy.optimize.dual_annealing``:
10 000 serial rollouts of one start, minimising the norm of the position differences (its lines 34-48).
``identify`` minimises the same quantity squared, summed over every start row (``RolloutErrors.position_cost``),
by a shrinking grid: each round is ONE ``mr_plant_rollout`` call over the grid^d parameter sets x all starts x
``horizon`` steps (csrc/mr_plantroll.h), the next round's box is centred on the best set, shrunk and clipped to
the original bounds, and its grid keeps the previous best point as a node, so the best cost never increases.
No random numbers: two calls return identical results.
"""
import itertools

import numpy as np

from . import rollout

MAX_FREE = 3


class IdentifyResult:
    """``values``: {name: value} of the free fields at the lowest cost; ``params`` [MR_PLANT_NPAR] the full vector;
    ``dt``: the fixed step (None: the log's ts); ``cost``: its position cost; ``history``: one dict per round
    (``lo``, ``hi`` of the box, ``n_sets``, ``best_values``, ``best_cost``: the best of everything evaluated so
    far, ``round_min``: the lowest cost of the round's own grid)."""

    def __init__(self, values, params, dt, cost, history):
        self.values, self.params, self.dt, self.cost, self.history = values, params, dt, cost, history


def _nodes(lo, hi, grid, keep):
    """``grid`` nodes over [lo, hi]; the node closest to ``keep`` is replaced by it (None: plain linspace)."""
    x = np.linspace(lo, hi, grid)
    if keep is not None:
        x[int(np.argmin(np.abs(x - keep)))] = keep
    return x


def identify(log, model, free, horizon, starts=None, grid=9, rounds=6, shrink=0.5, base=None, dt_free=None,
             device=0, host_twin=False):
    """Minimise the position cost of ``model``'s rollouts along ``log`` over the fields named by ``free`` =
    {"Cf": (lo, hi), ...} (at most three; "dt", or ``dt_free=(lo, hi)``, makes the fixed step length one of
    them -- otherwise the log's ts is used).  ``base``: the vector the other fields come from (default:
    ``rollout.plant_params()``).  A set one of whose rollouts stopped (non-finite state) costs inf.
    Returns an IdentifyResult."""
    free = dict(free)
    if dt_free is not None:
        if "dt" in free:
            raise ValueError('give the step length either as free["dt"] or as dt_free, not both')
        free["dt"] = dt_free
    names = list(free)
    d = len(names)
    if d < 1 or d > MAX_FREE:
        raise ValueError(f"free names {d} fields; between 1 and {MAX_FREE} are searched")
    unknown = [k for k in names if k != "dt" and k not in rollout.PLANT_FIELDS]
    if unknown:
        raise ValueError(f"unknown plant parameter(s) {unknown}; the fields are {rollout.PLANT_FIELDS} and dt")
    grid, rounds = int(grid), int(rounds)
    if grid < 2 or rounds < 1 or not 0.0 < shrink < 1.0:
        raise ValueError("grid >= 2, rounds >= 1 and 0 < shrink < 1")
    lo0 = np.array([float(free[k][0]) for k in names])
    hi0 = np.array([float(free[k][1]) for k in names])
    if not (np.isfinite(lo0).all() and np.isfinite(hi0).all() and (lo0 < hi0).all()):
        raise ValueError("every bound is a finite (lo, hi) with lo < hi")
    base = rollout.plant_params() if base is None else np.array(base, np.float64)
    lo, hi = lo0.copy(), hi0.copy()
    best_x, best_cost, history = None, np.inf, []
    for _ in range(rounds):
        axes = [_nodes(lo[j], hi[j], grid, None if best_x is None else best_x[j]) for j in range(d)]
        pts = np.array(list(itertools.product(*axes)))  # [grid^d][d], the first field slowest
        params = np.tile(base, (len(pts), 1))
        dt = None
        for j, k in enumerate(names):
            if k == "dt":
                dt = pts[:, j].copy()
            else:
                params[:, rollout.PLANT_FIELDS.index(k)] = pts[:, j]
        r = rollout.plant_rollout_errors(log, model, params, dt=dt, horizon=horizon, starts=starts, device=device,
                                         host_twin=host_twin)
        cost = np.where((r.count == len(r.starts)).all(axis=1), r.position_cost(), np.inf)
        cost = np.where(np.isnan(cost), np.inf, cost)
        i = int(np.argmin(cost))  # the first of equal minima
        if best_x is None or cost[i] < best_cost:  # a tie keeps the earlier point
            best_x, best_cost = pts[i].copy(), float(cost[i])
        history.append(dict(lo=lo.copy(), hi=hi.copy(), n_sets=len(pts), round_min=float(cost[i]),
                            best_values={k: float(best_x[j]) for j, k in enumerate(names)}, best_cost=best_cost))
        half = 0.5 * shrink * (hi - lo)
        lo, hi = np.maximum(best_x - half, lo0), np.minimum(best_x + half, hi0)
    values = {k: float(best_x[j]) for j, k in enumerate(names)}
    params = base.copy()
    for k, v in values.items():
        if k != "dt":
            params[rollout.PLANT_FIELDS.index(k)] = v
    return IdentifyResult(values, params, values.get("dt"), best_cost, history)
