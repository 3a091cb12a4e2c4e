"""The GA step of csrc/mr_ga.h restated in numpy (the checker of tests/evolve_cases.py): the rules of
include/mpcracing.h's mr_ga_breed in their order, the draws taken from ``numpy.random.Philox`` directly.

The operators are GA/pdGA.py's (select_parents :57-62 as its cumulative-sum search, crossover :64-69, mutate
:71-76, the replacement of np.argsort(rewards)[:2] at :87, np.argmax at :89), the rewards GA/mpcGA.py:40-56 as
mpcracing.ga.rewards states them, with the one stated addition that an unfinished segment is skipped.
"""
import numpy as np


def draws(seed, island, generation, count):
    """the first ``count`` doubles of the stream: Generator.random() of Philox(key, counter)"""
    bg = np.random.Philox(key=np.array([seed, island], np.uint64), counter=np.array([0, 0, generation, 0], np.uint64))
    return np.random.Generator(bg).random(count)


def rewards(times, avg, kT=4.0, lambda_T=0.3):
    """(r [P], the updated avg [K]): ga.rewards with non-finite times skipped"""
    avg = np.array(avg, np.float64)
    P, K = times.shape
    r = np.zeros(P)
    for i in range(P):
        for k in range(K):
            t, a = times[i, k], avg[k]
            if np.isfinite(t):
                avg[k] = lambda_T * t + (1 - lambda_T) * a
                r[i] += np.exp(-kT * (t - a))
    return r, avg


def select(r, u):
    """roulette: the first j with u cdf[-1] < cdf[j] (the last if none); uniform when the sum is 0 or not finite"""
    P = len(r)
    cdf = np.zeros(P)
    c = 0.0
    for i in range(P):
        c = c + r[i]
        cdf[i] = c
    if cdf[-1] == 0.0 or not np.isfinite(cdf[-1]):
        return int(np.floor(u * P))
    hit = np.nonzero(u * cdf[-1] < cdf)[0]
    return int(hit[0]) if len(hit) else P - 1


def breed(genes, times, avg, pairs=1, lo=None, hi=None, kT=4.0, lambda_T=0.3, mutation_rate=0.4, seed=0, island=0,
          generation=0, r=None):
    """One island's generation.  ``r``: rewards to decide with instead of this function's own (the library's, so
    that ulps of exp cannot move a decision).  Returns a dict: r, avg, parents [pairs][2], points [pairs], flags
    [pairs][2][D] (bool), replaced [2 pairs], genes [P][D], best = (reward, index, genes)."""
    genes = np.array(genes, np.float64)
    P, D = genes.shape
    r_own, avg_new = rewards(np.asarray(times, np.float64), avg, kT, lambda_T)
    r = r_own if r is None else np.asarray(r, np.float64)
    u = draws(seed, island, generation, pairs * (3 + 4 * D))
    parents, points, flags, children = [], [], [], []
    for m in range(pairs):
        d = u[m * (3 + 4 * D):(m + 1) * (3 + 4 * D)]
        a, b = select(r, d[0]), select(r, d[1])
        pt = 1 + int(np.floor(d[2] * (D - 1)))
        kids = [np.concatenate([genes[a][:pt], genes[b][pt:]]), np.concatenate([genes[b][:pt], genes[a][pt:]])]
        fl = []
        for c in range(2):
            f = d[3 + 2 * D * c:3 + 2 * D * c + D] < mutation_rate
            v = d[3 + 2 * D * c + D:3 + 2 * D * c + 2 * D] - 0.5
            kid = kids[c].copy()
            kid[f] = kid[f] + v[f]
            if lo is not None:
                lo_ = np.broadcast_to(np.asarray(lo, np.float64), (D,))
                kid = np.where(~np.isnan(lo_) & (kid < lo_), lo_, kid)
            if hi is not None:
                hi_ = np.broadcast_to(np.asarray(hi, np.float64), (D,))
                kid = np.where(~np.isnan(hi_) & (kid > hi_), hi_, kid)
            fl.append(f)
            children.append(kid)
        parents.append((a, b))
        points.append(pt)
        flags.append(fl)
    replaced = np.argsort(r, kind="stable")[:2 * pairs]
    best = int(np.argmax(r))
    new = genes.copy()
    for q, i in enumerate(replaced):
        new[i] = children[q]
    return dict(r=r_own, avg=avg_new, parents=np.array(parents), points=np.array(points), flags=np.array(flags),
                replaced=replaced, genes=new, best=(r[best], best, genes[best].copy()))
