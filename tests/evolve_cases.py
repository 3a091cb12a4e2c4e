"""Shared checks of the GA on the device (csrc/mr_ga.h, pid_segment_vehicle of csrc/mr_pid.h, pid.segment_times,
ga.breed, pid.tune_gains): test_evolve.py runs them on the host build (``KW = dict(host_twin=True)``),
test_gpu_evolve.py on gfx950 (``KW = {}``).  The checker of the breeding is tests/ga_ref.py (numpy, its draws from
numpy.random.Philox), that of the fused timing is ``pid.evaluate_gains`` (the drive's progress row through
``ga.crossing_times``).

Shapes: 9 gain vectors x 8 segments = 72 vehicles (one full wavefront and an 8-lane one) on Shanghai, bounds 100,
130, ..., 340, 70 ticks; breeding of 3 islands at (P, K, D, pairs) = (4, 2, 4, 1), (6, 4, 8, 3), (2, 1, 1, 1), (64,
64, 16, 5); a whole run of 3 generations x 3 islands x 6 individuals on four 30 m segments (72 vehicles).
"""
import ctypes
import functools

import numpy as np

import ga_ref
import pid_cases as pc
from mpcracing import abi, ga, pid, rollout

HOST = dict(host_twin=True)
DT, TICKS = 0.05, 70
BOUNDS = np.arange(100.0, 341.0, 30.0)
NG, K = 9, 8
SHAPES = [(4, 2, 4, 1), (6, 4, 8, 3), (2, 1, 1, 1), (64, 64, 16, 5)]
DEFAULT4 = np.array([0.1, 0.1, 0.82954, 1.21341])


def is_host(KW):
    return bool(KW.get("host_twin"))


# ---- 1. the random stream ----
STREAMS = [(0, 0, 0), (12345, 7, 3), (2 ** 64 - 1, 2 ** 32 + 5, 2 ** 32 - 1), (9, 2 ** 63 + 1, 2 ** 40)]


def philox(seed, island, generation):
    return np.random.Philox(key=np.array([seed, island], np.uint64),
                            counter=np.array([0, 0, generation, 0], np.uint64))


def check_stream(host_twin):
    for seed, island, g in STREAMS:
        ref = philox(seed, island, g).random_raw(14)
        dbl = np.random.Generator(philox(seed, island, g)).random(14)
        for first in (0, 5):
            raw = ga.random(seed, island, g, first, 9, raw=True, host_twin=host_twin)
            assert raw.dtype == np.uint64 and np.array_equal(raw, ref[first:first + 9]), (seed, island, g, first)
            assert pc.same(ga.random(seed, island, g, first, 9, host_twin=host_twin), dbl[first:first + 9])
    assert len(ga.random(1, 2, 3, 4, 0, host_twin=host_twin)) == 0
    a, b = (ga.random(3, i, 0, 0, 8, raw=True, host_twin=host_twin) for i in (0, 1))
    assert not np.any(a == b)  # the island keys the stream


# ---- 2. segment times fused into the drive ----
@functools.lru_cache(maxsize=None)
def population():
    """[9][4] within 30 % of the agent's defaults (seeded)"""
    rng = np.random.default_rng(20250107)
    return DEFAULT4 * (1 + 0.3 * rng.uniform(-1, 1, (NG, 4)))


@functools.lru_cache(maxsize=None)
def vehicle_params():
    """[72][22]: mass, stiffnesses and inertia within 10 % of the defaults (seeded)"""
    rng = np.random.default_rng(20250108)
    q = np.tile(rollout.plant_params(), (NG * K, 1))
    for f in ("m", "Cf", "Cr", "Iz"):
        q[:, rollout.PLANT_FIELDS.index(f)] *= 1 + 0.1 * rng.uniform(-1, 1, NG * K)
    return q


def params(shared):
    return None if shared else vehicle_params()


@functools.lru_cache(maxsize=None)
def _reference(model, shared, host, ticks):
    KW = HOST if host else {}
    times, res = pid.evaluate_gains(pc.track(pc.SHANGHAI, KW), population(), BOUNDS, ticks, model=model,
                                    params=params(shared), dt=DT, **KW)
    times.setflags(write=False)
    return times, crossing_ticks(res.rows["progress"], BOUNDS, NG)


def reference(model, shared, KW, ticks=TICKS):
    """(times [9][8], crossing tick [9][8], -1 for none) of the parent path, once per backend"""
    return _reference(model, shared, is_host(KW), ticks)


def crossing_ticks(prog, bounds, G):
    """the tick of ga.crossing_times' first hit, [G][K] (-1: none)"""
    L = float(pc.G[pc.SHANGHAI + "/L"])
    s0, s1 = np.tile(bounds[:-1], G), np.tile(bounds[1:], G)
    tr = np.mod(prog - s0[None, :], L)
    tr = np.where(tr > 0.5 * L, tr - L, tr)
    hit = tr >= np.mod(s1 - s0, L)[None, :]
    return np.where(hit.any(0), hit.argmax(0), -1).reshape(G, -1)


def seg(KW, gains=None, bounds=BOUNDS, ticks=TICKS, model="blend", shared=False, q=None):
    return pid.segment_times(pc.track(pc.SHANGHAI, KW), population() if gains is None else gains, bounds, ticks,
                             model=model, params=params(shared) if q is None else q, dt=DT, **KW)


LONG = 150  # ticks within which every vehicle of the shape finishes (the slowest needs 103)


def check_fused_equals_evaluate_gains(model, shared, KW):
    """On the segment at 160 m (a corner) some vehicles of the blended plant need more than the 70 ticks: they are
    inf on both sides at 70 ticks, and the run capped at 4096 ticks is checked for every vehicle against the parent
    path at 150 ticks, where all have finished."""
    ref, tick = reference(model, shared, KW)
    times, done = seg(KW, model=model, shared=shared)
    assert times.shape == (NG, K) and done.shape == (NG, K) and done.dtype == np.int32
    fin = np.isfinite(ref)
    assert fin.sum() >= NG * K - 4 and np.all(tick[fin] > 0) and np.all(tick[~fin] == -1)
    assert pc.same(times, ref)
    assert pc.same(done, np.where(fin, tick + 1, TICKS))
    assert len(np.unique(done)) > 3  # lanes of one wave finish at different ticks
    # the early exit is real and the cap does not enter
    ref_long, tick_long = reference(model, shared, KW, LONG)
    assert np.isfinite(ref_long).all() and tick_long.max() < LONG - 1
    t_cap, d_cap = seg(KW, ticks=4096, model=model, shared=shared)
    assert pc.same(t_cap, ref_long) and pc.same(d_cap, tick_long + 1)
    assert pc.same(t_cap[fin], times[fin]) and pc.same(d_cap[fin], done[fin])


def check_unfinished_and_zero_length(KW):
    ref, _ = reference("blend", False, KW)
    # a segment no vehicle finishes in 70 ticks
    b = BOUNDS.copy()
    b[-1] = 2000.0
    t, d = seg(KW, bounds=b)
    assert np.all(np.isinf(t[:, -1])) and np.all(d[:, -1] == TICKS)
    assert pc.same(t[:, :-1], ref[:, :-1])
    # zero-length segments: need = 0.  Where the first projection lands at or ahead of the start the first hit is
    # tick 0 and the time inf, as in ga.crossing_times; where it lands behind it (by less than the projection's
    # 1e-5 tolerance) tick 0 is no hit and crossing_times interpolates inside tick 1.  The fused timing follows
    # the parent path bit for bit in both; the starts below show both
    tr = pc.track(pc.SHANGHAI, KW)
    seen = set()
    for s in (100.0, 114.0, 128.0, 156.0):
        b = np.array([s - 30.0, s, s, s + 30.0])
        t, d = seg(KW, bounds=b, shared=True)
        e, res = pid.evaluate_gains(tr, population(), b, TICKS, dt=DT, **KW)
        first_hit = crossing_ticks(res.rows["progress"], b, NG)[:, 1]
        assert pc.same(t, e) and pc.same(d[:, 1], first_hit + 1) and np.all((first_hit == 0) | (first_hit == 1))
        assert np.all(np.isinf(t[first_hit == 0, 1]))
        assert np.all((t[first_hit == 1, 1] >= 0) & (t[first_hit == 1, 1] < 1e-6))
        seen |= set(first_hit.tolist())
    assert seen == {0, 1}


def check_nan_gains_stop_their_vehicles_only(KW, row=4):
    ref, _ = reference("blend", False, KW)
    base_t, base_d = seg(KW)
    g = pid._full_gains(population())
    g[row, 4] = np.nan
    t, d = seg(KW, gains=g)
    others = np.arange(NG) != row
    assert np.all(np.isinf(t[row])) and np.all(d[row] == 0)
    assert pc.same(t[others], ref[others]) and pc.same(d[others], base_d[others])


def check_repeatable_and_alone(KW, row=3):
    t, d = seg(KW)
    t2, d2 = seg(KW)
    assert pc.same(t, t2) and pc.same(d, d2)
    ta, da = seg(KW, gains=population()[row:row + 1], q=vehicle_params()[row * K:(row + 1) * K])
    assert ta.shape == (1, K) and pc.same(ta[0], t[row]) and pc.same(da[0], d[row])
    # shared parameters = copies of the vector
    ts, ds = seg(KW, shared=True)
    tc, dc = seg(KW, q=np.tile(rollout.plant_params(), (NG * K, 1)))
    assert pc.same(ts, tc) and pc.same(ds, dc)


def check_timing_against_host(model, KW, tol=1e-6):
    """the drive's existing bar between the device and the host build"""
    t, d = seg(KW, model=model)
    th, dh = seg(HOST, model=model)
    fin = np.isfinite(th)  # (pc.close takes no inf: the unfinished vehicles are compared as such)
    assert pc.same(np.isinf(t), ~fin) and pc.close(t[fin], th[fin], tol) and pc.same(d, dh)


# ---- 3. breeding against ga_ref ----
@functools.lru_cache(maxsize=None)
def breed_inputs(shape):
    """(genes [3][P][D], times [3][P][K] with about a tenth inf, avg [3][K]), seeded by the shape"""
    P, Kk, D, pairs = shape
    rng = np.random.default_rng([20250109, P, Kk, D])
    genes = rng.uniform(0, 1, (3, P, D))
    times = rng.uniform(1.5, 2.5, (3, P, Kk))
    times[rng.uniform(size=times.shape) < 0.1] = np.inf
    avg = rng.uniform(1.8, 2.2, (3, Kk))
    for a in (genes, times, avg):
        a.setflags(write=False)
    return genes, times, avg


def against_ref(out, genes, times, avg, island0=0, tol=1e-12, **kw):
    """Rewards and averages within tol (exp differs by ulps between libm, numpy and the device); then, decided on
    the rewards the library returned, the reference's new genes bit for bit -- which holds the parents, the
    crossover points, the mutation flags and values, the clip and the replaced rows at once, the genes being
    distinct random numbers -- the rows that changed and the recorded best."""
    for i in range(genes.shape[0]):
        ref = ga_ref.breed(genes[i], times[i], avg[i], island=island0 + i, r=out.r[i], **kw)
        assert np.all(np.abs(out.r[i] - ref["r"]) <= tol * np.abs(ref["r"])), i
        assert np.all(np.abs(out.avg[i] - ref["avg"]) <= tol * np.abs(ref["avg"])), i
        assert pc.same(out.genes[i], ref["genes"]), (i, ref["parents"], ref["points"], ref["replaced"])
        changed = np.nonzero(np.any(out.genes[i] != genes[i], axis=1))[0]
        assert set(changed) <= set(ref["replaced"])
        assert out.best_idx[i] == ref["best"][1] and out.best_r[i] == out.r[i][ref["best"][1]]
        assert pc.same(out.best_genes[i], ref["best"][2])
    return out


def check_breed(shape, KW):
    P, Kk, D, pairs = shape
    genes, times, avg = breed_inputs(shape)
    kw = dict(pairs=pairs, seed=20250110, generation=5)
    out = against_ref(ga.breed(genes, times, avg, **kw, **KW), genes, times, avg, **kw)
    assert out.genes.shape == (3, P, D) and out.r.shape == (3, P) and out.avg.shape == (3, Kk)
    assert np.all(out.r >= 0) and np.isfinite(out.r).all()
    # island 2 alone is island 2 of the batch
    one = ga.breed(genes[2], times[2], avg[2], island0=2, **kw, **KW)
    for name in ("genes", "r", "avg", "best_r", "best_idx", "best_genes"):
        assert pc.same(getattr(one, name), getattr(out, name)[2]), name
    # two calls are equal; the next generation draws differently
    again = ga.breed(genes, times, avg, **kw, **KW)
    assert pc.same(again.genes, out.genes) and pc.same(again.r, out.r)
    nxt = ga.breed(genes, times, avg, **dict(kw, generation=6), **KW)
    assert pc.same(nxt.r, out.r) and not pc.same(nxt.genes, out.genes)
    against_ref(nxt, genes, times, avg, **dict(kw, generation=6))


def check_breed_edges(KW):
    shape = (6, 4, 8, 3)
    genes, times, avg = breed_inputs(shape)
    kw = dict(pairs=3, seed=77, generation=1)
    # every time inf: r = 0, uniform selection, the averages stay, the replacement runs through indices 0..5
    inf = np.full(times.shape, np.inf)
    out = against_ref(ga.breed(genes, inf, avg, **kw, **KW), genes, inf, avg, **kw)
    assert np.all(out.r == 0) and pc.same(out.avg, avg) and np.all(out.best_idx == 0)
    # equal rewards: individuals 1 and 4 finish nothing (r = 0 both), 4 takes the later child
    t = np.array(times)
    t[~np.isfinite(t)] = 2.0
    t[:, 1] = np.inf
    t[:, 4] = np.inf
    kw1 = dict(kw, pairs=1)
    out = against_ref(ga.breed(genes, t, avg, **kw1, **KW), genes, t, avg, **kw1)
    for i in range(3):
        ref = ga_ref.breed(genes[i], t[i], avg[i], island=i, r=out.r[i], **kw1)
        assert list(ref["replaced"]) == [1, 4] and out.r[i][1] == 0 and out.r[i][4] == 0
        assert not pc.same(out.genes[i][1], genes[i][1]) and not pc.same(out.genes[i][4], genes[i][4])
    # bounds that clip: mutation moves a gene by up to 0.5, the genes lie in [0, 1)
    lo = np.array([0.3, np.nan, 0.3, 0.45, np.nan, 0.0, 0.3, 0.3])
    hi = np.array([0.6, 0.5, np.nan, 0.55, np.nan, 1.0, 0.6, 0.6])
    kwb = dict(kw, lo=lo, hi=hi)
    out = against_ref(ga.breed(genes, times, avg, **kwb, **KW), genes, times, avg, **kwb)
    free = ga.breed(genes, times, avg, **kw, **KW)
    assert not pc.same(out.genes, free.genes)  # some gene was clipped
    for i in range(3):
        kids = np.any(out.genes[i] != genes[i], axis=1)
        assert np.all(out.genes[i][kids][:, [0, 2, 3, 6, 7]] >= lo[[0, 2, 3, 6, 7]])
        assert np.all(out.genes[i][kids][:, [0, 1, 3, 6, 7]] <= hi[[0, 1, 3, 6, 7]])
    # scalars bound every gene
    out = against_ref(ga.breed(genes, times, avg, **dict(kw, lo=0.4, hi=0.6), **KW), genes, times, avg,
                      **dict(kw, lo=0.4, hi=0.6))


def check_breed_against_host(KW):
    """identical input times: the decisions and the genes are identical on the two builds"""
    for shape in SHAPES:
        genes, times, avg = breed_inputs(shape)
        kw = dict(pairs=shape[3], seed=31, generation=2)
        dev, host = ga.breed(genes, times, avg, **kw, **KW), ga.breed(genes, times, avg, **kw, **HOST)
        assert pc.same(dev.genes, host.genes) and pc.same(dev.best_idx, host.best_idx)
        assert pc.same(dev.best_genes, host.best_genes)
        assert pc.close(dev.r, host.r, 1e-12) and pc.close(dev.avg, host.avg, 1e-12)


# ---- 4. end to end ----
TUNE_BOUNDS = np.arange(190.0, 311.0, 30.0)  # four 30 m segments after the slow corner at 160 m
TUNE = dict(generations=3, islands=3, population=6, pairs=1)
# Gene bounds within which the drives stay finite on these segments (tried on the host build: with the reference's
# uniform [0, 1) population some vehicles never reach the end of a segment), and a first population
# inside them
TUNE_LO, TUNE_HI = 0.5 * DEFAULT4, 1.5 * DEFAULT4


def tune_init(seed):
    u = np.random.Generator(philox(seed, 0, 123)).random((3, 6, 4))
    return TUNE_LO + (TUNE_HI - TUNE_LO) * u


def tune(KW, seed=5, **kw):
    return pid.tune_gains(pc.track(pc.SHANGHAI, KW), TUNE_BOUNDS, seed=seed, init=tune_init(seed), lo=TUNE_LO,
                          hi=TUNE_HI, ticks=TICKS, dt=DT, keep_times=True, **dict(TUNE, **kw), **KW)


def tune_same(a, b):
    for name in ("population", "gains", "best_reward", "best_index", "best_genes", "avg", "rewards", "ticks_done",
                 "times"):
        assert pc.same(getattr(a, name), getattr(b, name)), name


def check_tune(KW):
    tr = pc.track(pc.SHANGHAI, KW)
    res = tune(KW)
    I, P, G, D, Kk = 3, 6, 3, 4, 4
    assert res.times.shape == (G, I, P, Kk) and res.population.shape == (I, P, D) and res.gains.shape == (I, P, 8)
    assert np.isfinite(res.times).all()  # the precondition of the rewards below
    # the same three generations as separate calls with synchronises in between
    genes = tune_init(5)
    avg = np.full((I, Kk), TICKS * DT / 2)
    for g in range(G):
        full = np.tile(pid.gains(), (I * P, 1))
        full[:, 2:6] = genes.reshape(I * P, D)
        t, d = pid.segment_times(tr, full, TUNE_BOUNDS, TICKS, dt=DT, **KW)
        assert pc.same(res.times[g], t.reshape(I, P, Kk)), g
        if g == 0:  # the parent path on the initial population
            assert pc.same(pid.evaluate_gains(tr, genes.reshape(I * P, D), TUNE_BOUNDS, TICKS, dt=DT, **KW)[0], t)
        out = ga.breed(genes, t.reshape(I, P, Kk), avg, pairs=1, lo=TUNE_LO, hi=TUNE_HI, seed=5, generation=g, **KW)
        assert pc.same(res.best_reward[g], out.best_r) and pc.same(res.best_index[g], out.best_idx)
        assert pc.same(res.best_genes[g], out.best_genes)
        genes, avg = out.genes, out.avg
    assert pc.same(res.population, genes) and pc.same(res.avg, avg) and pc.same(res.rewards, out.r)
    assert pc.same(res.ticks_done, d.reshape(I, P, Kk))
    assert pc.same(res.gains[:, :, 2:6], genes) and pc.same(res.gains[:, :, [0, 1, 6, 7]],
                                                            np.broadcast_to(pid.gains()[[0, 1, 6, 7]], (I, P, 4)))
    assert np.all(np.isfinite(res.best_reward) & (res.best_reward > 0))
    assert np.all(res.population >= TUNE_LO) and np.all(res.population <= TUNE_HI)
    # the same seed again; another seed
    tune_same(res, tune(KW))
    other = pid.tune_gains(tr, TUNE_BOUNDS, seed=6, init=tune_init(5), lo=TUNE_LO, hi=TUNE_HI, ticks=TICKS, dt=DT,
                           keep_times=True, **TUNE, **KW)
    assert pc.same(other.times[0], res.times[0]) and not pc.same(other.population, res.population)
    # without keep_times nothing else changes
    lean = pid.tune_gains(tr, TUNE_BOUNDS, seed=5, init=tune_init(5), lo=TUNE_LO, hi=TUNE_HI, ticks=TICKS, dt=DT,
                          **TUNE, **KW)
    assert lean.times is None and pc.same(lean.population, res.population) and pc.same(lean.avg, res.avg)


def check_tune_default_population(KW):
    """init=None: uniform [0, 1) of the stream (seed, island, 2**32 - 1); other genes and a given average"""
    tr = pc.track(pc.SHANGHAI, KW)
    names = ("kP_throttle", "lookahead")
    res = pid.tune_gains(tr, TUNE_BOUNDS[:3], 1, islands=2, population=4, seed=9, genes=names, avg0=[1.9, 2.1],
                         keep_times=True, ticks=TICKS, dt=DT, **KW)
    pop = np.stack([np.random.Generator(philox(9, i, 2 ** 32 - 1)).random((4, 2)) for i in range(2)])
    full = np.tile(pid.gains(), (8, 1))
    full[:, [4, 6]] = pop.reshape(8, 2)
    t, _ = pid.segment_times(tr, full, TUNE_BOUNDS[:3], TICKS, dt=DT, **KW)
    assert pc.same(res.times[0], t.reshape(2, 4, 2))
    out = ga.breed(pop, t.reshape(2, 4, 2), np.tile([1.9, 2.1], (2, 1)), seed=9, generation=0, **KW)
    assert pc.same(res.population, out.genes) and pc.same(res.avg, out.avg) and res.genes == list(names)
    assert pc.same(res.gains[:, :, [0, 1, 2, 3, 5, 7]], np.broadcast_to(pid.gains()[[0, 1, 2, 3, 5, 7]], (2, 4, 6)))


# ---- 5. argument errors ----
def raises(fn, text):
    try:
        fn()
    except RuntimeError as e:
        assert text in str(e) and "error -1:" in str(e), (text, str(e))  # MR_ERR_ARG and its message
    else:
        raise AssertionError(f"accepted: {text}")


def check_segment_errors(KW):
    def drive(**kw):
        sd = pid._SegmentDrive(pc.track(pc.SHANGHAI, KW), BOUNDS, NG, 15.0, "blend", None, DT, is_host(KW), 0)
        be = sd.be
        a = dict(g=be.put(pid._full_gains(population())), t=be.empty((sd.n,)), d=be.empty((sd.n,), np.int32),
                 ticks=TICKS)
        for k, v in kw.items():
            if k in a:
                a[k] = v
            else:
                setattr(sd, k, v)
        sd.launch(a["g"], a["ticks"], a["t"], a["d"])
        sd.sync()

    drive()
    raises(lambda: drive(n=NG * K + 1), "n must be a multiple of K")
    raises(lambda: drive(K=0), "K < 1")
    raises(lambda: drive(n=-8), "n < 0")
    raises(lambda: drive(ticks=0), "T < 1")
    raises(lambda: drive(ticks=4097), "T > 4096")
    for bad in (0.0, -0.05, np.nan, np.inf):
        raises(lambda: drive(dt=bad), "dt must be a positive finite number")
    raises(lambda: drive(model_id=3), "unknown plant model")
    raises(lambda: drive(P=2), "P must be 1")
    for name in ("g", "t", "d", "start", "s_start", "s_end", "q"):
        raises(lambda: drive(**{name: None}), "null argument")


def check_breed_errors(KW):
    from mpcracing.tyrefit import _Device, _Host
    host = is_host(KW)

    def call(dims=(3, 6, 4, 8, 3), ld=8, col=None, null=None):
        genes, times, avg = breed_inputs((6, 4, 8, 3))
        be = _Host() if host else _Device(0)
        a = dict(genes=be.put(np.array(genes)), times=be.put(times), avg=be.put(np.array(avg)), r=be.empty((3, 6)),
                 best_r=be.empty((3,)), best_idx=be.empty((3,), np.int32), best_genes=be.empty((3, 8)))
        if null:
            a[null] = None
        ga.breed_launch(be, host, dims, a["genes"], ld, col, a["times"], a["avg"], None, (4.0, 0.3, 0.4), 1, 0, 0,
                        a["r"], a["best_r"], a["best_idx"], a["best_genes"])
        if not host:
            be.torch.cuda.synchronize(be.dev)

    call()
    raises(lambda: call(dims=(3, 1, 4, 8, 1)), "P outside 2..64")
    raises(lambda: call(dims=(3, 65, 4, 8, 1)), "P outside 2..64")
    raises(lambda: call(dims=(3, 6, 0, 8, 3)), "K outside 1..64")
    raises(lambda: call(dims=(3, 6, 65, 8, 3)), "K outside 1..64")
    raises(lambda: call(dims=(3, 6, 4, 0, 3)), "D outside 1..16")
    raises(lambda: call(dims=(3, 6, 4, 17, 3)), "D outside 1..16")
    raises(lambda: call(dims=(3, 6, 4, 8, 0)), "pairs < 1")
    raises(lambda: call(dims=(3, 6, 4, 8, 4)), "2 pairs > P")
    raises(lambda: call(dims=(-1, 6, 4, 8, 3)), "n_island < 0")
    raises(lambda: call(ld=7), "ld < D")
    raises(lambda: call(col=(ctypes.c_int32 * 8)(0, 1, 2, 3, 4, 5, 6, 8)), "col entry outside")
    raises(lambda: call(col=(ctypes.c_int32 * 8)(0, 1, 2, 3, 4, 5, 6, 6)), "col entries must be distinct")
    for name in ("genes", "times", "avg", "r", "best_r", "best_idx", "best_genes"):
        raises(lambda: call(null=name), "null argument")
    assert abi.MR_GA_P_MAX == 64 and abi.MR_GA_K_MAX == 64 and abi.MR_GA_D_MAX == 16
