"""Generate tests/golden/shift_golden.npz / .json: the dense IPOPT oracle's first 12 iterations on C3 instances
that accept a large inertia shift at once, with the compared rows selected by the scalar build alone.

TEST FIXTURE GENERATOR (CPU only; the GPU box never runs the oracle's solves).

Why a third fixture.  make_ipopt_trace_golden.py and make_config_grid_golden.py compare only the rows on which BOTH
host builds (the scalar Solver and the emulated wavefront) sit within 1e-8 of the oracle (n_cmp_rule), and their
cases were chosen so that this prefix is long.  A loss of accuracy that only the wave path has shortens n_cmp or
drops the case; it fails nothing.  Here the rows are selected by the scalar build only -- the yardstick the scalar
build exists to be -- and the wave builds (the host emulation in tests/test_shift.py, gfx950 in
tests/test_gpu_shift.py) are then held to the oracle on those rows at the bars of tests/ipopt_trace_cases.py.

Options, rel_dev, the column maps, the host solve and the oracle recipe (solve_ipopt(..., log=True, rules=PRODUCT) on
oracle.nlp.MPCProblem) are make_ipopt_trace_golden.py's, imported from it.  Per case the fixture keeps, in that
generator's layout so that ipopt_trace_cases.check_rows(case, trace, label, fx=...) applies unchanged,
  <case>/log         [12][7]: kkt, mu, alpha, delta, theta, phi, in_resto of every logged iteration; kkt and theta
                     restated over unscaled rows (below)
  <case>/log_scaled  [12][2]: kkt and theta of the same rows exactly as the oracle logged them (scaled rows)
  <case>/in_*        the instance's inputs (B = 1, ABI layout), to check that mpcracing.workload still makes them
and, in the json index, instance / lane_bounds / options, the oracle's status and iterations, n_cmp, the row-0 and
largest shift, the oracle's largest constraint-row gradient at the start and its smallest row scale, and the worst
deviation of the scalar and of the wave host build per column over the n_cmp rows (``scalar_worst_dev``,
``wave_worst_dev``: the wave's is recorded, not asserted -- it was up to 0.56 in alpha until the Riccati sweep's
cost-to-go tile was made symmetric, mr_wave.h frag_plan and DESIGN.md §4, and the tests hold it to 1e-6).

Cases.  All are mpcracing.workload.make_batch("C3") instances (dynamic model, N = 40) at PREFIX_OPT with max_iter 12.
  shift      79, 67, 62, 57, 33 (of instances 0..95; row-0 delta 100, instance 62: 1) and 2754, 6258, 3734, 5287,
             6101, 7151, 3022 (row-0 delta 100, 6258: 1); all slow cars (vx 5 to 11 m/s) under braking
  no lane    79 and 67 again with lane_bounds off
  controls   0 and 3: row-0 delta 100 as well, vx 14.8 and 14.5 m/s; both host builds within 3e-9 on all 12 rows
Instances 94 and 60, which the list first held, miss the condition below and were replaced, not the condition
shortened: on 94 the scalar build is 2.4e-7 from the oracle in alpha at row 7 (n_cmp 7, with and without lane rows),
on 60 4.8e-5 at row 6 (n_cmp 6).  67 and 57 take their places: the same segment's slow cars with row-0 delta 100
(the wave build of the time left the oracle at row 3 and row 2 there), and 67 takes 94's place without lane rows.

Compared rows.  n_cmp is the longest prefix of non-restoration rows on which the SCALAR build alone is within
N_CMP_RTOL = 1e-7 relative of the oracle in alpha, theta (plus 1e-10 absolute) and kkt -- 10 times inside the tests'
1e-6 -- with mu and delta within 1e-12.  Asserted: n_cmp >= MIN_N_CMP = 8 for every case.

kkt and theta: which quantity.  IPOPT scales every constraint row whose gradient at the starting point exceeds
nlp_scaling_max_gradient = 100 down to 100 (oracle.ipopt._scaled: dc_i = 100 / max_j |dc_i/dx_j|), and the oracle,
like IPOPT, measures theta = |c|_1 + |d - s|_1 and the constraint-violation term of the optimality error on the
SCALED rows.  The solver builds take every row scale as 1 (DESIGN.md §2 "Scaling and start").  That holds wherever
the car is not slow: of the cases above the largest row gradient is at most 72 for 79's neighbours 62, 57, 67 and for
2754, 6258, 7151, 3022, 0 and 3, and the two logs agree to 1e-10.  On 79, 33, 3734, 5287 and 6101 (gradients 114 to
368: a dynamics row of a car at 5 to 9 m/s) dc falls to between 0.85 and 0.27, and from row 1 on -- row 0 is a rollout,
its dynamics rows are met -- the logged theta differs from both builds' by 1e-3 to 2e-1 and, where the violation
is the largest term of the error, kkt by 1e-5, while alpha, mu and delta agree to 1e-9: the Newton step does not
depend on the row scales, so the iterates are the same and the two logs state two different quantities.  (The line
search's reference point after a rejected or watchdog step and the lane slack rows, the other candidates, are not
it: no step is rejected in these rows, and the difference is there without lane rows.)
    The generator therefore logs the quantity the builds log: in the worker process oracle.ipopt._Alg.measure is
wrapped so that every evaluated point also yields theta and the optimality error over unscaled rows (c / dc; the
multiplier sum of s_d over y_c dc; dd = 1 is asserted, no inequality row is scaled), and <case>/log holds those in
its kkt and theta columns for the very rows -- the same iterates, the same reference points -- that the oracle
logged; <case>/log_scaled keeps the oracle's own two columns.  No column is dropped, and no row: every case is
compared in alpha, theta, kkt, mu and delta on all its n_cmp rows.  That the solver's filter and error use unscaled
rows where IPOPT's use scaled ones is a gap of the restatement itself (both builds alike); it moved no
step size in these rows.

Usage: python tests/golden/make_shift_golden.py        (under a minute, 8 worker processes)
"""
import contextlib
import importlib.util
import json
import os
import sys
import time

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(_v, "1")  # one thread per worker process: the dense solves are small

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(REPO, "mpc-racing_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)


def _trace_generator():
    spec = importlib.util.spec_from_file_location("make_ipopt_trace_golden",
                                                  os.path.join(HERE, "make_ipopt_trace_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = _trace_generator()  # options, columns, rel_dev, the host solve and the oracle recipe: one definition
TRACE_COL, LOG_COL, IN_KEYS, THETA_ATOL = T.TRACE_COL, T.LOG_COL, T.IN_KEYS, T.THETA_ATOL

NPZ = os.path.join(HERE, "shift_golden.npz")
INDEX = os.path.join(HERE, "shift_golden.json")
MAX_BYTES = 100 * 1024

K_SHIFT = 12
OPT = dict(T.PREFIX_OPT, max_iter=K_SHIFT)
N_CMP_RTOL = 1e-7
MIN_N_CMP = 8
CONFIG = "C3"
SHIFT = (79, 67, 62, 57, 33, 2754, 6258, 3734, 5287, 6101, 7151, 3022)
NO_LANE = (79, 67)
CONTROLS = (0, 3)
REPLACED = {94: 67, 60: 57}  # listed first, missed n_cmp >= 8 (module docstring)


def _cases():
    out = {f"C3_{i}": dict(instance=i, lane=True, kind="shift") for i in SHIFT}
    out.update({f"C3_{i}_nolane": dict(instance=i, lane=False, kind="shift") for i in NO_LANE})
    out.update({f"C3_{i}": dict(instance=i, lane=True, kind="control") for i in CONTROLS})
    return out


CASES = _cases()
_batch = {}


def batch(limit=None):
    """mpcracing.workload.make_batch("C3") up to the last instance used (made once per process)."""
    from mpcracing import workload as wl
    if "b" not in _batch:
        _batch["b"] = wl.make_batch(CONFIG, limit=max(s["instance"] for s in CASES.values()) + 1)
    return _batch["b"]


def case_config(case):
    from mpcracing import workload as wl
    return dict(wl.CONFIGS[CONFIG], lane=CASES[case]["lane"])


def take(b, instances):
    """Columns ``instances`` of the batch ``b`` as a batch of their own (ABI layout)."""
    idx = np.asarray(instances)
    return {k: (np.ascontiguousarray(v[..., idx]) if v is not None else None) for k, v in b.items()}


def case_inputs(case):
    """The case's instance as a batch of one (ABI layout), made by mpcracing.workload."""
    return take(batch(), [CASES[case]["instance"]])


def host_solve(case, scalar):
    return T.host_solve(case_config(case), case_inputs(case), OPT, scalar)


@contextlib.contextmanager
def unscaled_columns(table):
    """oracle.ipopt._Alg.measure wrapped (this process only, restored afterwards): ``table`` maps every theta and
    every optimality error the oracle evaluates to the same quantity over unscaled rows (module docstring)."""
    from oracle import ipopt as oi
    orig = oi._Alg.measure

    def measure(self, it):
        E = orig(self, it)
        if self.resto is None and self.dc is not None:
            dc = self.dc
            assert np.all(self.dd == 1.0)  # no inequality row is scaled: only c / dc and y_c dc change
            c = np.abs(E["ev"]["c"] / dc)
            rd = np.abs(E["rd"])
            bsum = np.abs(it.vL[self.mL]).sum() + np.abs(it.vU[self.mU]).sum() + np.abs(it.zL[self.mx]).sum()
            nb = int(self.mL.sum() + self.mU.sum() + self.mx.sum())
            yd = E["yd"]
            ysum = np.abs(it.yc * dc).sum() + (np.abs(yd).sum() if self.R.sd_count_yd else 0.0)
            ny = it.yc.size + (yd.size if self.R.sd_count_yd else 0)
            s_d = max(100.0, (ysum + bsum) / max(ny + nb, 1)) / 100.0
            viol = max(c.max(initial=0.0), E["viol_d"].max(initial=0.0))
            pr = max(c.max(initial=0.0), rd.max(initial=0.0))
            table["theta", E["theta"]] = float(c.sum() + rd.sum())
            table["kkt", E["nlp_err"]] = max(E["dual_inf"] / s_d, viol if self.R.nlp_error_viol else pr,
                                             E["compl"](0.0) / E["s_c"])
            table["min_row_scale"] = float(dc.min())
        return E

    oi._Alg.measure = measure
    try:
        yield
    finally:
        oi._Alg.measure = orig


def _oracle(case):
    table = {}
    t0 = time.time()
    with unscaled_columns(table):
        _p, r = T.oracle_solve(case_config(case), case_inputs(case), OPT)
    scaled = T.log_rows(r)
    log = scaled.copy()
    log[:, LOG_COL["kkt"]] = [table["kkt", v] for v in scaled[:, LOG_COL["kkt"]]]
    log[:, LOG_COL["theta"]] = [table["theta", v] for v in scaled[:, LOG_COL["theta"]]]
    return dict(log=log, log_scaled=scaled[:, [LOG_COL["kkt"], LOG_COL["theta"]]].copy(), status=int(r.status),
                iters=int(r.iters), max_row_gradient=float(r.max_row_gradient), min_row_scale=table["min_row_scale"],
                seconds=time.time() - t0)


def deviations(log, trace):
    """Per-row relative deviation of a build's trace from the oracle's log, per compared column."""
    n = len(log)
    return {col: T.rel_dev(trace[:n, TRACE_COL[col]], log[:, LOG_COL[col]], THETA_ATOL if col == "theta" else 0.0)
            for col in ("alpha", "theta", "kkt", "mu", "delta")}


def scalar_n_cmp(log, trace, label=""):
    """n_cmp from the scalar build's ``trace`` alone: the longest prefix of non-restoration rows within N_CMP_RTOL
    of the oracle in alpha, theta and kkt; mu and delta asserted within 1e-12 on it."""
    n = len(log)
    dev = deviations(log, trace)
    ok = (log[:, LOG_COL["in_resto"]] == 0.0) & (trace[:n, TRACE_COL["marker"]] > -200.0)
    for col in ("alpha", "theta", "kkt"):
        ok &= dev[col] <= N_CMP_RTOL
    bad = np.nonzero(~ok)[0]
    n_cmp = int(bad[0]) if bad.size else n
    assert max(dev["mu"][:n_cmp].max(initial=0.0), dev["delta"][:n_cmp].max(initial=0.0)) <= 1e-12, label
    return n_cmp


def worst(log, trace, n_cmp):
    return {col: float(f"{d[:n_cmp].max(initial=0.0):.3g}") for col, d in deviations(log, trace).items()}


def load_fixture():
    """(arrays keyed "<case>/<name>", index keyed by case) of the committed files."""
    with np.load(NPZ) as z:
        arrays = {k: z[k] for k in z.files}
    with open(INDEX) as f:
        return arrays, json.load(f)


def main():
    from multiprocessing import Pool
    with Pool(8) as pool:
        res = dict(zip(CASES, pool.map(_oracle, list(CASES), chunksize=1)))
    assemble(res)


def assemble(res):
    """Set n_cmp from the scalar build, assert the cases' conditions and write the fixture."""
    arrays, index = {}, {}
    for case, s in CASES.items():
        r = res[case]
        log = r["log"]
        assert len(log) == K_SHIFT and r["status"] == 2, (case, len(log), r["status"])
        ts, tw = (host_solve(case, scalar)["trace"] for scalar in (True, False))
        n_cmp = scalar_n_cmp(log, ts, case)
        assert n_cmp >= MIN_N_CMP, (case, n_cmp)
        delta = log[:, LOG_COL["delta"]]
        assert delta[0] >= 1.0, (case, delta[0])  # every case starts with an accepted large shift
        arrays[f"{case}/log"] = log
        arrays[f"{case}/log_scaled"] = r["log_scaled"]
        for k, v in case_inputs(case).items():
            if v is not None:
                arrays[f"{case}/in_{k}"] = v
        index[case] = dict(config=CONFIG, instance=s["instance"], lane_bounds=s["lane"], kind=s["kind"], options=OPT,
                           status=r["status"], iters=r["iters"], rows=len(log), n_cmp=n_cmp,
                           delta0=float(delta[0]), max_delta=float(delta[:n_cmp].max()),
                           max_row_gradient=float(f"{r['max_row_gradient']:.4g}"),
                           min_row_scale=float(f"{r['min_row_scale']:.4g}"),
                           scalar_worst_dev=worst(log, ts, n_cmp), wave_worst_dev=worst(log, tw, n_cmp))
        print(case, f"oracle {r['seconds']:.1f} s", json.dumps(index[case]), flush=True)
    np.savez_compressed(NPZ, **arrays)
    with open(INDEX, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(c)}: {json.dumps(index[c], sort_keys=True)}"
                                   for c in sorted(index)) + "\n}\n")
    size = os.path.getsize(NPZ) + os.path.getsize(INDEX)
    assert size < MAX_BYTES, size
    print("wrote", NPZ, INDEX, size, "bytes")


if __name__ == "__main__":
    main()
