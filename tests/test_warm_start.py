"""The primal warm start on the host builds of the solver source (the scalar solver and the emulated wavefront):
mrh_solve_batch[_scalar]_warm and mrh_warm_shift (include/mpcracing.h mr_solve_batch_warm, mr_warm_shift).
tests/test_gpu_warm_start.py holds the gfx950 build to the same fixture and the same helpers (tests/warm_cases.py).

1. Trajectory parity: from each golden guess (tests/golden/warm_golden.npz, the oracle's
   solve_ipopt(p, w0=w, rules=PRODUCT)) a build's trace is the oracle's log at the bars of
   tests/ipopt_trace_cases.py, with its status, iteration count, objective (1e-10) and lam_g (1e-7 of max |lam_g|).
   Case f starts at theta_0 ~ 48: a start that left the dynamics defects out of theta_0 (theta_max, theta_min)
   takes other steps.
2. Exactness: without a guess (NULL, or use all zero) the bits of mrh_solve_batch_horizons; in a mixed batch
   (layout 16, horizons 2 / 8 / 15 / 16, warm and cold interleaved) every instance is bitwise its own B = 1
   solve, also permuted; rows 0 and beyond N_i of the guess are never read; a NaN in row N_i makes the instance
   cold (its cold bits, used = 0) and leaves its neighbours alone.
3. The shift's host twin against the numpy restatement.
4. The warm-started outputs certified by tests/kkt_certificate.py, fp64 and fp32.
"""
import numpy as np
import pytest

import horizon_cases as hc
import host_twin as ht
import kkt_certificate as kc
import warm_cases as wc

OUT_KEYS = ("X", "U", "S", "eC", "eL", "status", "iters", "obj", "kkt", "constr_viol", "lam_g")
BUILDS = pytest.mark.parametrize("scalar", [True, False], ids=["scalar", "wave"])


def _cfg(precision="fp64", N=wc.MIXED_NL, **kw):
    opt = dict(wc.OPTIONS)
    opt.update(kw)
    return ht.config(N, wc.MIXED_MODEL, precision, False, wc.TS, **opt)


def _same_bits(a, b, label, keys=OUT_KEYS):
    for k in keys:
        if k in a or k in b:
            assert hc.bit_equal(a[k], b[k]), (label, k)
    if "guard" in a:
        for k, tail in a["guard"].items():
            assert k not in b["guard"] or hc.bit_equal(tail, b["guard"][k]), (label, k, "guard")
            assert (tail == (-1 if tail.dtype.kind == "i" else wc.SENTINEL)).all(), (label, k, "written past its end")


_mixed = {}


def _mixed_solve(scalar):
    """The mixed batch's warm solve, once per build."""
    if scalar not in _mixed:
        new, warm, hz = wc.mixed_batch()
        _mixed[scalar] = wc.host_solve(_cfg(), new, horizon=hz, warm=warm, scalar=scalar, duals=not scalar,
                                       prefill=wc.SENTINEL, guard=7)
    return _mixed[scalar]


# ------------------------------------------------------------------------------------------- the fixture itself
def test_warm_fixture():
    """The stored guesses are shift_numpy of the stored previous solutions (the rough case: of its shifted controls
    only), w0 is the guess in the oracle's variable order, and the generator's conditions hold in the index."""
    arrays, index = wc.fixture()
    assert sorted(index) == sorted(wc.CASES)
    for case, c in wc.CASES.items():
        e = index[case]
        assert e["case"] == c and e["options"] == wc.OPTIONS
        sub, warm = wc.case_batch(case)
        N = c["N"]
        X, U, S = (np.array(arrays[f"{case}/prev_{k}"]) for k in ("X", "U", "S"))
        u, x, s, use, ex = wc.shift_numpy(X, U, S, 0, c["Np"], N, sub["state0"][:, 0], sub["s0"][0],
                                          wc.model_step(wc.oracle_problem(case, sub)))
        assert use == 1 and int(ex.sum()) == max(0, N - c["Np"] + 1)
        assert np.array_equal(sub["u_init"][..., 0], u)
        if not c["rough"]:
            assert hc.bit_equal(warm["x_init"][..., 0], x) and hc.bit_equal(warm["s_init"][..., 0], s)
        assert np.isnan(warm["x_init"][:, 0]).all() and np.isnan(warm["s_init"][0]).all()
        assert np.array_equal(arrays[f"{case}/w0"], wc.w0_of(sub, warm["x_init"][..., 0], warm["s_init"][..., 0], N))
        assert e["status"] == 0 and e["cold"]["status"] == 0 and e["max_row_gradient"] <= 100.0
        assert e["rows"] == e["iters"] and e["rows"] - 2 <= e["n_cmp"] <= e["rows"]
        if not c["rough"]:
            assert e["iters"] <= e["cold"]["iters"]
    assert index["f_dyn15_rough"]["theta0"] > 10.0
    assert index["c_blend16_from12"]["case"]["Np"] == 12


# ------------------------------------------------------------------------------------------- 1. trajectory parity
@BUILDS
@pytest.mark.parametrize("case", list(wc.CASES))
def test_host_build_matches_oracle_from_the_guess(case, scalar):
    sub, warm = wc.case_batch(case)
    o = wc.host_solve(wc.case_cfg(case), sub, warm=warm, scalar=scalar, duals=not scalar, tyres=wc.case_tyres(case),
                      nthreads=1, trace_instance=0, trace_cap=520)
    wc.check_case(case, o, "scalar" if scalar else "wave")


# ------------------------------------------------------------------------------------------- 2. exactness
@BUILDS
def test_without_a_guess_the_bits_of_the_horizons_entry(scalar):
    """(i) warm = NULL, and a guess with use all zero, against mrh_solve_batch[_scalar]_horizons: every output,
    sentinel-prefilled buffers with guards."""
    new, warm, hz = wc.mixed_batch()
    kw = dict(horizon=hz, scalar=scalar, duals=not scalar, prefill=wc.SENTINEL, guard=7)
    ref = wc.host_solve(_cfg(), new, entry="horizons", **kw)
    _same_bits(wc.host_solve(_cfg(), new, warm=None, **kw), ref, "warm = NULL")
    off = wc.host_solve(_cfg(), new, warm=dict(warm, use=np.zeros(8, np.int32)), **kw)
    _same_bits(off, ref, "use all zero")
    assert (off["used"] == 0).all()
    assert (ref["status"] == 0).all()


@BUILDS
def test_mixed_batch_instances_are_their_own_solves(scalar):
    """(ii) instance i of the mixed batch is bitwise the B = 1 solve of a solver with N = N_i from its own guess
    (or cold, where its use flag is 0); the permuted batch gives the permuted columns."""
    new, warm, hz = wc.mixed_batch()
    o = _mixed_solve(scalar)
    assert np.array_equal(o["used"], wc.MIXED_WANT) and (o["status"] == 0).all()
    assert all((tail == (-1 if tail.dtype.kind == "i" else wc.SENTINEL)).all() for tail in o["guard"].values())
    cold = wc.host_solve(_cfg(), new, horizon=hz, scalar=scalar, entry="horizons")
    for i, N in enumerate(hz):
        one = wc.host_solve(_cfg(N=int(N)), hc.one_instance(new, i, int(N)), warm=wc.one_warm(warm, i, int(N)),
                            scalar=scalar, duals=not scalar)
        assert int(one["used"][0]) == wc.MIXED_WANT[i]
        hc.assert_column_is_uniform_solve(hc.column(o, i), one, int(N), f"instance {i} N {N}")
        if wc.MIXED_WANT[i] and i != 7:  # (instance 7: Np = Nn = 2, a one-row guess that changes little)
            assert int(o["iters"][i]) != int(cold["iters"][i]) or not hc.bit_equal(o["X"][..., i], cold["X"][..., i])
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    wp = {k: np.ascontiguousarray(v[..., perm]) for k, v in warm.items()}
    p = wc.host_solve(_cfg(), hc.permuted(new, perm), horizon=hz[perm], warm=wp, scalar=scalar, duals=not scalar)
    for k in OUT_KEYS + ("used",):
        if k in p:
            assert hc.bit_equal(p[k], np.asarray(o[k])[..., perm]), k


@BUILDS
def test_rows_outside_the_horizon_are_never_read(scalar):
    """(iii) row 0 and the rows beyond N_i hold NaN in the mixed batch; with finite junk there the bits are the same."""
    new, warm, hz = wc.mixed_batch()
    junk = dict(x_init=warm["x_init"].copy(), s_init=warm["s_init"].copy(), use=warm["use"])
    for i, N in enumerate(hz):
        assert np.isnan(warm["x_init"][:, 0, i]).all() and np.isnan(warm["x_init"][:, N + 1:, i]).all()
        assert np.isnan(warm["s_init"][0, i]) and np.isnan(warm["s_init"][N + 1:, i]).all()
        junk["x_init"][:, 0, i] = junk["s_init"][0, i] = 1e3
        junk["x_init"][:, N + 1:, i] = junk["s_init"][N + 1:, i] = -1e3
    o = wc.host_solve(_cfg(), new, horizon=hz, warm=junk, scalar=scalar, duals=not scalar, prefill=wc.SENTINEL,
                      guard=7)
    _same_bits(o, _mixed_solve(scalar), "junk rows", OUT_KEYS + ("used",))


@BUILDS
@pytest.mark.parametrize("what", ["x_init", "s_init"])
def test_non_finite_guess_starts_cold(scalar, what):
    """(iv) a NaN (x_init) or an inf (s_init) in row N_i of instance 2's guess: its cold bits and used = 0, every
    other instance unchanged."""
    new, warm, hz = wc.mixed_batch()
    bad = dict(x_init=warm["x_init"].copy(), s_init=warm["s_init"].copy(), use=warm["use"])
    if what == "x_init":
        bad["x_init"][4, hz[2], 2] = np.nan
    else:
        bad["s_init"][hz[2], 2] = np.inf
    o = wc.host_solve(_cfg(), new, horizon=hz, warm=bad, scalar=scalar, duals=not scalar)
    ref, cold = _mixed_solve(scalar), wc.host_solve(_cfg(), new, horizon=hz, scalar=scalar, duals=not scalar,
                                                   entry="horizons")
    want = wc.MIXED_WANT.copy()
    want[2] = 0
    assert np.array_equal(o["used"], want)
    for k in OUT_KEYS:
        if k in o:
            exp = np.array(ref[k])
            exp[..., 2] = cold[k][..., 2]
            assert hc.bit_equal(o[k], exp), k
    assert not hc.bit_equal(ref["X"][..., 2], cold["X"][..., 2]) or ref["iters"][2] != cold["iters"][2]


# ------------------------------------------------------------------------------------------- 3. the shift
@pytest.mark.parametrize("model", ["kin", "dyn", "blend", "blend_pacejka"])
def test_host_shift_matches_numpy(model):
    from mpcracing import workload as wl
    from oracle.nlp import MPCProblem
    sb = wc.shift_batch()
    NL = sb["U"].shape[1]
    tyres = wl.tyre_coeffs("pacejka-2") if model.endswith("pacejka") else None
    cfg = ht.config(NL, model, "fp64", False, wc.TS)
    got = wc.host_shift(cfg, sb["X"], sb["U"], sb["S"], sb["status"], sb["Np"], sb["state0"], sb["s0"], sb["Nn"],
                        tyres=tyres)
    inst = wl.instance_dicts(wl.make_batch("C1"))[0]
    prob = MPCProblem(inst["state0"], inst["s0"], inst["cx"], inst["cy"], inst["max_error"], N=NL, Ts=wc.TS,
                      model=model, tyres=tyres)
    wc.check_shift(got, sb, wc.model_step(prob), f"host {model}")
    # horizon arrays absent: both horizons are the layout's
    full = wc.host_shift(cfg, sb["X"][..., 3:4], sb["U"][..., 3:4], sb["S"][..., 3:4], sb["status"][3:4], None,
                         sb["state0"][:, 3:4], sb["s0"][3:4], None, tyres=tyres)
    one = {k: (v[..., 3:4] if isinstance(v, np.ndarray) else v) for k, v in sb.items()}
    wc.check_shift(full, dict(one, Np=np.array([NL]), Nn=np.array([NL]), use=np.array([1])), wc.model_step(prob),
                   f"host {model} NULL horizons")


def test_shift_out_of_range_horizon():
    """A horizon outside [1, NL] on either side: use 0, the guess NaN, the controls still shifted."""
    sb = wc.shift_batch()
    NL = sb["U"].shape[1]
    cfg = ht.config(NL, "dyn", "fp64", False, wc.TS)
    Np, Nn = sb["Np"].copy(), sb["Nn"].copy()
    Nn[0], Np[2] = NL + 1, 0
    got = wc.host_shift(cfg, sb["X"], sb["U"], sb["S"], sb["status"], Np, sb["state0"], sb["s0"], Nn)
    for i in (0, 2):
        assert got["use"][i] == 0 and np.isnan(got["x_init"][..., i]).all() and np.isnan(got["s_init"][:, i]).all()
        u, _x, _s, use, _ex = wc.shift_numpy(sb["X"][..., i], sb["U"][..., i], sb["S"][..., i], 0, int(Np[i]),
                                             int(Nn[i]), sb["state0"][:, i], sb["s0"][i], None)
        assert use == 0 and hc.bit_equal(got["u_init"][..., i], u)
    assert got["use"][1] == 1


# ------------------------------------------------------------------------------------------- 4. certificate
def _mixed_case(precision, options):
    new, _warm, hz = wc.mixed_batch()
    return dict(model=wc.MIXED_MODEL, N=wc.MIXED_NL, Ts=wc.TS, lane=False, precision=precision, options=options,
                tyres=None, batch=new, horizon=hz)


@pytest.mark.parametrize("precision,options", [("fp64", "default"), ("fp32", "reference")])
@pytest.mark.parametrize("scalar", [False, True], ids=["wave", "scalar"])
def test_warm_started_outputs_are_certified(scalar, precision, options):
    """tests/kkt_certificate.certify at the host's own bars (factor 2, as tests/test_certificate.py) on the mixed
    batch's warm-started outputs."""
    new, warm, hz = wc.mixed_batch()
    case = _mixed_case(precision, options)
    cfg = ht.config(wc.MIXED_NL, wc.MIXED_MODEL, precision, False, wc.TS, **kc.OPTIONS[options])
    out = wc.host_solve(cfg, new, horizon=hz, warm=warm, scalar=scalar, duals=not scalar)
    assert np.array_equal(out["used"], wc.MIXED_WANT)
    bad = [(i, st, f) for i, (_c, st, f) in enumerate(kc.certify_batch(case, out, factor=2.0)) if f]
    assert not bad, bad
    assert np.isin(out["status"], (0, 1)).all(), out["status"]
