"""Test helper (not a conftest): certify one returned point of the solver by re-deriving its outputs from the oracle
NLP.

A solver build returns, per instance, a point ``X, U, S`` and measures of it: ``constr_viol``, ``obj``, ``eC``, ``eL``,
``lam_g`` and a status.  The trajectory / grid / tail tests pin how the solver gets to a point; this module checks what
the caller gets back, at whatever point the solve ended, against ``oracle.nlp.MPCProblem`` evaluated in fp64 at the
returned ``X, U, S`` (no second solve, so it holds at every exit and at fp32):

* ``viol_ref``  max violation of ``opti_rows(w)`` against ``lbg / ubg`` (plus the lane rows of ``c(w)`` with lane
  bounds),
* ``obj_ref``   ``f(w)``; ``eC_ref, eL_ref`` = ``unpack(w)``,
* the stationarity residual ``r = grad_w [f(w) + lam_g . g_opti(w)]`` by autograd, split into the U, S and X blocks,
  with ``||grad f||_inf`` and ``max_j |lam_j| ||J_j||_inf`` to normalise it,
* the sign of the multipliers of one-sided rows and the one-sided complementarity
  ``max(v_U (ubg - g), v_L (g - lbg))``, ``v_U = max(lam, 0)``, ``v_L = max(-lam, 0)``.

``g_opti`` restates the Opti rows in torch in ``opti_rows`` order (tests/test_nlp_golden.py pins that order to the
reference's own recording; tests/test_certificate.py asserts ``g_opti`` equals ``opti_rows`` row for row).

Bars (DESIGN.md §4 "Certificate").  A deviation is measured in units of the scale that sets the precision's resolution:

  constr_viol   (|constr_viol - viol_ref| - relax)+ in ulps (of the solve's precision) of the largest local coordinate
                |X - X0|, |Y - Y0|, |yaw|, |v|, |S - s0| -- the solver measures against bounds relaxed by IPOPT's
                bound_relax_factor, relax = 1e-8 max(1, |bound|), so the two may differ by that much on top;
  obj           |obj - obj_ref| / (eps max(1, |obj_ref|, lambda_s |S_N - s0| + the cost terms)): the solve sums the
                objective in local coordinates, where the progress term and the costs can cancel;
  eC, eL        max |e - e_ref| / (eps max(1, largest local coordinate));
                (obj, eC and eL also carry, in fp64, the conditioning of the global-s centerline polynomials,
                eps64 sum_j |c_j| |s0|^j: Certificate.units)
  stationarity  ||r||_inf / max(1, ||grad f||_inf, max_j |lam_j| ||J_j||_inf)  (the number itself).

``HOST_DEV`` holds the maxima of these over the CPU cases of tests/test_certificate.py, measured with the host builds
of the solver source (the scalar C++ solver -- primal quantities only, it exports no lam_g -- and the emulated wave).
The device build is held to ``max(8 x host deviation, floor)`` units: 8 x is the project's allowance for FMA
contraction and the device libm; the floors are 64 units in fp64 and, in fp32, one unit (one ulp of
the largest local coordinate for constr_viol, eps32 max(1, |obj_ref|) for obj, eps32 max(1, coordinate) for eC / eL,
eps32 for the relative stationarity).  No bar comes from the device build.
"""
import importlib.util
import math
import os

import numpy as np
import torch

from mpcracing import workload as wl
from oracle.nlp import MPCProblem, Runtime

EPS = {"fp64": 2.0 ** -52, "fp32": 2.0 ** -23}
BOUND_RELAX = 1e-8  # IPOPT bound_relax_factor (mr_solver.h relax_amt)
DEVICE_FACTOR = 8.0
FLOOR = {"fp64": 64.0, "fp32": 1.0}
QUANTITIES = ("viol", "obj", "eC", "eL")

# Host deviations (units above): max over the CPU cases of tests/test_certificate.py, scalar and wave host builds,
# g++ -O2 without FMA contraction on x86-64.  tests/test_certificate.py asserts they are what the host builds give.
HOST_DEV = {
    "fp64": {"viol": 0.0, "obj": 0.15, "eC": 0.49, "eL": 0.93},
    "fp32": {"viol": 0.67, "obj": 2.2, "eC": 0.49, "eL": 1.2},
}
# Relative stationarity at exits of class (c), wave host build, by (precision, options): "default" = tol 1e-8 /
# acceptable_tol 1e-6, "reference" = the reference's IPOPT options tol 1e-4 / acceptable_tol 1e-2 (MPC.py:152-161).
HOST_STAT = {
    ("fp64", "default"): 9.3e-11,
    ("fp64", "reference"): 5.0e-16,
    ("fp32", "reference"): 9.0e-7,
}
STAT_FLOOR = {"fp64": 64.0 * EPS["fp64"], "fp32": EPS["fp32"]}


def ulp(v, precision):
    """One unit in the last place of |v| in the precision's format (v = 0: of 1)."""
    v = abs(float(v))
    return EPS[precision] * 2.0 ** math.floor(math.log2(v)) if v > 0 else EPS[precision]


def problem(inst, model, N, Ts, runtime, lane=False, tyres=None, u_init=None):
    """The oracle NLP of one instance: ``inst`` from workload.instance_dicts, ``runtime`` its column [5] of the batch
    (d_max bounds the throttle as the class attribute does in the reference, MPC.py:50), ``u_init`` its column [2][N]
    where the solve was given one (the shifted last_controls, MPC.py:120-125)."""
    rt = Runtime(alpha_c=float(runtime[0]), d_max=float(runtime[1]), q_v_y=float(runtime[2]), n=int(runtime[3]),
                 beta_delta=float(runtime[4]))
    lc = None
    if u_init is not None:
        cols = [(float(a), float(s)) for a, s in zip(*np.asarray(u_init)[:, :N])]
        lc = [(0.0, 0.0)] + cols[:-1]  # MPCProblem shifts last_controls itself: lc[1:] + [lc[-1]] == cols
    return MPCProblem(inst["state0"], inst["s0"], inst["cx"], inst["cy"], inst["max_error"], runtime=rt, N=int(N),
                      Ts=float(Ts), model=model, tyres=tyres, lane_bounds=bool(lane), last_controls=lc,
                      d_max_class=float(runtime[1]))


def g_opti(prob, w):
    """The Opti rows of ``MPCProblem.opti_rows`` as a torch function of w (same order, same canonical rows)."""
    N = prob.N
    U, S, X = prob.split(w)
    defects = prob.g(w)[7:].reshape(N, 6)  # X_i - f(X_{i-1}, U_{i-1}), i = 1..N
    stage = torch.cat([defects, (S[1:] - S[:-1]).reshape(N, 1)], dim=1).reshape(-1)
    Um = torch.roll(U, 1, dims=1)  # Python index i-1: U[:, -1] at i = 0
    box = torch.stack([U[0], U[0], U[1], U[1], U[0] - Um[0], U[1] - Um[1]], dim=1).reshape(-1)
    out = [S[:1], X[:, 0], stage, box]
    st = prob.state0
    if st.get("throttle") is not None:
        out.append((U[0, 0] - st["throttle"]).reshape(1))
    if st.get("steer") is not None:
        out.append((U[1, 0] - st["steer"]).reshape(1))
    return torch.cat(out)


def column(out, i, N=None):
    """Instance i of a batch's outputs cut to horizon N (default: the arrays' own): X [6][N+1], U [2][N], S, eC, eL,
    the scalars, and lam_g as the whole column (its NaN rows are part of what is certified)."""
    o = {k: np.asarray(v)[..., i] for k, v in out.items() if k not in ("trace", "timeline", "guard")}
    if N is not None:
        o["X"], o["U"], o["S"] = o["X"][:, :N + 1], o["U"][:, :N], o["S"][:N + 1]
        o["eC"], o["eL"] = o["eC"][:N], o["eL"][:N]
    return o


class Certificate:
    """The oracle's view of one returned point; see the module doc.  ``col``: ``column()``."""

    def __init__(self, prob, col, precision):
        self.prob, self.col, self.precision = prob, col, precision
        N = self.N = prob.N
        X, U, S = (np.array(col[k], np.float64) for k in ("X", "U", "S"))
        assert X.shape == (6, N + 1) and U.shape == (2, N) and S.shape == (N + 1,)
        self.finite = bool(np.isfinite(X).all() and np.isfinite(U).all() and np.isfinite(S).all())
        self.w = np.concatenate([U.reshape(-1), S, X.reshape(-1)])
        st = prob.state0
        self.local = float(max(np.abs(X[0] - st["x"]).max(), np.abs(X[1] - st["y"]).max(), np.abs(X[2:]).max(),
                               np.abs(S - prob.s0).max())) if self.finite else math.nan
        if not self.finite:
            return
        g, lo, hi = prob.opti_rows(self.w)
        self.g, self.lo, self.hi = g, lo, hi
        eq = lo == hi
        self.viol_eq = float(np.abs(g - lo)[eq].max())
        self.viol_bound = float(max(0.0, (lo - g)[~eq].max(), (g - hi)[~eq].max()))
        bounds = np.concatenate([lo[~eq], hi[~eq]])
        if prob.lane:
            c = prob.c(torch.as_tensor(self.w)).numpy()
            k = np.array([r[0] == "lane" for r in prob.rows])
            self.viol_bound = float(max(self.viol_bound, (prob.lo - c)[k].max(), (c - prob.hi)[k].max()))
            bounds = np.concatenate([bounds, prob.lo[k], prob.hi[k]])
        self.viol_ref = max(self.viol_eq, self.viol_bound)
        self.relax = BOUND_RELAX * max(1.0, float(np.abs(bounds[np.isfinite(bounds)]).max()))
        self.obj_ref = float(prob.f(torch.as_tensor(self.w)))
        _X, _U, _S, self.eC_ref, self.eL_ref = prob.unpack(self.w)
        # the input's own conditioning: the centerline polynomials come in global s, and moving them to s0 in fp64
        # (taylor_shift4; the oracle shifts in rationals) costs ~eps64 sum_j |c_j| |s0|^j in e_C, e_L, hence
        # that times |d f / d e| in the objective
        self.cond = max(sum(abs(c) * abs(prob.s0) ** (len(cs) - 1 - j) for j, c in enumerate(cs))
                        for cs in (prob.cx, prob.cy))
        eC, eL = (t.numpy() for t in prob.errors(torch.as_tensor(S), torch.as_tensor(X[0]), torch.as_tensor(X[1])))
        rp, fp = prob.rp, prob.fp
        self.obj_sens = float((rp.n * rp.alpha_c * np.abs(eC[1:]) ** (rp.n - 1)
                               + 2 * fp.alpha_L * np.abs(eL[1:])).sum())
        self._dual = None

    # ---- primal quantities: deviations in units, and the device bars ----
    def units(self):
        """The unit of each deviation.  The objective's: the solve sums f in local coordinates, -lambda_s (S_N - s0)
        plus the (positive) cost terms, and subtracts lambda_s s0 in fp64; the two parts can cancel, so its
        rounding is set by their sizes, not by |obj| alone (plus fp64 rounding of lambda_s S_N, which the oracle's
        own f(w) carries too).  e_C, e_L and through them
        the objective also carry the fp64 conditioning of the global-s polynomials (``cond``)."""
        p, eps = self.precision, EPS[self.precision]
        lam_s, SN = self.prob.fp.lambda_s, float(self.w[3 * self.N])
        terms = lam_s * abs(SN - self.prob.s0) + abs(self.obj_ref + lam_s * SN)  # |progress term| + the cost terms
        e = eps * max(1.0, self.local) + EPS["fp64"] * self.cond
        return {"viol": ulp(self.local, p), "eC": e, "eL": e,
                "obj": eps * max(1.0, abs(self.obj_ref), terms)
                + EPS["fp64"] * (lam_s * abs(SN) + self.cond * self.obj_sens)}

    def floors(self):
        """The least bar of each quantity (absolute): FLOOR units; the objective's is FLOOR eps max(1, |obj_ref|)."""
        u, fl = self.units(), FLOOR[self.precision]
        e = fl * EPS[self.precision] * max(1.0, self.local)
        return {"viol": fl * u["viol"], "eC": e, "eL": e,
                "obj": fl * EPS[self.precision] * max(1.0, abs(self.obj_ref))}

    def primal_errors(self):
        """{quantity: absolute difference} of the reported constr_viol, obj, eC, eL from the oracle's (the bound
        relaxation taken off constr_viol's)."""
        c = self.col
        return {"viol": max(0.0, abs(float(c["constr_viol"]) - self.viol_ref) - self.relax),
                "obj": abs(float(c["obj"]) - self.obj_ref),
                "eC": float(np.abs(np.asarray(c["eC"]) - self.eC_ref).max()),
                "eL": float(np.abs(np.asarray(c["eL"]) - self.eL_ref).max())}

    def primal_deviations(self):
        """primal_errors() in units()."""
        e, u = self.primal_errors(), self.units()
        return {q: e[q] / u[q] for q in QUANTITIES}

    def bar(self, q, factor=DEVICE_FACTOR):
        """The absolute bar of quantity q: max(factor x host deviation x unit, floor); factor 1 = the host builds'."""
        return max(factor * HOST_DEV[self.precision][q] * self.units()[q], self.floors()[q])

    def viol_abs_bar(self, factor=DEVICE_FACTOR):
        return self.relax + self.bar("viol", factor)

    def primal_failures(self, factor=DEVICE_FACTOR):
        """Check (a): the quantities whose reported value is not the oracle's at the returned point."""
        if not (self.finite and all(np.isfinite(np.asarray(self.col[k])).all()
                                    for k in ("constr_viol", "obj", "eC", "eL"))):
            return ["non-finite"]
        e = self.primal_errors()
        return [f"{q}: off by {e[q]:.3g} > {self.bar(q, factor):.3g}" for q in QUANTITIES
                if not e[q] <= self.bar(q, factor)]

    # ---- multipliers ----
    def lam(self, layout_rows=None):
        """(rows kept, lam_g on them) after checking which rows are NaN: exactly the absent state0 rows and the rows
        beyond 13 N + 9 (``layout_rows``: the column's length, default its own)."""
        lam = np.asarray(self.col["lam_g"], np.float64)
        N, st = self.N, self.prob.state0
        rows = 13 * N + 9
        assert lam.shape == (rows if layout_rows is None else layout_rows,) and lam.shape[0] >= rows, lam.shape
        want_nan = np.zeros(lam.shape[0], bool)
        want_nan[rows:] = True
        want_nan[rows - 2] = st.get("throttle") is None
        want_nan[rows - 1] = st.get("steer") is None
        assert np.array_equal(np.isnan(lam), want_nan), \
            ("NaN rows of lam_g", int(np.isnan(lam).sum()), int(want_nan.sum()),
             np.nonzero(np.isnan(lam) != want_nan)[0][:8])
        keep = ~want_nan[:rows]
        assert int(keep.sum()) == len(self.g), (int(keep.sum()), len(self.g))
        return keep, lam[:rows][keep]

    def dual(self, layout_rows=None):
        """Stationarity, sign and complementarity of lam_g at the returned point (dict, cached)."""
        if self._dual is not None:
            return self._dual
        prob, N = self.prob, self.N
        _keep, lam = self.lam(layout_rows)
        wt = torch.as_tensor(self.w).clone().requires_grad_(True)
        gf = torch.autograd.grad(prob.f(wt), wt)[0].numpy()
        r = torch.autograd.grad(prob.f(wt) + torch.dot(torch.as_tensor(lam), g_opti(prob, wt)), wt)[0].numpy()
        row_norm = self._row_norms()
        assert row_norm.shape == lam.shape
        rU, rS, rX = r[:2 * N], r[2 * N:3 * N + 1], r[3 * N + 1:].reshape(6, N + 1)
        if prob.lane:  # the lane rows' multipliers are not in lam_g: judge the blocks those rows do not touch
            judged = max(np.abs(rU).max(), np.abs(rX[2:]).max())
        else:
            judged = np.abs(r).max()
        norm = max(1.0, float(np.abs(gf).max()), float((np.abs(lam) * row_norm).max()))
        lo, hi, g = self.lo, self.hi, self.g
        ineq = lo < hi
        vU, vL = np.maximum(lam, 0.0), np.maximum(-lam, 0.0)
        wrong = np.where(ineq & np.isinf(lo), vL, 0.0) + np.where(ineq & np.isinf(hi), vU, 0.0)
        with np.errstate(invalid="ignore"):
            cU = np.where(ineq & np.isfinite(hi) & (vU > 0), vU * np.abs(hi - g), 0.0)
            cL = np.where(ineq & np.isfinite(lo) & (vL > 0), vL * np.abs(g - lo), 0.0)
        self._dual = {"r_U": float(np.abs(rU).max()), "r_S": float(np.abs(rS).max()), "r_X": float(np.abs(rX).max()),
                      "r": float(judged), "grad_f": float(np.abs(gf).max()), "norm": norm,
                      "stat_rel": float(judged) / norm, "wrong_sign": float(wrong.max()),
                      "compl": float(max(cU.max(), cL.max())), "lam_max": float(np.abs(lam).max())}
        return self._dual

    def _row_norms(self):
        """||J_j||_inf of every Opti row kept by lam(): 1 for the rows that are a variable or a difference of two;
        for the dynamics row q of stage i, max(1, |d f_q / d(x, u)|_inf at (X_{i-1}, U_{i-1})) (six backward passes:
        column k of F depends on column k of its arguments alone)."""
        prob, N = self.prob, self.N
        U, _S, X = prob.split(torch.as_tensor(self.w))
        Xc, Uc = X[:, :-1].clone().requires_grad_(True), U.clone().requires_grad_(True)
        from oracle import dynamics as dyn
        Fk = prob.F(Xc, Uc, dyn._torch_ns())
        stage = np.ones((N, 7))
        for q in range(6):
            gx, gu = torch.autograd.grad(Fk[q].sum(), (Xc, Uc), retain_graph=True, allow_unused=True)
            for gr in (gx, gu):
                if gr is not None:
                    stage[:, q] = np.maximum(stage[:, q], gr.abs().max(dim=0).values.numpy())
        return np.concatenate([np.ones(7), stage.reshape(-1), np.ones(len(self.g) - 7 - 7 * N)])

    def stat_bar(self, options, factor=DEVICE_FACTOR):
        return max(factor * HOST_STAT[(self.precision, options)], STAT_FLOOR[self.precision])

    def status_failures(self, status, factor=DEVICE_FACTOR, layout_rows=None):
        """Check (b): what status 0 / 1 claim by IPOPT's definitional thresholds (converged() / acceptable():
        constr_viol_tol = compl_inf_tol = 1e-4, acceptable_* = 1e-2), each with the allowance max|lam| (viol_ref +
        relax) the one-sided complementarity can exceed the true one by, plus the precision's bar."""
        if status not in (0, 1):
            return []
        thr = 1e-4 if status == 0 else 1e-2
        d = self.dual(layout_rows)
        vb = self.viol_abs_bar(factor)
        out = []
        if not self.viol_ref <= thr + vb:
            out.append(f"status {status} but viol_ref {self.viol_ref:.3g}")
        allow = d["lam_max"] * (self.viol_ref + vb)
        if not d["compl"] <= thr + allow:
            out.append(f"status {status} but complementarity {d['compl']:.3g} > {thr:g} + {allow:.3g}")
        return out

    def dual_failures(self, options, factor=DEVICE_FACTOR, layout_rows=None):
        """Check (c): relative stationarity within the bar; no wrong-signed multiplier on a one-sided row beyond the
        bar (such a multiplier is the row's slack stationarity residual, so it is held to the same bar on the
        same scale)."""
        d = self.dual(layout_rows)
        bar = self.stat_bar(options, factor)
        out = []
        if not d["stat_rel"] <= bar:
            out.append(f"stationarity {d['stat_rel']:.3g} > {bar:.3g} (r_U {d['r_U']:.3g} r_S {d['r_S']:.3g} "
                       f"r_X {d['r_X']:.3g}, |grad f| {d['grad_f']:.3g})")
        if not d["wrong_sign"] <= bar * d["norm"]:
            out.append(f"wrong-signed multiplier {d['wrong_sign']:.3g} > {bar * d['norm']:.3g}")
        return out


def in_class_c(status, kkt, tol):
    """Exits from the original problem's iterate at or below the claimed tolerance: status 0 and 1, and status 3
    with kkt <= tol (a stop at the mu floor whose point meets the KKT test but not an unscaled one)."""
    return status in (0, 1) or (status == 3 and kkt <= tol)


def certify(prob, col, precision, options, tol, factor=DEVICE_FACTOR, layout_rows=None):
    """Every check the status of the column calls for -> list of failure texts (empty: certified)."""
    cert = Certificate(prob, col, precision)
    status = int(col["status"])
    fails = cert.primal_failures(factor)
    if fails == ["non-finite"]:
        return cert, (fails if status in (0, 1) else [])  # only a claimed solve must be finite
    if "lam_g" in col:
        cert.lam(layout_rows)  # the NaN rows, at every exit
        fails += cert.status_failures(status, factor, layout_rows)
        if in_class_c(status, float(col["kkt"]), tol):
            fails += cert.dual_failures(options, factor, layout_rows)
    return cert, fails


# ---------------------------------------------------------------------------------------------------- cases
# Shared by tests/test_certificate.py (host builds, a few instances each) and tests/test_gpu_certificate.py (the
# library, whole batches): inputs from mpcracing.workload only.
OPTIONS = {"default": dict(tol=1e-8, acceptable_tol=1e-6, acceptable_iter=15, max_iter=500),
           "reference": dict(tol=1e-4, acceptable_tol=1e-2, acceptable_iter=15, max_iter=500)}  # MPC.py:152-161


def _tail_generator():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_tail_golden.py")
    spec = importlib.util.spec_from_file_location("make_tail_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def take(batch, idx):
    return {k: (None if v is None else np.ascontiguousarray(v[..., idx])) for k, v in batch.items()}


def take_case(case, idx):
    """The instances ``idx`` of a case."""
    return dict(case, batch=take(case["batch"], np.asarray(idx)),
                horizon=None if case["horizon"] is None else case["horizon"][np.asarray(idx)])


def tail_case(name, precision, options, idx=None):
    """The instances of make_tail_golden.case_batch(name) (``idx``: a subset of them) as a case."""
    cfg = wl.CONFIGS[name]
    _n, _p, _i, b = _tail_generator().case_batch(name)
    if idx is not None:
        b = take(b, np.asarray(idx))
    return dict(model=cfg["model"], N=cfg["N"], Ts=cfg["Ts"], lane=cfg["lane"], precision=precision, options=options,
                tyres=wl.tyre_coeffs(cfg["tyres"]) if cfg["tyres"] else None, batch=b, horizon=None)


def config_case(name, B, precision="fp64", options="default"):
    cfg = wl.CONFIGS[name]
    return dict(model=cfg["model"], N=cfg["N"], Ts=cfg["Ts"], lane=cfg["lane"], precision=precision, options=options,
                tyres=None, batch=wl.make_batch(name, limit=B), horizon=None)


def nan_state0_case(B=8):
    """C2's first instances under the dynamic model with a u_init: state0 throttle and steer NaN (None) in the first
    half, throttle alone in the next quarter, both given in the rest."""
    case = dict(config_case("C2", B), model="dyn")
    b = case["batch"]
    b["state0"][6:, :B // 2] = np.nan
    b["state0"][6, B // 2:B // 2 + B // 4] = np.nan
    N = case["N"]
    rng = np.random.default_rng(3)
    u = np.stack([rng.uniform(-0.5, 0.8, (N, B)), rng.uniform(-0.3, 0.3, (N, B))])
    u[:, -1] = u[:, -2]  # a shifted last_controls repeats its last column (MPC.py:120-121)
    b["u_init"] = u
    return case


def horizons_case(horizons=None):
    """The kin family of tests/horizon_cases.py: 14 instances with horizons 1 .. 63 under the layout horizon 63
    (``horizons``: those of them to keep)."""
    import horizon_cases as hc
    cases = [c for c in hc.FAMILIES["kin"] if horizons is None or hc.G.CASES[c]["N"] in horizons]
    model, lane, Ts, over, tyres = hc.family_config(cases)
    assert not over and tyres is None
    return dict(model=model, N=hc.NL, Ts=Ts, lane=lane, precision="fp64", options="default", tyres=None,
                batch=hc.mixed_inputs(cases), horizon=hc.horizons(cases))


def certify_batch(case, out, factor=DEVICE_FACTOR):
    """certify() for every instance of a case's outputs -> list of (Certificate, status, failures)."""
    b, N = case["batch"], case["N"]
    res = []
    for i, inst in enumerate(wl.instance_dicts(b)):
        Ni = N if case["horizon"] is None else int(case["horizon"][i])
        prob = problem(inst, case["model"], Ni, case["Ts"], b["runtime"][:, i], case["lane"], case["tyres"],
                       None if b.get("u_init") is None else b["u_init"][:, :, i])
        col = column(out, i, Ni)
        cert, fails = certify(prob, col, case["precision"], case["options"], OPTIONS[case["options"]]["tol"], factor,
                              layout_rows=13 * N + 9)
        res.append((cert, int(col["status"]), fails))
    return res
