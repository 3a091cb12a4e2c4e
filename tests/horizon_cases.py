"""Shared by tests/test_horizons.py and tests/test_gpu_horizons.py: batches whose instances have different horizons
(mr_solve_batch_horizons, include/mpcracing.h) and the comparison a solver build is held to.

The yardstick is exact: instance i of a mixed batch under the layout horizon NL must be, bit for bit, the solve of
that instance alone by the existing entry point with N = N_i, inside arrays that keep the strides of NL, and NaN in
every row beyond N_i.  The instances and configurations are those of the committed oracle log
(tests/config_grid_cases.py), so the whole-solve columns are also held to IPOPT directly.
"""
import ctypes

import numpy as np

import config_grid_cases as cg
import host_twin as ht

G = cg.GEN
NL = 63  # the layout horizon of every mixed batch here
SENTINEL = -7.25  # pre-filled into output buffers: a row nobody may write keeps it
FLOAT_KEYS = ("X", "U", "S", "eC", "eL", "obj", "kkt", "constr_viol", "lam_g")

# family -> the case of each horizon (the horizon sweep (a) of make_config_grid_golden.py)
FAMILIES = {
    "kin": [f"kin_N{N}" for N in (1, 2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 62, 63)],
    "dyn_lane": [f"dyn_lane_N{N}" for N in (1, 2, 16, 17, 32, 33, 48, 63)],
    "blend_par": [f"blend_N{N}_par" for N in (2, 16, 31, 47, 63)],
}
# the batches held to the oracle directly: the whole-solve cases and their fillers
WHOLE_BATCHES = {
    "kin": ["kin_N1_whole", "kin_N16", "kin_N63_whole", "kin_N33"],
    "blend_par": ["blend_N2_par", "blend_N31_par_whole", "blend_N63_par"],
}


def horizons(cases):
    return np.array([G.CASES[c]["N"] for c in cases], np.int32)


def family_config(cases):
    """(model, lane, Ts, overrides, tyres) shared by the cases of a batch (asserted)."""
    s0 = G.CASES[cases[0]]
    for c in cases:
        s = G.CASES[c]
        assert (s["model"], s["lane"], s["Ts"]) == (s0["model"], s0["lane"], s0["Ts"]), c
        assert G.case_overrides(c) == G.case_overrides(cases[0]), c
    return s0["model"], s0["lane"], s0["Ts"], G.case_overrides(cases[0]), G.case_tyres(cases[0])


def mixed_inputs(cases, u_init=None):
    """The B = 1 inputs of ``cases`` side by side (no u_init of their own in these families); ``u_init``
    [2][NL][B] optional."""
    subs = [G.case_inputs(c) for c in cases]
    assert all(s["u_init"] is None for s in subs)
    b = {k: np.ascontiguousarray(np.concatenate([s[k] for s in subs], axis=-1)) for k in subs[0] if k != "u_init"}
    b["u_init"] = u_init
    return b


def nan_padded_u_init(Ns, seed=11):
    """A random u_init [2][NL][B] inside every bound whose column i is NaN from row N_i on: a solve that read a row
    it must not (a stride mix-up) is poisoned."""
    rng = np.random.default_rng(seed)
    u = np.stack([rng.uniform(-0.4, 0.6, (NL, len(Ns))), rng.uniform(-0.3, 0.3, (NL, len(Ns)))])
    for i, N in enumerate(Ns):
        u[:, N:, i] = np.nan
    return u


def one_instance(batch, i, N):
    """Instance i of a mixed batch as the B = 1 batch of a solver with horizon N."""
    sub = {k: (None if v is None else np.ascontiguousarray(v[..., i:i + 1])) for k, v in batch.items()}
    if sub.get("u_init") is not None:
        sub["u_init"] = np.ascontiguousarray(sub["u_init"][:, :N])
    return sub


def permuted(batch, perm):
    return {k: (None if v is None else np.ascontiguousarray(v[..., perm])) for k, v in batch.items()}


def host_solve(cfg, batch, horizon, scalar=False, duals=False, tyres=None, nthreads=8, prefill=None, guard=0):
    """tests/host_twin.solve through mrh_solve_batch[_scalar]_horizons (``horizon``: int32 [B] or None).  The output
    buffers are pre-filled with ``prefill`` (default 0, as host_twin.solve; -1 in status / iters); with ``guard``
    each is followed by that many pre-filled elements, returned as out["guard"][key]."""
    N = cfg.N
    B = batch["s0"].shape[0]
    arr = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in batch.items() if v is not None}
    inp = ht.abi.MRInputs(*[ht._p(arr.get(k)) for k in ("state0", "s0", "cx", "cy", "max_error", "runtime",
                                                         "u_init")])
    fill = 0.0 if prefill is None else prefill
    shapes = {"X": (6, N + 1, B), "U": (2, N, B), "S": (N + 1, B), "eC": (N, B), "eL": (N, B), "status": (B,),
              "iters": (B,), "obj": (B,), "kkt": (B,), "constr_viol": (B,)}
    if duals:
        shapes["lam_g"] = (13 * N + 9, B)
    out, tails = {}, {}
    for k, shp in shapes.items():
        n = int(np.prod(shp))
        flat = np.full(n + guard, -1, np.int32) if k in ("status", "iters") else np.full(n + guard, fill)
        out[k], tails[k] = flat[:n].reshape(shp), flat[n:]
    o = ht.abi.MROutputs(*[ht._p(out.get(k)) for k in ("X", "U", "S", "eC", "eL", "status", "iters", "obj", "kkt")],
                         None, -1, 0, ht._p(out.get("lam_g")), None, ht._p(out["constr_viol"]))
    if tyres is not None:
        (af, Fzf), (ar, Fzr) = tyres
        af, ar = np.asarray(af, np.float64), np.asarray(ar, np.float64)
        pa = af.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        pb = ar.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    else:
        pa = pb = None
        Fzf = Fzr = 0.0
    hz = None
    if horizon is not None:
        hz = np.ascontiguousarray(horizon, np.int32)
        assert hz.shape == (B,)
    fn = ht.lib().mrh_solve_batch_scalar_horizons if scalar else ht.lib().mrh_solve_batch_horizons
    rc = fn(ctypes.byref(cfg), pa, Fzf, pb, Fzr, B, ctypes.byref(inp), ctypes.byref(o),
            hz.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if hz is not None else None, nthreads)
    assert rc == 0
    if guard:
        out["guard"] = tails
    return out


def bit_equal(a, b):
    """np.array_equal on the bit patterns: equal values, NaNs at equal positions."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def rows_of(N, NLay=NL):
    """key -> (axis of the stage rows, rows instance horizon N reaches) in arrays of layout horizon NLay."""
    return {"X": (1, N + 1), "U": (1, N), "S": (0, N + 1), "eC": (0, N), "eL": (0, N), "lam_g": (0, 13 * N + 9)}


def column(o, i):
    return {k: np.asarray(v)[..., i] for k, v in o.items() if k not in ("trace", "timeline", "guard")}


def sliced(col, N):
    """A column of a mixed batch cut to the arrays a solver with horizon N returns (B = 1)."""
    out = {}
    for k, v in col.items():
        if k in rows_of(N):
            ax, n = rows_of(N)[k]
            v = np.take(v, np.arange(n), axis=ax)
        out[k] = np.asarray(v)[..., None]
    return out


def assert_column_is_uniform_solve(col, one, N, label):
    """``col``: column i of a mixed solve (layout NL); ``one``: the B = 1 outputs of the uniform solve at N.  Rows
    within N bitwise equal, every row beyond NaN, status and iterations equal."""
    assert int(col["status"]) == int(one["status"][0]) and int(col["iters"]) == int(one["iters"][0]), \
        (label, int(col["status"]), int(one["status"][0]), int(col["iters"]), int(one["iters"][0]))
    for k in FLOAT_KEYS:
        if k not in col or k not in one:
            continue
        v, ref = np.asarray(col[k]), np.asarray(one[k])[..., 0]
        if k in rows_of(N):
            ax, n = rows_of(N)[k]
            inside = np.take(v, np.arange(n), axis=ax)
            beyond = np.take(v, np.arange(n, v.shape[ax]), axis=ax)
            assert np.isnan(beyond).all(), (label, k, "rows beyond the horizon are not NaN")
        else:
            inside = v
        assert bit_equal(inside, ref), (label, k, float(np.nanmax(np.abs(inside - ref))) if inside.shape == ref.shape
                                        else (inside.shape, ref.shape))


def assert_not_solved(col, label):
    """An instance whose horizon is out of range: status 3, 0 iterations, NaN in every float output."""
    assert int(col["status"]) == 3 and int(col["iters"]) == 0, (label, int(col["status"]), int(col["iters"]))
    for k in FLOAT_KEYS:
        if k in col:
            assert np.isnan(np.asarray(col[k])).all(), (label, k)


def check_against_oracle(case, col, label, device=False):
    """A whole-solve column of a mixed batch, cut to its horizon, against the oracle log: the checks and bars of
    tests/config_grid_cases.py unchanged (whole-solve record, final point 1e-6, lam_g 1e-7 of its largest entry)."""
    N = G.CASES[case]["N"]
    o = sliced(col, N)
    cg.check_whole(case, o["status"][0], o["iters"][0], o["obj"][0], label)
    cg.check_point(case, o, label, device=device)
    if "lam_g" in o and not G.CASES[case]["lane"]:
        lam = o["lam_g"][:, 0]
        assert not np.isnan(lam).any(), (label, case)
        cg.check_lam_g(case, lam, label)
