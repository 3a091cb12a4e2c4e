"""Shared checks of the tyre fit against tests/golden/tyrefit_golden.* (generator: make_tyrefit_golden.py).

Used by test_tyrefit.py (host build of the source) and test_gpu_tyrefit.py (gfx950).  Tolerances: 100 x the
reference's own spread under permutations of the rows (``ref_noise`` in the json), floor 1e-13, relative and
taken per gradient component / per parameter (a component the reference reproduces to 2e-15 is held to
1e-13 even where a neighbouring one is only reproducible to 6e-9); 1e-10 relative against the mpmath values.
"""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "tyrefit_golden.npz"))
with open(os.path.join(HERE, "golden", "tyrefit_golden.json")) as _f:
    META = json.load(_f)
ROWS = G["rows"]  # [200][15]
FZ_WELL, FZ_DEG = META["Fz_well"], META["Fz_degenerate"]
LOSS_GRAD_CASES = sorted(META["cases"])
TRAJECTORIES = sorted(META["trajectories"])
MP_TOL = 1e-10


def tol(noise):
    return np.maximum(100.0 * np.asarray(noise, np.float64), 1e-13)


def rel_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)


def check_loss_grad(case, fn):
    """fn(rows, params, Fz, kind) -> (loss, grad) of one parameter set."""
    m = META["cases"][case]
    name, n = case.split("/")[0], m["n"]
    loss, grad = fn(ROWS[:n], G[f"{name}/params"], G[f"{name}/Fz"], m["kind"])
    comp = m["components"]
    el = float(rel_err(loss, G[f"{case}/loss"]))
    eg = rel_err(np.asarray(grad)[comp], G[f"{case}/grad"][comp])
    tg = tol(m["ref_noise_grad_components"])
    print(f"{case}: loss rel err {el:.3e} (tol {tol(m['ref_noise_loss']):.1e}), grad rel err / tol per component "
          f"{np.array2string(eg, precision=1)} / {np.array2string(tg, precision=1)}")
    assert el <= tol(m["ref_noise_loss"]), (case, el)
    assert (eg <= tg).all(), (case, eg, tg)


def check_mp_loss8(fn):
    """8-row loss and all 18 gradient components at the degenerate load against mpmath."""
    loss, grad = fn(ROWS[:8], G["pac_deg/params"], G["pac_deg/Fz"], "pacejka")
    el, eg = float(rel_err(loss, G["mp/loss8/loss"])), rel_err(grad, G["mp/loss8/grad"])
    print(f"mpmath 8-row loss rel err {el:.3e}, grad rel err max {eg.max():.3e}: {eg}")
    assert el <= MP_TOL and eg.max() <= MP_TOL, (el, eg)
    return max(el, float(eg.max()))


def check_trajectory(name, fit):
    """fit(rows, kind, init, Fz, optimizer, lr, epochs, factor, patience, perm, weight_decay) -> FitResult of one run with
    the parameters after every step recorded."""
    m = META["trajectories"][name]
    r = fit(ROWS, m["kind"], G[f"traj/{name}/init"], G[f"traj/{name}/Fz"], m["optimizer"], m["lr"], m["epochs"],
            m["factor"], m["patience"], G[m["perm"]], m["weight_decay"])
    assert r.steps[0].shape == G[f"traj/{name}/steps"].shape
    assert np.array_equal(r.steps[0][-1], r.p_final[0])
    es = rel_err(r.steps[0], G[f"traj/{name}/steps"]).max(axis=0)  # per parameter, over all steps
    ts = tol(m["ref_noise_steps_params"])
    et = rel_err(r.train_loss[0], G[f"traj/{name}/train_loss"]).max()
    ev = rel_err(r.val_loss[0], G[f"traj/{name}/val_loss"]).max()
    print(f"{name}: per-step params rel err / tol per parameter {np.array2string(es, precision=1)} / "
          f"{np.array2string(ts, precision=1)}, train loss {et:.3e} "
          f"(tol {tol(m['ref_noise_train_loss']):.1e}), val loss {ev:.3e} (tol {tol(m['ref_noise_val_loss']):.1e})")
    assert int(r.flag[0]) == 0
    assert (es <= ts).all(), (name, es, ts)
    assert et <= tol(m["ref_noise_train_loss"]), (name, et)
    assert ev <= tol(m["ref_noise_val_loss"]), (name, ev)
    assert np.array_equal(r.lr[0], G[f"traj/{name}/lr"]), (r.lr[0], G[f"traj/{name}/lr"])
    return r
