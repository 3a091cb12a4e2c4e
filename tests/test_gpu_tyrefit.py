"""Tyre fit on gfx950 (mr_tyre_loss_grad, mr_tyre_fit) against tests/golden/tyrefit_golden.* and the host
build of the same source.

Tolerances as in test_tyrefit.py: 100 x the reference's own spread under a row permutation (floor 1e-13),
1e-10 against mpmath; device vs host build at the same 100 x spread (libm differs, so not bit-equal).
Launch-shape independence and repeatability are bitwise.  All cases run at the fixture's n <= 200.
"""
import ctypes

import numpy as np
import pytest
import torch

import tyrefit_cases as tc
from mpcracing import abi
from mpcracing import tyrefit as tf

pytestmark = pytest.mark.gpu


def _lg(rows, params, Fz, kind):
    loss, grad = tf.loss_grad(rows, params, Fz, kind)
    return loss[0], grad[0]


def _fit(rows, kind, init, Fz, opt, lr, epochs, factor, patience, perm, weight_decay=None, **kw):
    return tf.fit_tyres(rows, rows, kind, init, Fz, 1, None, opt, lr, epochs, factor, patience, perm=perm,
                        weight_decay=weight_decay, record_steps=True, **kw)


@pytest.mark.parametrize("case", tc.LOSS_GRAD_CASES)
def test_device_loss_grad_matches_reference_and_host(case):
    tc.check_loss_grad(case, _lg)
    m = tc.META["cases"][case]
    name, n = case.split("/")[0], m["n"]
    args = (tc.ROWS[:n], tc.G[f"{name}/params"], tc.G[f"{name}/Fz"], m["kind"])
    (ld, gd), (lh, gh) = tf.loss_grad(*args), tf.loss_grad(*args, host_twin=True)
    # every component is well conditioned in the cancellation-free form: all 18 are compared
    el, eg = tc.rel_err(ld, lh).max(), tc.rel_err(gd, gh).max()
    print(f"{case}: device vs host loss {el:.3e}, grad {eg:.3e}")
    assert el <= tc.tol(m["ref_noise_loss"]) and eg <= tc.tol(m["ref_noise_grad"]), (el, eg)
    assert (tc.rel_err(gd[0][m["components"]], gh[0][m["components"]]) <= tc.tol(m["ref_noise_grad_components"])).all()


def test_device_degenerate_loss_gradient_matches_mpmath():
    tc.check_mp_loss8(_lg)


@pytest.mark.parametrize("name", tc.TRAJECTORIES)
def test_device_trajectory_matches_torch_optim_and_host(name):
    r = tc.check_trajectory(name, _fit)
    m = tc.META["trajectories"][name]
    h = tf.fit_tyres(tc.ROWS, tc.ROWS, m["kind"], tc.G[f"traj/{name}/init"], tc.G[f"traj/{name}/Fz"], 1, None,
                     m["optimizer"], m["lr"], m["epochs"], m["factor"], m["patience"], perm=tc.G[m["perm"]],
                     weight_decay=m["weight_decay"], host_twin=True, record_steps=True)
    es = tc.rel_err(r.steps, h.steps).max()
    assert (tc.rel_err(r.steps[0], h.steps[0]).max(axis=0) <= tc.tol(m["ref_noise_steps_params"])).all()
    et, ev = tc.rel_err(r.train_loss, h.train_loss).max(), tc.rel_err(r.val_loss, h.val_loss).max()
    print(f"{name}: device vs host steps {es:.3e}, train loss {et:.3e}, val loss {ev:.3e}")
    assert es <= tc.tol(m["ref_noise_steps"]) and et <= tc.tol(m["ref_noise_train_loss"])
    assert ev <= tc.tol(m["ref_noise_val_loss"]) and np.array_equal(r.lr, h.lr)


def _many_runs(R):
    rng = np.random.default_rng(5)
    init = np.tile(np.concatenate([tf.PACEJKA_INIT, tf.PACEJKA_INIT]), (R, 1)) * (1 + 0.01 * rng.standard_normal((R, 18)))
    init[0] = np.concatenate([tf.PACEJKA_INIT, tf.PACEJKA_INIT])
    lr = 1e-3 * (1 + np.arange(R) % 7)
    betas = np.stack([0.9 - 0.001 * (np.arange(R) % 5), np.full(R, 0.999)], axis=1)
    return init, lr, betas


def test_run_is_independent_of_the_launch_and_repeatable():
    R = 130  # more than two waves per SIMD row of a CU, and no multiple of anything
    init, lr, betas = _many_runs(R)
    kw = dict(Fz=tc.FZ_WELL, optimizer="adamw", epochs=2, perm=tc.G["perm2"], record_steps=True)
    a = tf.fit_tyres(tc.ROWS, tc.ROWS, "pacejka", init, runs=R, lr=lr, betas=betas, **kw)
    b = tf.fit_tyres(tc.ROWS, tc.ROWS, "pacejka", init, runs=R, lr=lr, betas=betas, **kw)
    alone = tf.fit_tyres(tc.ROWS, tc.ROWS, "pacejka", init[0], runs=1, lr=lr[0], betas=betas[:1], **kw)
    assert (a.flag == 0).all()
    for k in ("p_final", "p_best", "train_loss", "val_loss", "lr", "steps"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k          # repeated launches: bitwise
        assert np.array_equal(getattr(a, k)[0], getattr(alone, k)[0]), k  # run 0 of 130 == the run alone
    assert len({a.p_final[r].tobytes() for r in range(R)}) == R  # the runs really differ


def test_loss_grad_is_independent_of_the_number_of_sets():
    P = 70
    p = np.tile(tc.G["pac_well/params"], (P, 1)) * (1 + 1e-3 * np.arange(P))[:, None]
    Fz = np.full((P, 2), tc.FZ_WELL)
    la, ga = tf.loss_grad(tc.ROWS, p, Fz, "pacejka")
    lb, gb = tf.loss_grad(tc.ROWS, p, Fz, "pacejka")
    l1, g1 = tf.loss_grad(tc.ROWS, p[69], Fz[69], "pacejka")
    assert np.array_equal(la, lb) and np.array_equal(ga, gb)
    assert la[69] == l1[0] and np.array_equal(ga[69], g1[0])


@pytest.mark.parametrize("n", [5, 64])
def test_single_minibatch_sgd_step_is_loss_grad(n):
    # one epoch over n <= 64 rows is one step (n = 5: a single partial minibatch, mean over 5 x 6)
    rows, p0 = tc.ROWS[:n], np.array([65000.0, 64000.0])
    lr = 1e9
    perm = np.arange(n, dtype=np.int32)[::-1].reshape(1, n).copy()
    r = tf.fit_tyres(rows, rows, "linear", p0, None, 1, None, "sgd", lr, 1, perm=perm)
    loss, g = tf.loss_grad(rows[perm[0]], p0, None, "linear")
    assert np.array_equal(r.p_final[0], p0 - lr * g[0]) and r.train_loss[0, 0] == loss[0] and r.flag[0] == 0
    assert r.val_loss[0, 0] == tf.loss_grad(rows, r.p_final[0], None, "linear")[0][0]
    h = tf.fit_tyres(rows, rows, "linear", p0, None, 1, None, "sgd", lr, 1, perm=perm, host_twin=True)
    assert tc.rel_err(r.p_final, h.p_final).max() <= 1e-13


def test_nan_seed_sets_flag_and_leaves_other_runs_alone():
    init = np.tile(np.concatenate([tf.PACEJKA_INIT, tf.PACEJKA_INIT]), (3, 1))
    init[1, 4] = np.nan
    kw = dict(Fz=tc.FZ_WELL, optimizer="adam", lr=1e-3, epochs=2, perm=tc.G["perm2"])
    r = tf.fit_tyres(tc.ROWS, tc.ROWS, "pacejka", init, runs=3, **kw)
    alone = tf.fit_tyres(tc.ROWS, tc.ROWS, "pacejka", init[0], runs=1, **kw)
    assert r.flag.tolist() == [0, 1, 0]
    assert np.isnan(r.train_loss[1]).all() and np.isnan(r.val_loss[1]).all() and np.isnan(r.lr[1]).all()
    assert np.array_equal(r.p_final[1], init[1], equal_nan=True)
    for k in (0, 2):
        assert np.array_equal(r.p_final[k], alone.p_final[0]) and np.array_equal(r.val_loss[k], alone.val_loss[0])
    assert r.best_run in (0, 2)


def test_device_argument_errors():
    lib = abi.load_product()
    rows = tc.ROWS

    def err():
        return lib.mr_last_error().decode()
    bad = np.arange(200, dtype=np.int32).reshape(1, 200).copy()
    for v in (200, -1, 2 ** 31 - 1):  # refused by the checking pass: never used as a row index
        bad[0, 199] = v
        with pytest.raises(RuntimeError, match="perm entry out of range"):
            tf.fit_tyres(rows, rows, "linear", epochs=1, perm=bad)
    c = abi.MRTyrefitConfig()
    assert lib.mr_tyrefit_config_default(ctypes.byref(c)) == 0
    assert (c.kind, c.optimizer, c.epochs, c.patience, c.factor) == (1, 1, 25, 2, 0.5)
    d = torch.zeros(64, dtype=torch.float64, device="cuda")
    di = torch.zeros(64, dtype=torch.int32, device="cuda")
    p, pi = ctypes.c_void_p(d.data_ptr()), ctypes.c_void_p(di.data_ptr())

    def fit(cfg, n_train=1, R=1):
        return lib.mr_tyre_fit(ctypes.byref(cfg), n_train, p, 1, p, R, p, p, p, pi, 0, p, p, p, p, p, pi, None, None)
    c.kind, c.epochs = 0, 1
    for field, value, msg in (("kind", 7, "unknown tyre kind"), ("optimizer", 3, "unknown optimiser")):
        c2 = abi.MRTyrefitConfig.from_buffer_copy(c)
        setattr(c2, field, value)
        assert fit(c2) == -1 and msg in err()
        assert lib.mr_tyre_loss_grad(ctypes.byref(c2), 1, p, 1, p, p, p, p, None) == -1 and msg in err()
    assert fit(c, n_train=0) == -1 and "n_train < 1" in err()
    assert fit(c, R=0) == -1 and "R < 1" in err()
    assert fit(c) == 0  # the same arrays with valid arguments run
    torch.cuda.synchronize()


def test_fitted_tyres_feed_the_solver():
    from mpcracing import workload as wl
    from mpcracing.batch import solver_for_config
    r = tf.fit_tyres(tc.ROWS, tc.ROWS, "pacejka", runs=3, seeds=[1, 2, 3], lr=[1e-3, 3e-3, 1e-2], epochs=3)
    assert (r.flag == 0).all() and r.best_val_loss <= r.val_loss[:, 0].min()
    s = solver_for_config("C5", 4, tyres=r.tyres)
    out = {k: v.cpu().numpy() for k, v in s.solve(wl.make_batch("C5", limit=4)).items()}
    assert all(np.isfinite(out[k]).all() for k in ("X", "U", "S", "eC", "eL"))
    assert (out["iters"] > 0).all()


def test_per_run_perm_equals_the_run_alone_and_is_checked():
    # perm_stride_run != 0: run r reads its own shuffle; the checking pass covers every run's perm
    R, n, E = 3, 200, 2
    perms = np.stack([tf.make_perm(s, E, n) for s in (11, 12, 13)])
    kw = dict(kind="linear", optimizer="adam", lr=10.0, epochs=E, record_steps=True)
    r = tf.fit_tyres(tc.ROWS, tc.ROWS, runs=R, perm=perms, **kw)
    for k in range(R):
        alone = tf.fit_tyres(tc.ROWS, tc.ROWS, runs=1, perm=perms[k], **kw)
        assert np.array_equal(r.steps[k], alone.steps[0]) and np.array_equal(r.val_loss[k], alone.val_loss[0])
    assert not np.array_equal(r.steps[0], r.steps[2])
    for where in ((2, 1, 199), (1, 0, 0)):
        bad = perms.copy()
        bad[where] = n
        with pytest.raises(RuntimeError, match="perm entry out of range"):
            tf.fit_tyres(tc.ROWS, tc.ROWS, runs=R, perm=bad, **kw)
