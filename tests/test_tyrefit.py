"""Tyre fit (csrc/mr_tyrefit.h) on the host build of the source, against tests/golden/tyrefit_golden.*.

* loss and gradient vs the reference's torch fp64 model (tolerance 100 x its own spread under row
  permutations, per component, floor 1e-13; at the degenerate load the loss and the a3..a5 components, where
  torch is an oracle);
* Fy, dFy/da[0..8] and an 8-row loss gradient at the degenerate load vs mpmath, 1e-10 relative.
  Measured maxima (host build): default coefficients 2.3e-15 (Fy, dFy/da) and 2.3e-15 (8-row loss
  gradient); pacejka-1's front tyre 5.9e-16.  Those coefficients sit on a zero of cos(a4 atan(a5 Fz))
  (1.0467e-12 exactly, 1.3050e-12 in plain fp64: the product a4 * atan(a5 Fz) ~ -4208 rounds at 4.5e-13),
  which dFy/da4 and dFy/da5 carry as a factor: plain fp64 is 25 % off there, the double-double angle of
  tf_psi_trig (mr_tyrefit.h) is what this case checks;
* optimiser trajectories (every step; SGD and Adam also with L2 weight decay) and the ReduceLROnPlateau
  history vs torch.optim; per-run shuffles (perm_stride_run != 0) against the same run alone;
* finite differences of the twin's own loss (consistency), argument errors, the result object.
"""
import ctypes

import numpy as np
import pytest

import tyrefit_cases as tc
from mpcracing import abi
from mpcracing import tyrefit as tf


def _lg(rows, params, Fz, kind):
    loss, grad = tf.loss_grad(rows, params, Fz, kind, host_twin=True)
    return loss[0], grad[0]


def _fit(rows, kind, init, Fz, opt, lr, epochs, factor, patience, perm, weight_decay=None, **kw):
    return tf.fit_tyres(rows, rows, kind, init, Fz, 1, None, opt, lr, epochs, factor, patience, perm=perm,
                        weight_decay=weight_decay, host_twin=True, record_steps=True, **kw)


_PD = ctypes.POINTER(ctypes.c_double)


def _dparams(a, Fz, alpha):
    a = np.ascontiguousarray(a, np.float64)
    fy, d = np.zeros(1), np.zeros(9)
    abi.load_host_twin().mrh_pacejka_dparams(a.ctypes.data_as(_PD), float(Fz), float(alpha), fy.ctypes.data_as(_PD),
                                             d.ctypes.data_as(_PD))
    return fy[0], d


@pytest.mark.parametrize("case", tc.LOSS_GRAD_CASES)
def test_loss_grad_matches_reference(case):
    tc.check_loss_grad(case, _lg)


def test_degenerate_loss_gradient_matches_mpmath():
    tc.check_mp_loss8(_lg)


@pytest.mark.parametrize("tag", ["default", "pacejka1_front"])
def test_pacejka_parameter_derivatives_match_mpmath(tag):
    a = tc.G[f"mp/{tag}/a"]
    worst = np.zeros(10)
    for i, al in enumerate(tc.G["mp/alphas"]):
        fy, d = _dparams(a, tc.FZ_DEG, al)
        e = np.concatenate([tc.rel_err([fy], [tc.G[f"mp/{tag}/Fy"][i]]), tc.rel_err(d, tc.G[f"mp/{tag}/dFy"][i])])
        worst = np.maximum(worst, e)
    print(f"{tag}: max rel err of Fy, dFy/da0..a8 over {len(tc.G['mp/alphas'])} slip angles: {worst}")
    assert worst.max() <= tc.MP_TOL, worst


@pytest.mark.parametrize("name", tc.TRAJECTORIES)
def test_trajectory_matches_torch_optim(name):
    r = tc.check_trajectory(name, _fit)
    if name == "lin_sched":
        assert tc.META["trajectories"][name]["halvings"] >= 2 and r.lr[0][-1] < r.lr[0][0]


@pytest.mark.parametrize("kind", ["linear", "pacejka"])
def test_gradient_matches_finite_differences(kind):
    # consistency of the twin's analytic gradient with its own loss (well-conditioned load): central
    # differences with step h |p|, truncation O(h^2) and rounding eps / h -> 1e-5 at h = 1e-5 ... 1e-6
    name = "lin_65000" if kind == "linear" else "pac_well"
    p0, Fz = tc.G[f"{name}/params"], tc.G[f"{name}/Fz"]
    _, g = _lg(tc.ROWS, p0, Fz, kind)
    for j in range(len(p0)):
        h = 1e-5 * max(abs(p0[j]), 1e-2)
        pp, pm = p0.copy(), p0.copy()
        pp[j] += h
        pm[j] -= h
        fd = (_lg(tc.ROWS, pp, Fz, kind)[0] - _lg(tc.ROWS, pm, Fz, kind)[0]) / (pp[j] - pm[j])
        assert abs(fd - g[j]) <= 1e-5 * abs(g[j]) + 1e-9 * np.abs(g).max(), (j, fd, g[j])


def test_loss_grad_batch_of_sets_equals_single():
    p = np.stack([tc.G["pac_well/params"], tc.G["pac_well/params"] * 1.01, tc.G["pac_well/params"]])
    Fz = np.full((3, 2), tc.FZ_WELL)
    loss, grad = tf.loss_grad(tc.ROWS, p, Fz, "pacejka", host_twin=True)
    l1, g1 = tf.loss_grad(tc.ROWS, p[1], Fz[1], "pacejka", host_twin=True)
    assert loss[0] == loss[2] and np.array_equal(grad[0], grad[2])
    assert loss[1] == l1[0] and np.array_equal(grad[1], g1[0])


@pytest.mark.parametrize("n", [5, 64])
def test_single_minibatch_sgd_step_is_loss_grad(n):
    # one epoch over n <= 64 rows is one step: p1 = p0 - lr * grad of the same rows, bit for bit
    rows, p0 = tc.ROWS[:n], np.array([65000.0, 64000.0])
    lr = 1e9
    perm = np.arange(n, dtype=np.int32)[::-1].reshape(1, n).copy()
    r = tf.fit_tyres(rows, rows, "linear", p0, None, 1, None, "sgd", lr, 1, perm=perm, host_twin=True)
    loss, g = tf.loss_grad(rows[perm[0]], p0, None, "linear", host_twin=True)
    assert np.array_equal(r.p_final[0], p0 - lr * g[0]) and r.train_loss[0, 0] == loss[0] and r.flag[0] == 0
    assert r.val_loss[0, 0] == tf.loss_grad(rows, r.p_final[0], None, "linear", host_twin=True)[0][0]


def test_nan_seed_sets_flag_and_leaves_other_runs_alone():
    init = np.tile(np.concatenate([tf.PACEJKA_INIT, tf.PACEJKA_INIT]), (3, 1))
    init[1, 4] = np.nan
    perm = tc.G["perm2"]
    kw = dict(Fz=tc.FZ_WELL, optimizer="adam", lr=1e-3, epochs=2, perm=perm, host_twin=True)
    r = tf.fit_tyres(tc.ROWS, tc.ROWS, "pacejka", init, runs=3, **kw)
    alone = tf.fit_tyres(tc.ROWS, tc.ROWS, "pacejka", init[0], runs=1, **kw)
    assert r.flag.tolist() == [0, 1, 0]
    assert np.isnan(r.train_loss[1]).all() and np.isnan(r.val_loss[1]).all()
    assert np.array_equal(r.p_final[1], init[1], equal_nan=True)
    for k in (0, 2):
        assert np.array_equal(r.p_final[k], alone.p_final[0]) and np.array_equal(r.val_loss[k], alone.val_loss[0])
    assert r.best_run in (0, 2)


def test_argument_errors():
    rows = tc.ROWS
    with pytest.raises(ValueError, match="unknown tyre kind"):
        tf.fit_tyres(rows, rows, "mlp", host_twin=True)
    with pytest.raises(ValueError, match="unknown optimizer"):
        tf.fit_tyres(rows, rows, "linear", optimizer="lbfgs", host_twin=True)
    with pytest.raises(ValueError, match="runs < 1"):
        tf.fit_tyres(rows, rows, "linear", runs=0, host_twin=True)
    with pytest.raises(ValueError, match=r"rows \[n\]\[15\]"):
        tf.fit_tyres(rows[:, :14], rows, "linear", host_twin=True)
    bad = np.arange(200, dtype=np.int32).reshape(1, 200).copy()
    bad[0, 17] = 200
    with pytest.raises(RuntimeError):  # perm entry out of range: refused before any row is read
        tf.fit_tyres(rows, rows, "linear", epochs=1, perm=bad, host_twin=True)
    bad[0, 17] = -1
    with pytest.raises(RuntimeError):
        tf.fit_tyres(rows, rows, "linear", epochs=1, perm=bad, host_twin=True)
    # the C layer itself: unknown kind / optimiser, n_train < 1, R < 1
    lib = abi.load_host_twin()
    c = abi.MRTyrefitConfig()
    lib.mrh_tyrefit_config_default(ctypes.byref(c))
    assert (c.kind, c.optimizer, c.epochs, c.patience, c.factor) == (1, 1, 25, 2, 0.5)
    assert (c.m, c.Iz, c.lf, c.lr, c.max_steer_deg, c.C_wheel) == (1845.0, 3960.0, 0.8, 2.0, 70.0, 2 * 3.14 * 0.37)
    z = np.zeros(64)
    p = z.ctypes.data_as(ctypes.c_void_p)
    pi = np.zeros(64, np.int32).ctypes.data_as(ctypes.c_void_p)

    def fit(cfg, n_train=1, R=1):
        return lib.mrh_tyre_fit(ctypes.byref(cfg), n_train, p, 1, p, R, p, p, p, pi, 0, p, p, p, p, p, pi, None, 1)
    c.kind, c.epochs = 0, 1
    for field, value in (("kind", 7), ("optimizer", 3), ("optimizer", -1)):
        c2 = abi.MRTyrefitConfig.from_buffer_copy(c)
        setattr(c2, field, value)
        assert fit(c2) == -1
        assert lib.mrh_tyre_loss_grad(ctypes.byref(c2), 1, p, 1, p, p, p, p) == -1
    assert fit(c, n_train=0) == -1 and fit(c, R=0) == -1


def test_state_dict_and_tyres():
    import torch
    r = _fit(tc.ROWS, "pacejka", tc.G["traj/pac_adam/init"], tc.G["traj/pac_adam/Fz"], "adam", 1e-3, 2, 0.5, 2,
             tc.G["perm2"])
    sd = r.state_dict()
    assert list(sd) == ["front_tire.a", "front_tire.Fz", "back_tire.a", "back_tire.Fz"]
    assert [tuple(v.shape) for v in sd.values()] == [(9,), (1,), (9,), (1,)]
    assert all(v.dtype == torch.float64 for v in sd.values())
    (af, Fzf), (ar, Fzr) = r.tyres
    assert np.array_equal(af, r.params[:9]) and np.array_equal(ar, r.params[9:]) and Fzf == Fzr == tc.FZ_WELL
    assert np.array_equal(sd["front_tire.a"].numpy(), af) and float(sd["back_tire.Fz"]) == Fzr
    assert np.array_equal(r.params, r.p_best[r.best_run]) and np.nanmin(r.val_loss[0]) == r.best_val_loss
    # .tyres feeds the solver's tyre law: pacejka_coef + pacejka_jet (mrh_pacejka) give the fit's Fy
    lib = abi.load_host_twin()
    for a, Fz in ((af, Fzf), (ar, Fzr)):
        for al in (-0.2, -1e-3, 0.0, 0.05, 0.3):
            out = np.zeros(3)
            lib.mrh_pacejka(np.ascontiguousarray(a).ctypes.data_as(_PD), Fz, al, 0, out.ctypes.data_as(_PD))
            assert abs(out[0] - _dparams(a, Fz, al)[0]) <= 1e-12 * abs(out[0])
    with pytest.raises(ValueError):
        r.linear
    rl = _fit(tc.ROWS, "linear", tc.G["traj/lin_adam/init"], None, "adam", 10.0, 2, 0.5, 2, tc.G["perm2"])
    sdl = rl.state_dict()
    assert list(sdl) == ["front_tire.stiffness", "back_tire.stiffness"]
    assert all(tuple(v.shape) == (1,) and v.dtype == torch.float64 for v in sdl.values())
    assert rl.linear == {"Cf": float(rl.params[0]), "Cr": float(rl.params[1])}
    assert set(rl.linear) <= {n for n, _ in abi.MRConfig._fields_}
    with pytest.raises(ValueError):
        rl.tyres


def test_config_struct_layout_matches_header(tmp_path):
    import os
    import subprocess
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpcracing.h")
    src = ('#include "%s"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%%zu %%zu %%zu\\n",'
           'sizeof(mr_tyrefit_config), offsetof(mr_tyrefit_config, factor), '
           'offsetof(mr_tyrefit_config, max_steer_deg));}' % header)
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-o", str(tmp_path / "t"), str(tmp_path / "t.c")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()]
    C = abi.MRTyrefitConfig
    assert got == [ctypes.sizeof(C), C.factor.offset, C.max_steer_deg.offset]
    assert abi.ABI_VERSION == 103 and "#define MR_ABI_VERSION 103" in open(header).read()


def test_load_rows(tmp_path):
    cols = tf.FEATURES + tf.TARGETS
    order = cols[::-1]  # columns are found by name, whatever their order in the file
    f = tmp_path / "rows.csv"
    with open(f, "w") as fh:
        fh.write(",".join(order) + "\n")
        for row in tc.ROWS[:7]:
            fh.write(",".join(repr(float(v)) for v in row[::-1]) + "\n")
    assert np.array_equal(tf.load_rows(str(f)), tc.ROWS[:7])


def test_per_run_perm_equals_the_run_alone_and_is_checked():
    # perm_stride_run != 0: run r reads its own shuffle; an out-of-range entry in a later run's perm is refused
    R, n, E = 3, 200, 2
    perms = np.stack([tf.make_perm(s, E, n) for s in (11, 12, 13)])
    assert not np.array_equal(perms[0], perms[2])
    kw = dict(kind="linear", optimizer="adam", lr=10.0, epochs=E, record_steps=True, host_twin=True)
    r = tf.fit_tyres(tc.ROWS, tc.ROWS, runs=R, perm=perms, **kw)
    for k in range(R):
        alone = tf.fit_tyres(tc.ROWS, tc.ROWS, runs=1, perm=perms[k], **kw)
        assert np.array_equal(r.steps[k], alone.steps[0]) and np.array_equal(r.val_loss[k], alone.val_loss[0])
    assert not np.array_equal(r.steps[0], r.steps[2])
    bad = perms.copy()
    bad[2, 1, 199] = n
    with pytest.raises(RuntimeError, match="perm entry out of range"):
        tf.fit_tyres(tc.ROWS, tc.ROWS, runs=R, perm=bad, **kw)
    with pytest.raises(RuntimeError, match="R < 1|n_train < 1|unknown"):
        c = tf.make_config("linear", host_twin=True)
        c.optimizer = 9
        be = tf._Host()
        z = np.zeros(64)
        be.check(be.lib.mrh_tyre_loss_grad(ctypes.byref(c), 1, be.ptr(z), 1, be.ptr(z), be.ptr(z), be.ptr(z), be.ptr(z)))


def test_result_of_runs_that_all_stopped_is_refused():
    init = np.full((2, 2), np.nan)
    r = tf.fit_tyres(tc.ROWS, tc.ROWS, "linear", init, runs=2, epochs=1, perm=tc.G["perm2"][:1], host_twin=True)
    assert r.flag.tolist() == [1, 1] and not r.ok
    for attr in ("params", "linear"):
        with pytest.raises(RuntimeError, match="no run finished an epoch"):
            getattr(r, attr)
    with pytest.raises(RuntimeError, match="no run finished an epoch"):
        r.state_dict()
