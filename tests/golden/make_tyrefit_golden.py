"""Generate tests/golden/tyrefit_golden.npz / tyrefit_golden.json: what the reference's torch training
code computes for the tyre fit, and 50-digit values where torch is no oracle.

TEST FIXTURE GENERATOR (build container only, CPU only; no test imports it).

It imports the reference's ``learning.vehicle`` (never copied) with tests/golden/casadi_standin.py
registered as ``casadi``, builds ``Vehicle('linear')`` and, for the Pacejka cases, replaces its tyres by
``Pacejka()`` (``Vehicle('pacejka')`` raises), all in torch fp64.  Data: the first 200 rows of
``learning/data/nodamp-pid-79/validate.csv`` (3 x 64 + 8: the last minibatch is partial), used as the
training and the validation set of every case.

Recorded:
* loss and gradient (nn.MSELoss, autograd) at n = 8, 64, 200: linear at 65000 / 65000 and at
  linear-best's values, Pacejka defaults at Fz = 18.09945 (the load in kN, well conditioned);
* at the reference's load Fz = 18099.44921875 torch's gradient is rounding noise for a0..a2, a6..a8
  (measured here: ``degenerate`` in the json), so only its a3..a5 components are an oracle; Fy and
  dFy/da[0..8] at 17 slip angles and the loss gradient over the first 8 rows are recorded from mpmath
  (80 digits) for the default coefficients and for pacejka-1's front tyre;
* optimiser trajectories (parameters after every step of 2 epochs, explicit ``perm``) by stepping
  torch.optim on the reference's model, and one 8-epoch ReduceLROnPlateau history;
* ``ref_noise``: every quantity is evaluated again with the rows permuted (32 permutations; trajectories:
  4, within each minibatch); the largest componentwise relative difference is the reference's own noise,
  and each test's tolerance is 100 x that (floor 1e-13).

Usage: python tests/golden/make_tyrefit_golden.py <path to the reference checkout>
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FEATURES = ['X_0', 'Y_0', 'yaw_0', 'vx_0', 'vy_0', 'yawdot_0', 'throttle_0', 'steer_0', 'last_ts']
TARGETS = ['X_1', 'Y_1', 'yaw_1', 'vx_1', 'vy_1', 'yawdot_1']
FZ_WELL = 18.09945
N_ROWS = 200
BATCH = 64
N_PERMUTATIONS = 32


def rel_each(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.maximum(np.abs(a), 1e-300)


def rel_spread(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    den = np.maximum(np.abs(a), 1e-300)
    return float(np.max(np.abs(a - b) / den)) if a.size else 0.0


def main():
    ref = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.environ.get("MR_REFERENCE_DIR", "")
    if not os.path.isdir(os.path.join(ref, "learning")):
        raise SystemExit("usage: make_tyrefit_golden.py <reference checkout>")
    os.environ["PYTHONBREAKPOINT"] = "0"
    sys.path.insert(0, HERE)
    import casadi_standin as cs
    cs.install()
    sys.path.insert(0, ref)
    import mpmath as mp
    import torch
    from learning.vehicle import Pacejka, Vehicle
    from models.VehicleParameters import VehicleParameters as VP
    torch.set_num_threads(1)
    mp.mp.dps = 80

    raw = np.genfromtxt(os.path.join(ref, "learning", "data", "nodamp-pid-79", "validate.csv"), delimiter=",",
                        names=True, max_rows=N_ROWS)
    rows = np.stack([raw[c] for c in FEATURES + TARGETS], axis=1).astype(np.float64)  # [200][15]
    assert rows.shape == (N_ROWS, 15) and np.isfinite(rows).all()
    Xall, Yall = torch.tensor(rows[:, :9]), torch.tensor(rows[:, 9:])
    rng = np.random.default_rng(20241019)
    FZ_DEG = float(np.float32(VP.m * 9.81))
    A_DEFAULT = Pacejka().a.detach().numpy().astype(np.float64)  # float32-rounded defaults, as the reference's
    lin_best = torch.load(os.path.join(ref, "learning", "models", "linear-best", "model"), map_location="cpu")
    pac1 = torch.load(os.path.join(ref, "learning", "models", "pacejka-1", "model"), map_location="cpu")
    A_PAC1 = pac1["front_tire.a"].double().numpy()

    def model(kind, params, Fz=None):
        v = Vehicle('linear')
        if kind == "pacejka":
            v.front_tire, v.back_tire = Pacejka(), Pacejka()
        v = v.to(dtype=torch.float64)
        with torch.no_grad():
            if kind == "pacejka":
                v.front_tire.a.copy_(torch.tensor(params[:9]))
                v.back_tire.a.copy_(torch.tensor(params[9:]))
                v.front_tire.Fz.fill_(Fz[0])
                v.back_tire.Fz.fill_(Fz[1])
            else:
                v.front_tire.stiffness.fill_(params[0])
                v.back_tire.stiffness.fill_(params[1])
        return v

    def flat(v):
        return np.concatenate([p.detach().numpy().ravel() for p in v.parameters()])

    crit = torch.nn.MSELoss()

    def loss_grad(kind, params, Fz, idx):
        v = model(kind, params, Fz)
        loss = crit(v(Xall[idx]).squeeze(), Yall[idx])
        loss.backward()
        return float(loss.detach()), np.concatenate([p.grad.numpy().ravel() for p in v.parameters()])

    npz = {"rows": rows}
    meta = {"cases": {}, "trajectories": {}, "torch": torch.__version__, "mpmath": mp.__version__,
            "Fz_well": FZ_WELL, "Fz_degenerate": FZ_DEG}

    # ---- loss / gradient cases ---------------------------------------------------------------------
    lg = {
        "lin_65000": ("linear", np.array([65000.0, 65000.0]), None),
        "lin_best": ("linear", np.array([float(lin_best["front_tire.stiffness"]),
                                         float(lin_best["back_tire.stiffness"])]), None),
        "pac_well": ("pacejka", np.concatenate([A_DEFAULT, A_DEFAULT]), [FZ_WELL, FZ_WELL]),
        "pac_deg": ("pacejka", np.concatenate([A_DEFAULT, A_DEFAULT]), [FZ_DEG, FZ_DEG]),
    }
    BCD_IDX = [3, 4, 5, 12, 13, 14]
    for name, (kind, params, Fz) in lg.items():
        npz[f"{name}/params"] = params
        npz[f"{name}/Fz"] = np.array(Fz if Fz else [0.0, 0.0])
        for n in (8, 64, 200):
            idx = np.arange(n)
            l, g = loss_grad(kind, params, Fz, idx)
            comp = BCD_IDX if name == "pac_deg" else list(range(len(g)))
            noise_l, noise_c = 0.0, np.zeros(len(comp))
            for _ in range(N_PERMUTATIONS):  # the spread is the largest difference over these permutations
                l2, g2 = loss_grad(kind, params, Fz, rng.permutation(n))
                noise_l, noise_c = max(noise_l, rel_spread([l], [l2])), np.maximum(noise_c, rel_each(g[comp], g2[comp]))
            noise_g = float(noise_c.max())
            npz[f"{name}/n{n}/loss"] = np.array(l)
            npz[f"{name}/n{n}/grad"] = g
            meta["cases"][f"{name}/n{n}"] = {
                "kind": kind, "n": n, "components": comp,
                "ref_noise_loss": noise_l, "ref_noise_grad": noise_g,
                "ref_noise_grad_components": [float(v) for v in noise_c]}  # per gradient component of `components`
            if name == "pac_deg":
                # a0..a2, a6..a8 of both tyres under the last of the permutations (components torch returns as
                # exactly 0 are counted, not divided by)
                rest = np.array([i for i in range(18) if i not in BCD_IDX])
                nz = rest[g[rest] != 0]
                change = np.abs(g[nz] - g2[nz]) / np.abs(g[nz])
                meta["cases"][f"{name}/n{n}"]["noise_other_components"] = {
                    "max_abs_grad": float(np.max(np.abs(g[rest]))), "min_abs_nonzero_grad": float(np.min(np.abs(g[nz]))),
                    "exactly_zero": int(len(rest) - len(nz)),
                    "rel_change_under_permutation_min": float(change.min()),
                    "rel_change_under_permutation_max": float(change.max())}

    # ---- mpmath: Fy, dFy/da and an 8-row loss gradient at the degenerate load ---------------------------
    def fy_mp(a, Fz, al):
        C = a[0]
        D = (a[1] * Fz + a[2]) * Fz
        BCD = a[3] * mp.sin(a[4] * mp.atan(a[5] * Fz))
        B = BCD / (C * D)
        E = a[6] * Fz ** 2 + a[7] * Fz + a[8]
        if al == 0:
            return mp.mpf(0)
        phi = (1 - E) * al + (E / B) * mp.atan(B * al)
        return D * mp.sin(C * mp.atan(B * phi))

    def dfy_mp(a, Fz, al):
        out = []
        for i in range(9):
            def f(t, i=i):
                b = list(a)
                b[i] = t
                return fy_mp(b, Fz, al)
            out.append(mp.diff(f, a[i]))
        return out

    alphas = np.array([-0.3, -0.2, -0.1, -0.03, -0.01, -1e-3, -1e-4, -1e-6, 0.0, 1e-6, 1e-4, 1e-3, 0.01, 0.03, 0.1,
                       0.2, 0.3])
    npz["mp/alphas"] = alphas
    for tag, a64 in (("default", A_DEFAULT), ("pacejka1_front", A_PAC1)):
        am = [mp.mpf(float(x)) for x in a64]
        Fzm = mp.mpf(FZ_DEG)
        fy = np.array([float(fy_mp(am, Fzm, mp.mpf(float(al)))) for al in alphas])
        dfy = np.array([[float(d) for d in dfy_mp(am, Fzm, mp.mpf(float(al)))] for al in alphas])
        npz[f"mp/{tag}/a"] = a64
        npz[f"mp/{tag}/Fy"] = fy
        npz[f"mp/{tag}/dFy"] = dfy

    def forward_mp(x, af, ar, Fz):
        m_, Iz, lf, lr = [mp.mpf(float(v)) for v in (VP.m, VP.Iz, VP.lf, VP.lr)]
        X, Y, yaw, vx, vy, r, thr, steer, dt = [mp.mpf(float(v)) for v in x[:9]]
        f = lambda v: mp.mpf(float(v))  # noqa: E731
        rpm = (vx / f(VP.C_wheel)) * 60 * f(VP.R) * f(4.5)
        eta = f(-0.00004428225806) * rpm + f(1.282413306)
        Fx = thr * eta * f(VP.T_max) * f(VP.R) / f(VP.r_wheel) - f(0.5) * f(VP.rho) * f(VP.C_d) * f(VP.A_f) * vx ** 2 \
            - f(VP.C_roll) * f(VP.m) * f(VP.g)
        vel = mp.sqrt(vx ** 2 + vy ** 2) * f(3.6)
        gain = f(-0.001971664699) * vel + f(0.986547)
        delta = (steer * gain * f(VP.max_steer) / 360) * 2 * f(3.14)
        thf = mp.atan2(vy + lf * r, vx + f(0.1))
        thr_ = mp.atan2(vy - lr * r, vx + f(0.1))
        Fyf, Fyr = fy_mp(af, Fz, delta - thf), fy_mp(ar, Fz, -thr_)
        vxd = (Fx - Fyf * mp.sin(delta)) / m_ + vy * r
        vyd = (Fyf * mp.cos(delta) + Fyr) / m_ - vx * r
        rd = (Fyf * mp.cos(delta) * lf - Fyr * lr) / Iz
        return [X + (vx * mp.cos(yaw) - vy * mp.sin(yaw)) * dt, Y + (vx * mp.sin(yaw) + vy * mp.cos(yaw)) * dt,
                yaw + r * dt, vx + vxd * dt, vy + vyd * dt, r + rd * dt]

    def loss_mp(p, Fz, n):
        s = mp.mpf(0)
        for i in range(n):
            o = forward_mp(rows[i], p[:9], p[9:], Fz)
            s += sum((o[j] - mp.mpf(float(rows[i, 9 + j]))) ** 2 for j in range(6))
        return s / (n * 6)

    p0 = [mp.mpf(float(x)) for x in np.concatenate([A_DEFAULT, A_DEFAULT])]
    gmp = []
    for i in range(18):
        def f(t, i=i):
            q = list(p0)
            q[i] = t
            return loss_mp(q, mp.mpf(FZ_DEG), 8)
        gmp.append(float(mp.diff(f, p0[i])))
    npz["mp/loss8/loss"] = np.array(float(loss_mp(p0, mp.mpf(FZ_DEG), 8)))
    npz["mp/loss8/grad"] = np.array(gmp)
    tg = npz["pac_deg/n8/grad"]
    rest = [i for i in range(18) if i not in BCD_IDX]
    meta["degenerate"] = {
        "torch_vs_mpmath_rel_err_a3_a5": rel_spread(np.array(gmp)[BCD_IDX], tg[BCD_IDX]),
        "torch_vs_mpmath_rel_err_other_min": float(np.min(np.abs(tg[rest] - np.array(gmp)[rest]) /
                                                           np.abs(np.array(gmp)[rest]))),
        "torch_vs_mpmath_rel_err_other_max": rel_spread(np.array(gmp)[rest], tg[rest])}

    # ---- optimiser trajectories ----------------------------------------------------------------------
    def batches(perm_e, shuffle_within):
        out = []
        for b in range(0, N_ROWS, BATCH):
            idx = np.array(perm_e[b:b + BATCH])
            out.append(rng.permutation(idx) if shuffle_within else idx)
        return out

    def make_opt(name, v, lr, wd=None):
        kw = {} if wd is None else {"weight_decay": wd}  # None: the optimiser's default
        return {"sgd": torch.optim.SGD, "adam": torch.optim.Adam, "adamw": torch.optim.AdamW}[name](
            v.parameters(), lr=lr, **kw)

    def trajectory(kind, params, Fz, opt_name, lr, perm, shuffle_within, sched=None, wd=None):
        v = model(kind, params, Fz)
        opt = make_opt(opt_name, v, lr, wd)
        scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, factor=sched[0], patience=sched[1]) if sched else None
        steps, tl, vl, lrs = [], [], [], []
        for e in range(perm.shape[0]):
            running, bs = 0.0, batches(perm[e], shuffle_within)
            for idx in bs:
                opt.zero_grad()
                loss = crit(v(Xall[idx]).squeeze(), Yall[idx])
                loss.backward()
                opt.step()
                running += loss.item()
                steps.append(flat(v).copy())
            tl.append(running / len(bs))
            val = 0.0
            vb = batches(np.arange(N_ROWS), shuffle_within)
            with torch.no_grad():
                for idx in vb:
                    val += crit(v(Xall[idx]).squeeze(), Yall[idx]).item()
            vl.append(val / len(vb))
            if scheduler:
                scheduler.step(vl[-1])
            lrs.append(opt.param_groups[0]["lr"])
        return np.array(steps), np.array(tl), np.array(vl), np.array(lrs)

    perm2 = np.stack([rng.permutation(N_ROWS) for _ in range(2)]).astype(np.int32)
    perm8 = np.stack([rng.permutation(N_ROWS) for _ in range(8)]).astype(np.int32)
    npz["perm2"], npz["perm8"] = perm2, perm8
    lin0 = np.array([65000.0, 65000.0])
    pacw = np.concatenate([A_DEFAULT, A_DEFAULT])
    _, g0 = loss_grad("linear", lin0, None, np.arange(N_ROWS))
    sgd_lr = float(10.0 ** np.ceil(np.log10(1e-3 * 65000.0 / np.max(np.abs(g0)))))  # first step ~1e-3 relative
    trajs = {
        "lin_adam": ("linear", lin0, None, "adam", 10.0, perm2, None),
        "lin_sgd": ("linear", lin0, None, "sgd", sgd_lr, perm2, None),
        "pac_adam": ("pacejka", pacw, [FZ_WELL, FZ_WELL], "adam", 1e-3, perm2, None),
        "pac_adamw": ("pacejka", pacw, [FZ_WELL, FZ_WELL], "adamw", 1e-3, perm2, None),
    }
    # the scheduler case: the smallest Adam lr of this ladder at which the lr halves at least twice in 8 epochs
    for sched_lr in (10.0, 100.0, 300.0, 1000.0, 3000.0, 10000.0):
        lrs = trajectory("linear", lin0, None, "adam", sched_lr, perm8, False, (0.5, 0))[3]
        if lrs[-1] <= sched_lr / 4:
            break
    trajs["lin_sched"] = ("linear", lin0, None, "adam", sched_lr, perm8, (0.5, 0))
    # L2 weight decay (SGD, Adam): wd * stiffness is of the gradient's size (6.5e-9)
    trajs["lin_sgd_wd"] = ("linear", lin0, None, "sgd", sgd_lr, perm2, None, 1e-13)
    trajs["lin_adam_wd"] = ("linear", lin0, None, "adam", 10.0, perm2, None, 1e-13)
    for name, spec in trajs.items():
        kind, params, Fz, opt, lr, perm, sched = spec[:7]
        wd = spec[7] if len(spec) > 7 else None
        s, tl, vl, lrs = trajectory(kind, params, Fz, opt, lr, perm, False, sched, wd)
        noise = {"steps": 0.0, "train_loss": 0.0, "val_loss": 0.0}
        noise_p = np.zeros(s.shape[1])  # per parameter, over all steps
        lr_equal = True
        for _ in range(4):  # the spread is the largest difference over these within-minibatch permutations
            s2, tl2, vl2, lrs2 = trajectory(kind, params, Fz, opt, lr, perm, True, sched, wd)
            noise_p = np.maximum(noise_p, rel_each(s, s2).max(axis=0))
            noise = {"steps": max(noise["steps"], rel_spread(s, s2)),
                     "train_loss": max(noise["train_loss"], rel_spread(tl, tl2)),
                     "val_loss": max(noise["val_loss"], rel_spread(vl, vl2))}
            lr_equal = lr_equal and bool((lrs == lrs2).all())
        assert np.isfinite(s).all()
        moved = float(np.max(np.abs(s[-1] - params) / np.abs(np.where(params == 0, 1.0, params))))
        assert moved > 1e-6, (name, moved)
        for k, v in (("init", params), ("Fz", np.array(Fz if Fz else [0.0, 0.0])), ("steps", s), ("train_loss", tl),
                     ("val_loss", vl), ("lr", lrs)):
            npz[f"traj/{name}/{k}"] = v
        # parameters that are exactly 0 (a6) move from 0: relative spread against the step size there
        meta["trajectories"][name] = {
            "kind": kind, "optimizer": opt, "lr": lr, "epochs": int(perm.shape[0]),
            "perm": "perm2" if perm is perm2 else "perm8", "factor": sched[0] if sched else 0.5,
            "patience": sched[1] if sched else 2, "moved_rel": moved,
            "weight_decay": wd, "ref_noise_steps_params": [float(v) for v in noise_p],
            "ref_noise_steps": noise["steps"], "ref_noise_train_loss": noise["train_loss"],
            "ref_noise_val_loss": noise["val_loss"], "lr_equal_under_permutation": lr_equal}
    halvings = int(round(np.log2(sched_lr / npz["traj/lin_sched/lr"][-1])))
    assert halvings >= 2, npz["traj/lin_sched/lr"]
    meta["trajectories"]["lin_sched"]["halvings"] = halvings

    np.savez_compressed(os.path.join(HERE, "tyrefit_golden.npz"), **npz)
    with open(os.path.join(HERE, "tyrefit_golden.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print(json.dumps(meta, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
