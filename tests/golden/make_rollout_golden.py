"""Generate tests/golden/rollout_golden.npz / rollout_golden.json: open-loop rollouts of the reference's torch
vehicle model along a logged drive, and the same rollouts at 50 digits.

TEST FIXTURE GENERATOR (build container only, CPU only; no test imports it).

It imports the reference's ``learning.vehicle`` (never copied) with tests/golden/casadi_standin.py registered
as ``casadi``, and composes the model as make_tyrefit_golden.py does: ``Vehicle('linear')`` in torch fp64,
its tyres replaced by ``Pacejka()`` for the Pacejka sets.

Recorded:
* the log [9][330]: rows 100..429 of the reference's ``data/t4/steps.csv`` (X, Y, yaw, vx, vy, yawdot,
  cmd_throttle - cmd_brake, cmd_steer, last_ts): no NaN, no yaw wrap, 59 braking rows;
* three parameter sets: linear 65000 / 65000, Pacejka defaults at the reference's load, and the learned
  ``pacejka-1`` coefficients;
* per start pattern (``c70``: starts 0..69, H = 12; ``s3``: starts 3 j, j < 70, H = 12; ``h40``: 8 starts,
  H = 40; ``h1``: every admissible row, H = 1) the predictions of the torch model iterated
  (x_k = f(x_{k-1}, throttle[s+k-1], steer[s+k-1], ts[s+k])) and the same in mpmath at 50 digits, both
  [3][H][6][n_start];
* ``ref_noise`` [3][H][6] per pattern: the largest |torch - mpmath| over the starts divided by ``scale``
  [6], the largest |value| of the component in the log.  The tests' tolerance is 100 x that (floor 1e-13) on
  the scaled error against the mpmath values.

Usage: python tests/golden/make_rollout_golden.py <path to the reference checkout>
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROW0, T = 100, 330
COLS = ["X", "Y", "yaw", "vx", "vy", "yawdot"]


def main():
    ref = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.environ.get("MR_REFERENCE_DIR", "")
    if not os.path.isdir(os.path.join(ref, "learning")):
        raise SystemExit("usage: make_rollout_golden.py <reference checkout>")
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
    mp.mp.dps = 50

    with open(os.path.join(ref, "data", "t4", "steps.csv")) as f:
        names = f.readline().strip().split(",")
        lines = [ln.strip().split(",") for ln in f if ln.strip()][ROW0:ROW0 + T]
    col = lambda c: np.array([float("nan") if r[names.index(c)] == "None" else float(r[names.index(c)])  # noqa: E731
                              for r in lines])
    log = np.stack([col(c) for c in COLS] + [col("cmd_throttle") - col("cmd_brake"), col("cmd_steer"), col("last_ts")])
    assert log.shape == (9, T) and np.isfinite(log).all()
    assert np.abs(np.diff(log[2])).max() < 1.0  # no yaw wrap
    scale = np.abs(log[:6]).max(axis=1)

    FZ = float(np.float32(VP.m * 9.81))
    A_DEFAULT = Pacejka().a.detach().numpy().astype(np.float64)
    pac1 = torch.load(os.path.join(ref, "learning", "models", "pacejka-1", "model"), map_location="cpu")
    sets = [
        ("linear", np.array([65000.0, 65000.0]), np.array([0.0, 0.0])),
        ("pacejka", np.concatenate([A_DEFAULT, A_DEFAULT]), np.array([FZ, FZ])),
        ("pacejka", np.concatenate([pac1["front_tire.a"].double().numpy(), pac1["back_tire.a"].double().numpy()]),
         np.array([float(pac1["front_tire.Fz"]), float(pac1["back_tire.Fz"])])),
    ]
    names_sets = ["linear_65000", "pacejka_default", "pacejka_1"]

    def model(kind, params, Fz):
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

    def rollout_torch(v, starts, H):
        x = torch.tensor(log[:6, starts].T.copy())
        out = np.empty((H, 6, len(starts)))
        with torch.no_grad():
            for k in range(1, H + 1):
                u = torch.tensor(np.stack([log[6, starts + k - 1], log[7, starts + k - 1], log[8, starts + k]], axis=1))
                x = v(torch.cat([x, u], dim=1))
                out[k - 1] = x.numpy().T
        return out

    f = lambda v: mp.mpf(float(v))  # noqa: E731

    def fy_mp(kind, a, Fz, al):
        if kind == "linear":
            return a * al
        C = a[0]
        D = (a[1] * Fz + a[2]) * Fz
        BCD = a[3] * mp.sin(a[4] * mp.atan(a[5] * Fz))
        B = BCD / (C * D)
        E = a[6] * Fz ** 2 + a[7] * Fz + a[8]
        if al == 0:
            return mp.mpf(0)
        phi = (1 - E) * al + (E / B) * mp.atan(B * al)
        return D * mp.sin(C * mp.atan(B * phi))

    def forward_mp(kind, x, thr, steer, dt, tf_, tr_):
        m_, Iz, lf, lr = f(VP.m), f(VP.Iz), f(VP.lf), f(VP.lr)
        X, Y, yaw, vx, vy, r = x
        rpm = (vx / f(VP.C_wheel)) * 60 * f(VP.R) * f(4.5)
        eta = f(-0.00004428225806) * rpm + f(1.282413306)
        Fx = thr * eta * f(VP.T_max) * f(VP.R) / f(VP.r_wheel) - f(0.5) * f(VP.rho) * f(VP.C_d) * f(VP.A_f) * vx ** 2 \
            - f(VP.C_roll) * f(VP.m) * f(VP.g)
        vel = mp.sqrt(vx ** 2 + vy ** 2) * f(3.6)
        gain = f(-0.001971664699) * vel + f(0.986547)
        delta = (steer * gain * f(VP.max_steer) / 360) * 2 * f(3.14)
        thf = mp.atan2(vy + lf * r, vx + f(0.1))
        thr_ = mp.atan2(vy - lr * r, vx + f(0.1))
        Fyf, Fyr = fy_mp(kind, tf_[0], tf_[1], delta - thf), fy_mp(kind, tr_[0], tr_[1], -thr_)
        vxd = (Fx - Fyf * mp.sin(delta)) / m_ + vy * r
        vyd = (Fyf * mp.cos(delta) + Fyr) / m_ - vx * r
        rd = (Fyf * mp.cos(delta) * lf - Fyr * lr) / Iz
        return [X + (vx * mp.cos(yaw) - vy * mp.sin(yaw)) * dt, Y + (vx * mp.sin(yaw) + vy * mp.cos(yaw)) * dt,
                yaw + r * dt, vx + vxd * dt, vy + vyd * dt, r + rd * dt]

    def rollout_mp(kind, params, Fz, starts, H):
        if kind == "linear":
            tf_, tr_ = (f(params[0]), None), (f(params[1]), None)
        else:
            tf_ = ([f(v) for v in params[:9]], f(Fz[0]))
            tr_ = ([f(v) for v in params[9:]], f(Fz[1]))
        out = np.empty((H, 6, len(starts)))
        for j, s in enumerate(starts):
            x = [f(log[c, s]) for c in range(6)]
            for k in range(1, H + 1):
                x = forward_mp(kind, x, f(log[6, s + k - 1]), f(log[7, s + k - 1]), f(log[8, s + k]), tf_, tr_)
                out[k - 1, :, j] = [float(v) for v in x]
        return out

    patterns = {
        "c70": (np.arange(70), 12),
        "s3": (3 * np.arange(70), 12),
        "h40": (np.array([0, 37, 64, 111, 150, 200, 257, T - 1 - 40]), 40),
        "h1": (np.arange(T - 1), 1),
    }
    npz = {"log": log, "scale": scale}
    meta = {"T": T, "row0": ROW0, "sets": names_sets, "kinds": [s[0] for s in sets], "patterns": {},
            "torch": torch.__version__, "mpmath": mp.__version__, "digits": mp.mp.dps}
    for i, (kind, params, Fz) in enumerate(sets):
        npz[f"set{i}/params"], npz[f"set{i}/Fz"] = params, Fz
    for name, (starts, H) in patterns.items():
        starts = starts.astype(np.int32)
        assert starts.min() >= 0 and starts.max() <= T - 1 - H
        pt = np.stack([rollout_torch(model(*s), starts, H) for s in sets])
        pm = np.stack([rollout_mp(*s, starts, H) for s in sets])
        assert np.isfinite(pt).all() and np.isfinite(pm).all()
        noise = np.abs(pt - pm).max(axis=3) / scale[None, None, :]
        npz[f"{name}/starts"], npz[f"{name}/torch"], npz[f"{name}/mp"], npz[f"{name}/ref_noise"] = starts, pt, pm, noise
        meta["patterns"][name] = {"H": int(H), "n_start": int(len(starts)),
                                  "ref_noise_max_per_set": [float(v) for v in noise.max(axis=(1, 2))]}
        print(name, meta["patterns"][name], flush=True)
    np.savez_compressed(os.path.join(HERE, "rollout_golden.npz"), **npz)
    with open(os.path.join(HERE, "rollout_golden.json"), "w") as fjs:
        json.dump(meta, fjs, indent=1, sort_keys=True)
    print(json.dumps(meta, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
