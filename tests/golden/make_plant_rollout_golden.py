"""Generate tests/golden/plant_rollout_golden.npz / plant_rollout_golden.json: open-loop rollouts of the
reference's numpy plant models (models/KinematicBicycleModel.py, DynamicBicycleModel.py, BlendedBicycleModel.py)
along a logged drive for three parameter sets, and the same rollouts at 50 digits.

TEST FIXTURE GENERATOR (build container only, CPU only; no test imports it).

It imports the reference's ``models`` package (never copied) and iterates ``Model.step(throttle, steer, dt)``
with the set's values put on ``model.params`` of every model -- the blended model builds fresh sub-models in
every step, so the two classes it instantiates are wrapped by factories that set ``params`` on each new
sub-model -- and with the three constants of the penalty term (``stats.norm.pdf(throttle, loc=0.5,
scale=0.0775)`` in ``Model.Fx``) supplied by a stand-in for the ``stats`` name of ``models.Model`` that calls
scipy's ``norm.pdf`` with the set's location and width and multiplies by the set's amplitude.

Recorded:
* the log is NOT stored again: it is the [9][330] log of tests/golden/rollout_golden.npz (with its ``scale``);
* ``params`` [3][22]: the defaults; Cf = 80000, Cr = 50000, m = 1700; penalty amplitude 0 with Vblendmax = 25
  (the blend active over the whole log);
* per start pattern (``c70``: starts 0..69, H = 12; ``s3``: starts 3 j, j < 70, H = 12; ``h40``: the 8 starts of
  rollout_golden, H = 40) the rollouts in mpmath at 50 digits, ``mp`` [3 sets][3 models][H][6][n_start]
  (x_k = step(x_{k-1}, throttle[s+k-1], steer[s+k-1], ts[s+k]); models in the order kin, dyn, blend);
* ``ref_noise`` [3][3][H][6] per pattern: the largest |numpy - mpmath| over the starts divided by ``scale``.
  The tests' tolerance is 100 x that (floor 1e-13) on the scaled error against the mpmath values.

Asserted per set, model and pattern: every state (mpmath) stays at least 1e-9 (relative) away from every
branch point of the models -- the rpm steps 9000 / 9500 / 10400 / 12500, the 20 / 60 / 120 km/h gain steps, the
blend corners Vblendmin / Vblendmax, and the yaw wrap at +-pi -- so that a last-ulp difference cannot flip a
branch; no row of the log has throttle exactly 0 (the regenerative-brake branch is a test of its own).

Usage: python tests/golden/make_plant_rollout_golden.py <path to the reference checkout>
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ["m", "max_steer", "T_max", "r_wheel", "C_wheel", "R", "rho", "C_d", "A_f", "C_roll", "regen_brake_accel",
          "Iz", "lf", "lr", "Cf", "Cr", "g", "Vblendmin", "Vblendmax"]
MODELS = ["kin", "dyn", "blend"]
BRANCH_REL = 1e-9


def main():
    ref = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.environ.get("MR_REFERENCE_DIR", "")
    if not os.path.isdir(os.path.join(ref, "models")):
        raise SystemExit("usage: make_plant_rollout_golden.py <reference checkout>")
    sys.path.insert(0, ref)
    import mpmath as mp
    import scipy
    import scipy.stats
    import models.BlendedBicycleModel as bl
    import models.Model as model_mod
    from models.DynamicBicycleModel import DynamicBicycleModel
    from models.KinematicBicycleModel import KinematicBicycleModel
    from models.State import State
    from models.VehicleParameters import VehicleParameters as VP
    mp.mp.dps = 50

    G = np.load(os.path.join(HERE, "rollout_golden.npz"))
    log, scale = G["log"], G["scale"]
    T = log.shape[1]
    assert log.shape == (9, 330) and np.isfinite(log).all() and not (log[6] == 0.0).any()

    default = np.array([getattr(VP, k) for k in FIELDS] + [1.0, 0.5, 0.0775], dtype=np.float64)

    def with_(**kw):
        q = default.copy()
        for k, v in kw.items():
            q[(FIELDS + ["penalty_amp", "penalty_loc", "penalty_width"]).index(k)] = v
        return q

    sets = [default, with_(Cf=80000.0, Cr=50000.0, m=1700.0), with_(penalty_amp=0.0, Vblendmax=25.0)]
    names_sets = ["default", "Cf80000_Cr50000_m1700", "no_penalty_Vblendmax25"]

    # ---- the reference's models with a parameter set -------------------------------------------------
    current = {"q": default}

    class _Norm:
        @staticmethod
        def pdf(x, loc, scale):  # Model.Fx's call; the set's constants replace its literals
            q = current["q"]
            return q[19] * scipy.stats.norm.pdf(x, loc=q[20], scale=q[21])

    class _Stats:
        norm = _Norm

    model_mod.stats = _Stats

    def set_params(m):
        for j, k in enumerate(FIELDS):
            setattr(m.params, k, float(current["q"][j]))
        return m

    bl.KinematicBicycleModel = lambda initial_state: set_params(KinematicBicycleModel(initial_state))
    bl.DynamicBicycleModel = lambda initial_state: set_params(DynamicBicycleModel(initial_state))
    CLASSES = {"kin": KinematicBicycleModel, "dyn": DynamicBicycleModel, "blend": bl.BlendedBicycleModel}

    def rollout_numpy(model, q, starts, H):
        current["q"] = q
        out = np.empty((H, 6, len(starts)))
        for j, s in enumerate(starts):
            m = set_params(CLASSES[model](State(*[float(log[c, s]) for c in range(6)])))
            for k in range(1, H + 1):
                m.step(float(log[6, s + k - 1]), float(log[7, s + k - 1]), dt=float(log[8, s + k]))
                st = m.state
                out[k - 1, :, j] = [st.x, st.y, st.yaw, st.v_x, st.v_y, st.yaw_dot]
        return out

    # ---- the same at 50 digits -----------------------------------------------------------------------
    f = lambda v: mp.mpf(float(v))  # noqa: E731
    closest = {"v": mp.mpf(1)}

    def away(value, point):
        rel = abs(value - point) / abs(point)
        closest["v"] = min(closest["v"], rel)
        assert rel >= BRANCH_REL, (value, point)

    def fx_mp(q, thr, vx):
        regen = q[10] * f(9.81) * q[0] if thr == 0 else mp.mpf(0)
        rpm = (vx / q[4]) * 60 * q[5] * f(4.5)
        for step in (9000, 9500, 10400, 12500):
            away(rpm, step)
        eta = f(1.0) if rpm < 9000 else f(0.88) if rpm < 9500 else f(0.81) if rpm < 10400 else f(0.71) \
            if rpm < 12500 else f(0.675)
        z = (thr - q[20]) / q[21]
        penalty = q[19] * (mp.exp(-z * z / 2) / mp.sqrt(2 * mp.pi) / q[21]) * q[0]
        return thr * eta * q[2] * q[5] / q[3] - f(0.5) * q[6] * q[7] * q[8] * vx ** 2 - q[9] * q[0] * q[16] - regen \
            - penalty

    def delta_mp(q, steer, vx, vy):
        vel = mp.sqrt(vx ** 2 + vy ** 2) * f(3.6)
        for step in (20, 60, 120):
            away(vel, step)
        gain = f(1.0) if vel < 20 else f(0.9) if vel < 60 else f(0.8) if vel < 120 else f(0.7)
        return steer * q[1] * gain * (mp.pi / 180)

    def wrap(a):
        w = mp.atan2(mp.sin(a), mp.cos(a))
        away(abs(w), mp.pi)
        return w

    def kin_mp(q, x, thr, steer, dt):
        X, Y, yaw, vx, vy, r = x
        d = delta_mp(q, steer, vx, vy)
        Fx = fx_mp(q, thr, vx)
        rate = (vx / (q[13] + q[12])) * mp.tan(d)
        return [X + (vx * mp.cos(yaw) - vy * mp.sin(yaw)) * dt, Y + (vx * mp.sin(yaw) + vy * mp.cos(yaw)) * dt,
                wrap(yaw + rate * dt), vx + (Fx / q[0]) * dt, r * q[13], rate]

    def dyn_mp(q, x, thr, steer, dt):
        X, Y, yaw, vx, vy, r = x
        Fx = fx_mp(q, thr, vx)
        d = delta_mp(q, steer, vx, vy)
        thf, thr_ = mp.atan2(vy + q[12] * r, vx), mp.atan2(vy - q[13] * r, vx)
        Fyf, Fyr = q[14] * (d - thf), q[15] * (-thr_)
        vxd = (Fx - Fyf * mp.sin(d)) / q[0] + vy * r
        vyd = (Fyf * mp.cos(d) + Fyr) / q[0] - vx * r
        rd = (Fyf * mp.cos(d) * q[12] - Fyr * q[13]) / q[11]
        return [X + (vx * mp.cos(yaw) - vy * mp.sin(yaw)) * dt, Y + (vx * mp.sin(yaw) + vy * mp.cos(yaw)) * dt,
                wrap(yaw + r * dt), vx + vxd * dt, vy + vyd * dt, r + rd * dt]

    def blend_mp(q, x, thr, steer, dt):
        k, d = kin_mp(q, x, thr, steer, dt), dyn_mp(q, x, thr, steer, dt)
        vel = mp.sqrt(x[3] ** 2 + x[4] ** 2)
        away(vel, q[17])
        away(vel, q[18])
        lam = min(max((vel - q[17]) / (q[18] - q[17]), mp.mpf(0)), mp.mpf(1))
        return [lam * a + (1 - lam) * b for a, b in zip(d, k)]

    STEP_MP = {"kin": kin_mp, "dyn": dyn_mp, "blend": blend_mp}

    def rollout_mp(model, qf, starts, H):
        q = [f(v) for v in qf]
        out = np.empty((H, 6, len(starts)))
        for j, s in enumerate(starts):
            x = [f(log[c, s]) for c in range(6)]
            for k in range(1, H + 1):
                x = STEP_MP[model](q, x, f(log[6, s + k - 1]), f(log[7, s + k - 1]), f(log[8, s + k]))
                out[k - 1, :, j] = [float(v) for v in x]
        return out

    patterns = {"c70": (np.arange(70), 12), "s3": (3 * np.arange(70), 12), "h40": (G["h40/starts"], 40)}
    npz = {"params": np.stack(sets)}
    meta = {"T": T, "sets": names_sets, "models": MODELS, "fields": FIELDS + ["penalty_amp", "penalty_loc",
                                                                              "penalty_width"],
            "patterns": {}, "numpy": np.__version__, "scipy": scipy.__version__, "mpmath": mp.__version__,
            "digits": mp.mp.dps, "branch_rel": BRANCH_REL}
    for name, (starts, H) in patterns.items():
        starts = np.asarray(starts).astype(np.int32)
        assert starts.min() >= 0 and starts.max() <= T - 1 - H
        pn = np.stack([np.stack([rollout_numpy(m, q, starts, H) for m in MODELS]) for q in sets])
        pm = np.stack([np.stack([rollout_mp(m, q, starts, H) for m in MODELS]) for q in sets])
        assert np.isfinite(pn).all() and np.isfinite(pm).all()
        noise = np.abs(pn - pm).max(axis=4) / scale[None, None, None, :]
        npz[f"{name}/starts"], npz[f"{name}/mp"], npz[f"{name}/ref_noise"] = starts, pm, noise
        meta["patterns"][name] = {"H": int(H), "n_start": int(len(starts)),
                                  "ref_noise_max": [[float(v) for v in row] for row in noise.max(axis=(2, 3))]}
        print(name, meta["patterns"][name], "closest branch approach so far", float(closest["v"]), flush=True)
    meta["closest_branch_approach"] = float(closest["v"])
    np.savez_compressed(os.path.join(HERE, "plant_rollout_golden.npz"), **npz)
    with open(os.path.join(HERE, "plant_rollout_golden.json"), "w") as fjs:
        json.dump(meta, fjs, indent=1, sort_keys=True)
    print(json.dumps(meta, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
