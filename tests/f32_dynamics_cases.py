"""Evaluation points and error measures of the fp32 dynamics tests (TEST-ONLY), shared by
tests/test_f32_dynamics.py (CPU) and tests/test_gpu_f32_dynamics.py."""
import numpy as np

import host_twin as ht
from mpcracing import workload as wl

MODELS = ["kin", "dyn", "blend", "blend_pacejka", "dyn_pacejka"]
N = 1024
VMIN, VMAX = 2.0, 15.0  # Vblendmin / Vblendmax of the default configuration (csrc/mr_batch.h)
MARGIN = 1e-3
EPS32 = float(np.finfo(np.float32).eps)
# learning/vehicle.py's initial coefficients at a small load: |B alpha| ~ 1, the non-series branch of pacejka_jet
DEFAULT_FZ1 = ([1.3, -22.1, 1011, 1078, 1.82, 0.208, 0.0, -0.354, 0.707], 1.0)

# (case id, model, tyres name, point set)
CASES = [(m, m, "pacejka-2" if "pacejka" in m else None, "range") for m in MODELS] + \
        [("dyn_pacejka-learned-small_slip", "dyn_pacejka", "pacejka-2", "small_slip"),
         ("dyn_pacejka-default_Fz1-small_slip", "dyn_pacejka", "vehicle_default_Fz1", "small_slip"),
         ("dyn_pacejka-default_Fz1", "dyn_pacejka", "vehicle_default_Fz1", "range")]


def tyres(name):
    if name is None:
        return None
    if name == "vehicle_default_Fz1":
        return (DEFAULT_FZ1, DEFAULT_FZ1)
    return wl.tyre_coeffs(name)


def config(model):
    return ht.config(20, model, "fp32")


def speed64(x):
    return np.hypot(x[:, 3].astype(np.float64), x[:, 4].astype(np.float64))


def points(kind="range", n=N, seed=5):
    """float32 (x [n][6], u [n][2], nu [n][6]) in solver coordinates.
    range: |X|, |Y| <= 60 m, yaw in [-pi, pi], a third of the speeds in each blend region (at least 1e-2 m/s off the
    thresholds), vy ~ N(0, 1) limited to half the speed, yaw rate ~ N(0, 0.5), controls inside their boxes, nu ~
    N(0, 10); the first points are zero slip (steer = throttle = vy = r = 0), one per region.
    small_slip: straight driving with vy = (vx + 0.1) tan(alpha), alpha log-uniform in [1e-6, 0.3] with both signs."""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 6))
    x[:, 0], x[:, 1] = rng.uniform(-60, 60, n), rng.uniform(-60, 60, n)
    x[:, 2] = rng.uniform(-np.pi, np.pi, n)
    u = np.stack([rng.uniform(-1.0, 0.85, n), rng.uniform(-0.9, 0.9, n)], 1)
    nu = rng.normal(0, 10, (n, 6))
    if kind == "range":
        region = np.arange(n) % 3
        lo = np.array([0.6, VMIN + 1e-2, VMAX + 1e-2])[region]
        hi = np.array([VMIN - 1e-2, VMAX - 1e-2, 45.0])[region]
        s = rng.uniform(lo, hi)
        vy = np.clip(rng.normal(0, 1, n), -0.5 * s, 0.5 * s)
        x[:, 3], x[:, 4] = np.sqrt(s * s - vy * vy), vy
        x[:, 5] = rng.normal(0, 0.5, n)
        x[:3, 4:6] = 0.0
        x[:3, 3] = [1.0, 8.0, 30.0]
        u[:3] = 0.0
    else:
        x[:, 3] = rng.uniform(0.5, 45, n)
        alpha = np.exp(rng.uniform(np.log(1e-6), np.log(0.3), n)) * np.where(rng.random(n) < 0.5, -1, 1)
        x[:, 4] = (x[:, 3] + 0.1) * np.tan(alpha)
        u[:, 1] = 0.0
    return x.astype(np.float32), u.astype(np.float32), nu.astype(np.float32)


def threshold_points():
    """vy = 0 and vx exactly at Vblendmin / Vblendmax: the law is continuous there, its derivatives are not."""
    x, u, nu = points("range", 64, seed=6)
    x[:, 4] = 0.0
    x[:, 3] = np.where(np.arange(64) % 2 == 0, VMIN, VMAX)
    return x, u, nu


def column_errors(out, ref):
    """Per output index: max over the batch of |out - ref| over max over the batch of |ref| (0 where the reference
    column is structurally zero), and the column scales."""
    scale = np.abs(ref).max(0)
    err = np.abs(out.astype(np.float64) - ref).max(0)
    return np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), 0.0), scale
