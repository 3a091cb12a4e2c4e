"""Fit tyre models on the GPU: data -> ``fit_tyres`` -> ``BatchSolver(tyres=...)``.

Replaces the reference's torch training loop (learning/train.py:78-192 driving learning/vehicle.py:136-205)
with ``mr_tyre_fit`` (csrc/mr_tyrefit.h): one 64-lane wavefront per training run, a minibatch of 64 rows is
one row per lane, analytic gradients in the cancellation-free Pacejka form, all epochs in one launch.
Independent runs (seeds, initial guesses, learning rates) share a launch.

``host_twin=True`` runs the g++ build of the same source instead (TEST-ONLY, explicit; there is no
fallback: without it a missing GPU or library is an error).
"""
import ctypes
from collections import OrderedDict

import numpy as np

from . import abi

FEATURES = ["X_0", "Y_0", "yaw_0", "vx_0", "vy_0", "yawdot_0", "throttle_0", "steer_0", "last_ts"]
TARGETS = ["X_1", "Y_1", "yaw_1", "vx_1", "vy_1", "yawdot_1"]
N_PAR = {"linear": 2, "pacejka": 18}
# the reference's initial values (float32 tensors cast to float64, learning/vehicle.py:64,76-77)
PACEJKA_INIT = np.array([1.3, -22.1, 1011, 1078, 1.82, 0.208, 0.0, -0.354, 0.707], np.float32).astype(np.float64)
LINEAR_INIT = 65000.0
FZ_DEFAULT = float(np.float32(1845.0 * 9.81))
# torch.optim defaults: betas, eps; weight_decay 0 (SGD, Adam) / 1e-2 (AdamW)
_OPT_DEFAULTS = {"sgd": (0.9, 0.999, 1e-8, 0.0), "adam": (0.9, 0.999, 1e-8, 0.0), "adamw": (0.9, 0.999, 1e-8, 1e-2)}


def load_rows(csv):
    """Rows [n][15] of a reference dataset csv: FEATURES then TARGETS (learning/train.py:32-37)."""
    raw = np.genfromtxt(csv, delimiter=",", names=True)
    missing = [c for c in FEATURES + TARGETS if c not in raw.dtype.names]
    if missing:
        raise ValueError(f"{csv}: missing columns {missing}")
    rows = np.stack([np.atleast_1d(raw[c]) for c in FEATURES + TARGETS], axis=1).astype(np.float64)
    if not np.isfinite(rows).all():
        raise ValueError(f"{csv}: data has a nan")  # train.py:68-70
    return rows


def _rows(a, what):
    a = np.asarray(a, np.float64)
    if a.ndim != 2 or a.shape[1] != 15:
        raise ValueError(f"{what}: expected rows [n][15], got {a.shape}")
    return a


def make_config(kind="pacejka", optimizer="adam", epochs=25, factor=0.5, patience=2, host_twin=False, **vehicle):
    if kind not in abi.MR_TYRE:
        raise ValueError(f"unknown tyre kind {kind!r} (linear, pacejka; the reference's mlp tyres cannot feed the MPC)")
    if optimizer.lower() not in abi.MR_OPT:
        raise ValueError(f"unknown optimizer {optimizer!r} (sgd, adam, adamw)")
    c = abi.MRTyrefitConfig()
    if host_twin:
        abi.load_host_twin().mrh_tyrefit_config_default(ctypes.byref(c))
    else:
        abi.load_product().mr_tyrefit_config_default(ctypes.byref(c))
    c.kind, c.optimizer = abi.MR_TYRE[kind], abi.MR_OPT[optimizer.lower()]
    c.epochs, c.factor, c.patience = int(epochs), float(factor), int(patience)
    for k, v in vehicle.items():
        if k not in dict(abi.MRTyrefitConfig._fields_):
            raise ValueError(f"unknown vehicle constant {k!r}")
        setattr(c, k, float(v))
    return c


class _Device:
    """Moves numpy arrays to the GPU (torch tensors) and calls libmpcracing.so."""

    def __init__(self, device):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("mpcracing.tyrefit needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.torch = torch
        self.dev = torch.device("cuda", int(device))
        self.lib = abi.load_product()
        self.keep = []

    def put(self, a):
        t = self.torch.as_tensor(np.array(a, order="C")).to(self.dev)  # a writable contiguous copy
        self.keep.append(t)
        return t

    def empty(self, shape, dtype=np.float64):
        t = self.torch.empty(shape, dtype=self.torch.float64 if dtype == np.float64 else self.torch.int32,
                             device=self.dev)
        self.keep.append(t)
        return t

    @staticmethod
    def ptr(t):
        return ctypes.c_void_p(t.data_ptr())

    def get(self, t):
        return t.cpu().numpy()

    def stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    def check(self, rc):
        if rc != 0:
            raise RuntimeError(f"libmpcracing error {rc}: {self.lib.mr_last_error().decode()}")

    def call(self, name, *args, track=None, sync=True):
        """``mr_<name>(*args)`` on the current stream, its return code checked, then (``sync``) a synchronise of the
        device; ``track``: the DeviceTrack whose handle leads the arguments."""
        lead = [] if track is None else [track.h]
        self.check(getattr(self.lib, "mr_" + name)(*lead, *args, self.stream()))
        if sync:
            self.torch.cuda.synchronize(self.dev)


class _Host:
    """TEST-ONLY: numpy arrays and the host build of the same source."""

    def __init__(self):
        self.lib = abi.load_host_twin()

    def put(self, a):
        return np.ascontiguousarray(a)

    def empty(self, shape, dtype=np.float64):
        return np.full(shape, np.nan if dtype == np.float64 else -1, dtype)

    @staticmethod
    def ptr(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    def get(self, a):
        return a

    def check(self, rc):
        if rc != 0:
            raise RuntimeError(f"host twin error {rc}: {self.lib.mrh_tyrefit_last_error().decode()}")

    # the entries that spread their waves or vehicles over OpenMP threads: they take a thread count last
    THREADED = {"tyre_fit", "tyre_rollout", "plant_rollout", "pid_drive", "pid_segment_times"}

    def call(self, name, *args, track=None, sync=True):
        """``mrh_<name>(*args)`` (with 16 threads where the entry is ``THREADED``), its return code checked;
        ``track``: the host track whose blob arguments lead."""
        lead = [] if track is None else track.args()
        self.check(getattr(self.lib, "mrh_" + name)(*lead, *args, *([16] if name in self.THREADED else [])))


def loss_grad(rows, params, Fz=None, kind="pacejka", device=0, host_twin=False, **vehicle):
    """Loss (nn.MSELoss: mean over rows x 6) and its gradient for P parameter sets over rows [n][15].

    params [P][n_par] (or [n_par]); Fz [P][2] front / back loads (Pacejka).  Returns (loss [P], grad [P][n_par])."""
    rows = _rows(rows, "rows")
    cfg = make_config(kind, host_twin=host_twin, **vehicle)
    params = np.atleast_2d(np.asarray(params, np.float64))
    P, npar = params.shape
    if npar != N_PAR[kind]:
        raise ValueError(f"params: expected [P][{N_PAR[kind]}] for {kind}, got {params.shape}")
    Fz = np.broadcast_to(np.asarray(FZ_DEFAULT if Fz is None else Fz, np.float64), (P, 2))
    be = _Host() if host_twin else _Device(device)
    d_rows, d_par, d_Fz = be.put(rows.T), be.put(params), be.put(Fz)
    loss, grad = be.empty((P,)), be.empty((P, npar))
    n = rows.shape[0]
    be.call("tyre_loss_grad", ctypes.byref(cfg), n, be.ptr(d_rows), P, be.ptr(d_par), be.ptr(d_Fz), be.ptr(loss),
            be.ptr(grad), sync=False)  # the entry itself ends in a stream synchronise
    return be.get(loss), be.get(grad)


class FitResult:
    """Histories of every run and the best run (lowest validation loss among the runs that stayed finite)."""

    def __init__(self, kind, Fz, p_final, p_best, train_loss, val_loss, lr, flag, seeds):
        self.kind, self.Fz = kind, Fz
        self.p_final, self.p_best = p_final, p_best
        self.train_loss, self.val_loss, self.lr, self.flag, self.seeds = train_loss, val_loss, lr, flag, seeds
        score = np.where(np.isfinite(val_loss), val_loss, np.inf).min(axis=1)
        self.best_run = int(np.argmin(score))
        self.best_val_loss = float(score[self.best_run])
        self.ok = bool(np.isfinite(self.best_val_loss))  # False: no run finished an epoch with finite values
        self.runs = [dict(seed=seeds[r], flag=int(flag[r]), params=p_final[r], best_params=p_best[r],
                          train_loss=train_loss[r], val_loss=val_loss[r], lr=lr[r]) for r in range(len(flag))]

    @property
    def params(self):
        """Parameters of the best run at its best validation epoch."""
        if not self.ok:
            raise RuntimeError("no run finished an epoch: every run stopped on a non-finite value (see .flag, .runs)")
        return self.p_best[self.best_run]

    @property
    def tyres(self):
        """((a_front, Fz_front), (a_back, Fz_back)) for ``BatchSolver(tyres=...)`` / ``solver_for_config``."""
        if self.kind != "pacejka":
            raise ValueError("linear fits map to mr_config.Cf / Cr: use .linear")
        p, Fz = self.params, self.Fz[self.best_run]
        return ((p[:9].copy(), float(Fz[0])), (p[9:].copy(), float(Fz[1])))

    @property
    def linear(self):
        """{"Cf": ..., "Cr": ...}: ``BatchSolver(..., **result.linear)`` overrides mr_config.Cf / Cr."""
        if self.kind != "linear":
            raise ValueError("Pacejka fits feed BatchSolver(tyres=result.tyres)")
        return {"Cf": float(self.params[0]), "Cr": float(self.params[1])}

    def rank_by_rollout(self, log, horizon, **kw):
        """Run indices ordered by the position RMSE of their best parameters at step ``horizon`` of open-loop
        rollouts from every admissible row of ``log`` [9][T] (``mpcracing.rollout.load_log``), best first;
        runs without a finite value last.  The errors are kept as ``.rollout`` (a RolloutErrors)."""
        from .rollout import rollout_errors
        self.rollout = rollout_errors(log, self, horizon=horizon, **kw)
        rmse = self.rollout.position_rmse()
        return np.argsort(np.where(np.isfinite(rmse), rmse, np.inf), kind="stable")

    def state_dict(self):
        """The reference model's state dict (torch fp64 tensors; ``torch.save`` of it loads in its tooling)."""
        import torch
        p = self.params
        if self.kind == "linear":
            return OrderedDict([("front_tire.stiffness", torch.tensor([p[0]], dtype=torch.float64)),
                                ("back_tire.stiffness", torch.tensor([p[1]], dtype=torch.float64))])
        Fz = self.Fz[self.best_run]
        return OrderedDict([("front_tire.a", torch.tensor(p[:9], dtype=torch.float64)),
                            ("front_tire.Fz", torch.tensor([Fz[0]], dtype=torch.float64)),
                            ("back_tire.a", torch.tensor(p[9:], dtype=torch.float64)),
                            ("back_tire.Fz", torch.tensor([Fz[1]], dtype=torch.float64))])


def make_perm(seed, epochs, n_train):
    """Row order of every epoch: ``numpy.random.default_rng(seed).permutation`` per epoch, int32 [epochs][n]."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(n_train) for _ in range(epochs)]).astype(np.int32)


def fit_tyres(train, val, kind="pacejka", inits=None, Fz=None, runs=1, seeds=None, optimizer="adam", lr=1e-3,
              epochs=25, factor=0.5, patience=2, betas=None, eps=None, weight_decay=None, perm=None, device=0,
              host_twin=False, record_steps=False, **vehicle):
    """Train ``runs`` independent tyre fits on rows ``train`` [n][15], validated each epoch on ``val``.

    inits [runs][n_par] (default: the reference's initial values); Fz [runs][2]; lr, betas, eps, weight_decay:
    scalars or per-run sequences (torch's defaults); seeds: per-run shuffle seeds (default 1337 + run, the
    shuffles built by ``make_perm``), or ``perm`` int32 [epochs][n] (shared) / [runs][epochs][n] to reproduce
    another loader's order.  record_steps keeps the parameters after every optimiser step (``.steps``
    [runs][epochs * ceil(n / 64)][n_par]).  Returns a FitResult."""
    train, val = _rows(train, "train"), _rows(val, "val")
    cfg = make_config(kind, optimizer, epochs, factor, patience, host_twin=host_twin, **vehicle)
    R, npar, n = int(runs), N_PAR[kind], train.shape[0]
    if R < 1:
        raise ValueError("runs < 1")
    if inits is None:
        inits = np.concatenate([PACEJKA_INIT, PACEJKA_INIT]) if kind == "pacejka" else np.full(2, LINEAR_INIT)
    inits = np.array(np.broadcast_to(np.asarray(inits, np.float64), (R, npar)))
    Fz = np.array(np.broadcast_to(np.asarray(FZ_DEFAULT if Fz is None else Fz, np.float64), (R, 2)))
    b1, b2, e0, wd0 = _OPT_DEFAULTS[optimizer.lower()]
    betas = (b1, b2) if betas is None else betas
    hyper = np.empty((R, 5))
    hyper[:, 0] = lr
    hyper[:, 1] = np.asarray(betas, np.float64).T[0] if np.ndim(betas) == 2 else betas[0]
    hyper[:, 2] = np.asarray(betas, np.float64).T[1] if np.ndim(betas) == 2 else betas[1]
    hyper[:, 3] = e0 if eps is None else eps
    hyper[:, 4] = wd0 if weight_decay is None else weight_decay
    seeds = [1337 + r for r in range(R)] if seeds is None else list(seeds)
    if perm is None:
        if len(seeds) != R:
            raise ValueError("seeds: one per run")
        perm = np.stack([make_perm(s, int(epochs), n) for s in seeds])
    perm = np.ascontiguousarray(perm, np.int32)
    if perm.shape == (int(epochs), n):
        stride = 0
    elif perm.shape == (R, int(epochs), n):
        stride = int(epochs) * n
    else:
        raise ValueError(f"perm: expected [{epochs}][{n}] or [{R}][{epochs}][{n}], got {perm.shape}")
    be = _Host() if host_twin else _Device(device)
    d = [be.put(train.T), be.put(val.T), be.put(inits), be.put(Fz), be.put(hyper), be.put(perm)]
    out = [be.empty((R, npar)), be.empty((R, npar)), be.empty((R, int(epochs))), be.empty((R, int(epochs))),
           be.empty((R, int(epochs))), be.empty((R,), np.int32)]
    steps = be.empty((R, int(epochs) * ((n + 63) // 64), npar)) if record_steps else None
    args = [ctypes.byref(cfg), n, be.ptr(d[0]), val.shape[0], be.ptr(d[1]), R, be.ptr(d[2]), be.ptr(d[3]),
            be.ptr(d[4]), be.ptr(d[5]), stride] + [be.ptr(o) for o in out] + [be.ptr(steps) if record_steps else None]
    be.call("tyre_fit", *args)
    p_final, p_best, tl, vl, lrh, flag = [be.get(o) for o in out]
    res = FitResult(kind, Fz, p_final, p_best, tl, vl, lrh, flag, seeds)
    res.steps = be.get(steps) if record_steps else None
    return res
