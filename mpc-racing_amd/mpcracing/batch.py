"""Batched solve on the GPU through libmpcracing.so (PyTorch tensors for device storage only).

``BatchSolver`` is the batch API behind the drop-in ``control.MPC.MPC``: it
owns a solver handle (workspace sized for ``max_batch``) and solves B
independent instances per call.  Inputs/outputs follow the structure-of-arrays
layout of include/mpcracing.h.  There is no CPU fallback: without a GPU or
without the built library the constructor raises.
"""
import ctypes

import numpy as np
import torch

from . import abi

_IN_KEYS = ("state0", "s0", "cx", "cy", "max_error", "runtime", "u_init")
_WARM_KEYS = ("x_init", "s_init")  # the primal guess (include/mpcracing.h mr_warm)


class BatchSolver:
    def __init__(self, N, model="dyn", precision="fp64", lane=False, Ts=0.05, max_batch=1, device=0, tol=None,
                 tyres=None, **overrides):
        if not torch.cuda.is_available():
            raise RuntimeError("mpcracing.BatchSolver needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.lib = abi.load_product()
        c = abi.MRConfig()
        self.lib.mr_config_default(ctypes.byref(c))
        c.N = int(N)
        c.model = abi.MR_MODEL[model]
        c.precision = abi.MR_PREC[precision]
        c.lane_bounds = int(bool(lane))
        c.Ts = float(Ts)
        c.max_batch = int(max_batch)
        c.device = int(device)
        if tol is not None:
            c.tol = float(tol)
        elif precision == "fp32":
            # the reference's own IPOPT options (control/MPC.py:152-161): tol 1e-4, acceptable_tol 1e-2,
            # IPOPT's acceptable_iter 15 (the fp32 solve resolves the KKT error to 1e-4 through its fp64
            # multipliers, mr_wave.h eval_sweep; the acceptable exit catches the rare stalls)
            c.tol = 1e-4
            c.acceptable_tol = 1e-2
        for k, v in overrides.items():
            setattr(c, k, v)
        self.cfg = c
        self.device = torch.device("cuda", int(device))
        self.N = int(N)
        h = ctypes.c_void_p()
        self._check(self.lib.mr_create(ctypes.byref(h), ctypes.byref(c)))
        self.h = h
        if tyres is not None:
            (af, Fzf), (ar, Fzr) = tyres
            af = np.asarray(af, np.float64)
            ar = np.asarray(ar, np.float64)
            self._check(self.lib.mr_set_tyres(h, af.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), float(Fzf),
                                              ar.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), float(Fzr)))

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(f"libmpcracing error {rc}: {self.lib.mr_last_error().decode()}")

    def __del__(self):
        h = getattr(self, "h", None)
        if h is not None and h.value:
            self.lib.mr_destroy(h)
            self.h = None

    def to_device(self, batch):
        out = {}
        h = batch.get("order_hint")
        if h is not None:  # int32 [B] (dispatch_order 2), e.g. a previous solve's iters
            out["order_hint"] = (h if isinstance(h, torch.Tensor) else torch.from_numpy(np.asarray(h))).to(
                self.device, torch.int32).contiguous()
        n = batch.get("horizon")
        if n is not None:  # int32 [B]: one horizon per instance (mr_solve_batch_horizons)
            out["horizon"] = (n if isinstance(n, torch.Tensor) else torch.from_numpy(np.asarray(n))).to(
                self.device, torch.int32).contiguous()
        u = batch.get("warm_use")
        if u is not None:  # int32 [B]: 0 = this instance starts cold (mr_warm.use)
            out["warm_use"] = (u if isinstance(u, torch.Tensor) else torch.from_numpy(np.asarray(u))).to(
                self.device, torch.int32).contiguous()
        for k in _IN_KEYS + _WARM_KEYS:
            v = batch.get(k)
            if v is None:
                if k in _IN_KEYS:
                    out[k] = None
            elif isinstance(v, torch.Tensor):
                out[k] = v.to(self.device, torch.float64).contiguous()
            else:
                out[k] = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(self.device)
        return out

    def alloc_outputs(self, B, duals=False):
        """Output tensors; ``duals`` adds ``lam_g`` [13N+9][B] (the reference's opti.lam_g, Opti row order)."""
        N, d = self.N, self.device
        f = dict(dtype=torch.float64, device=d)
        out = {"X": torch.empty((6, N + 1, B), **f), "U": torch.empty((2, N, B), **f),
               "S": torch.empty((N + 1, B), **f), "eC": torch.empty((N, B), **f), "eL": torch.empty((N, B), **f),
               "status": torch.empty(B, dtype=torch.int32, device=d),
               "iters": torch.empty(B, dtype=torch.int32, device=d),
               "obj": torch.empty(B, **f), "kkt": torch.empty(B, **f), "constr_viol": torch.empty(B, **f)}
        if duals:
            out["lam_g"] = torch.empty((13 * N + 9, B), **f)
        return out

    def launch(self, dev_in, out, stream=None, trace_instance=-1):
        """Enqueue one batched solve on ``stream`` (default: torch's current stream); no sync.

        ``dev_in["horizon"]`` (int32 [B] on the device, optional) gives instance i the horizon N_i in 1 .. N: it
        is solved as a ``BatchSolver(N_i)`` would solve it, inside arrays that keep the strides of N
        (include/mpcracing.h mr_solve_batch_horizons); rows beyond N_i come back NaN.

        ``dev_in["x_init"]`` [6][N+1][B] and ``dev_in["s_init"]`` [N+1][B] (both or neither) are a primal guess of
        States and S_hat: the solve starts from it instead of the rollout of the controls (mr_solve_batch_warm).
        ``dev_in["warm_use"]`` (int32 [B], optional) switches the guess off per instance; ``out["warm_used"]``
        (int32 [B], optional) receives which instances took it (a non-finite guess is not taken)."""
        B = int(dev_in["s0"].shape[0])
        N = self.N
        shapes = {"state0": (8, B), "s0": (B,), "cx": (5, B), "cy": (5, B), "max_error": (B,), "runtime": (5, B),
                  "u_init": (2, N, B), "x_init": (6, N + 1, B), "s_init": (N + 1, B)}
        for k, shp in shapes.items():
            v = dev_in.get(k)
            if v is None:
                continue
            if tuple(v.shape) != shp or v.dtype != torch.float64 or not v.is_contiguous() or v.device != self.device:
                raise ValueError(f"input {k}: expected contiguous float64 {shp} on {self.device}, got "
                                 f"{tuple(v.shape)} {v.dtype} {v.device}")
        h = dev_in.get("order_hint")
        if h is not None and (tuple(h.shape) != (B,) or h.dtype != torch.int32 or not h.is_contiguous()
                              or h.device != self.device):
            raise ValueError(f"input order_hint: expected contiguous int32 ({B},) on {self.device}")
        n = dev_in.get("horizon")
        if n is not None and (tuple(n.shape) != (B,) or n.dtype != torch.int32 or not n.is_contiguous()
                              or n.device != self.device):
            raise ValueError(f"input horizon: expected contiguous int32 ({B},) on {self.device}")
        xi, si = dev_in.get("x_init"), dev_in.get("s_init")
        if (xi is None) != (si is None):
            raise ValueError("inputs x_init and s_init go together")
        for k, v in (("warm_use", dev_in.get("warm_use")), ("warm_used", out.get("warm_used"))):
            if v is not None and (tuple(v.shape) != (B,) or v.dtype != torch.int32 or not v.is_contiguous()
                                  or v.device != self.device):
                raise ValueError(f"{k}: expected contiguous int32 ({B},) on {self.device}")
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        inp = abi.MRInputs(*[ptr(dev_in.get(k)) for k in _IN_KEYS + ("order_hint",)])
        tr = out.get("trace")
        o = abi.MROutputs(*[ptr(out.get(k)) for k in ("X", "U", "S", "eC", "eL", "status", "iters", "obj", "kkt",
                                                      "trace")], int(trace_instance),
                          int(tr.shape[0]) if tr is not None else 0, ptr(out.get("lam_g")),
                          ptr(out.get("timeline")), ptr(out.get("constr_viol")))
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        if xi is not None:
            wm = abi.MRWarm(ptr(xi), ptr(si), ptr(dev_in.get("warm_use")), ptr(out.get("warm_used")))
            self._check(self.lib.mr_solve_batch_warm(self.h, B, ctypes.byref(inp), ctypes.byref(o), ptr(n),
                                                     ctypes.byref(wm), ctypes.c_void_p(st.cuda_stream)))
        elif n is None:
            self._check(self.lib.mr_solve_batch(self.h, B, ctypes.byref(inp), ctypes.byref(o),
                                                ctypes.c_void_p(st.cuda_stream)))
        else:
            self._check(self.lib.mr_solve_batch_horizons(self.h, B, ctypes.byref(inp), ctypes.byref(o), ptr(n),
                                                         ctypes.c_void_p(st.cuda_stream)))
        return out

    def alloc_warm(self, B):
        """Buffers of ``warm_shift``: u_init, x_init, s_init and warm_use of a batch of B."""
        N, f = self.N, dict(dtype=torch.float64, device=self.device)
        return {"u_init": torch.empty((2, N, B), **f), "x_init": torch.empty((6, N + 1, B), **f),
                "s_init": torch.empty((N + 1, B), **f),
                "warm_use": torch.empty(B, dtype=torch.int32, device=self.device)}

    def warm_shift(self, prev, state0, s0, horizon_prev=None, horizon_new=None, out=None, stream=None):
        """The next tick's guess from the previous tick's solution ``prev`` (its X, U, S, status; device tensors
        of this solver's layout), the new measured ``state0`` [8][B] (rows 0..5 read) and progress ``s0`` [B]:
        shifted controls, shifted States / S_hat with the tail extrapolated by the MPC model, and the per-instance
        use flag (include/mpcracing.h mr_warm_shift).  Enqueued on ``stream``, no sync; returns ``out``
        (``alloc_warm``), whose entries are ``launch`` inputs.  ``out`` must not alias ``prev``."""
        B = int(s0.shape[0])
        out = out if out is not None else self.alloc_warm(B)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        for t, shp, dt in ((prev["X"], (6, self.N + 1, B), torch.float64), (prev["U"], (2, self.N, B), torch.float64),
                           (prev["S"], (self.N + 1, B), torch.float64), (prev["status"], (B,), torch.int32),
                           (state0, (8, B), torch.float64), (s0, (B,), torch.float64),
                           (horizon_prev, (B,), torch.int32), (horizon_new, (B,), torch.int32)):
            if t is not None and (tuple(t.shape) != shp or t.dtype != dt or not t.is_contiguous()
                                  or t.device != self.device):
                raise ValueError(f"warm_shift: expected contiguous {dt} {shp} on {self.device}, got "
                                 f"{tuple(t.shape)} {t.dtype} {t.device}")
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        self._check(self.lib.mr_warm_shift(self.h, B, ptr(prev["X"]), ptr(prev["U"]), ptr(prev["S"]),
                                           ptr(prev["status"]), ptr(horizon_prev), ptr(state0), ptr(s0),
                                           ptr(horizon_new), ptr(out["u_init"]), ptr(out["x_init"]),
                                           ptr(out["s_init"]), ptr(out["warm_use"]),
                                           ctypes.c_void_p(st.cuda_stream)))
        return out

    def solve(self, batch, stream=None, trace_instance=-1, trace_cap=0, duals=False):
        """Blocking solve of a host or device batch; returns device output tensors."""
        dev_in = self.to_device(batch)
        out = self.alloc_outputs(int(dev_in["s0"].shape[0]), duals=duals)
        if trace_cap:
            out["trace"] = torch.zeros((trace_cap, 8), dtype=torch.float64, device=self.device)
        if dev_in.get("x_init") is not None:
            out["warm_used"] = torch.zeros(out["status"].shape, dtype=torch.int32, device=self.device)
        self.launch(dev_in, out, stream, trace_instance)
        torch.cuda.synchronize(self.device)
        return out


def solver_for_config(name, max_batch, device=0, **kw):
    """BatchSolver configured as BASELINE config ``name`` (C1..C5); ``tyres=`` replaces the config's
    learned tyre coefficients (e.g. ``mpcracing.tyrefit.fit_tyres(...).tyres``)."""
    from .workload import CONFIGS, tyre_coeffs
    c = CONFIGS[name]
    tyres = kw.pop("tyres", None)
    if tyres is None:
        tyres = tyre_coeffs(c["tyres"]) if c["tyres"] else None
    precision = kw.pop("precision", c["precision"])
    return BatchSolver(c["N"], c["model"], precision, c["lane"], c["Ts"], max_batch=max_batch,
                       device=device, tyres=tyres, **kw)
