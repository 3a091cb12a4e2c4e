"""Callers of the fp32 probes: libmpcracing_probe.so on the GPU and the libm float build of the host twin
(TEST-ONLY), with the error measures the fp32 accuracy tests share."""
import ctypes
import json
import os

import numpy as np

import host_twin as ht
from mpcracing import abi

EPS32 = float(np.finfo(np.float32).eps)
_PD = ctypes.POINTER(ctypes.c_double)


def record(name, figures):
    """Print the measured figures, and keep them as <MR_F32_ACCURACY_OUT>/<name>.json where that is set (the source
    of profiles/f32_accuracy.json)."""
    print(name, json.dumps(figures))
    out = os.environ.get("MR_F32_ACCURACY_OUT")
    if out:
        with open(os.path.join(out, name + ".json"), "w") as f:
            json.dump(figures, f, indent=1)


def ulp_err(out, ref):
    """|out - ref| in units of the fp32 spacing at ref (ref fp64, finite and non-zero where compared)."""
    sp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return np.abs(out.astype(np.float64) - ref) / sp


def abs_err_eps(out, ref):
    """|out - ref| / max(|ref|, 1) in units of eps32."""
    return np.abs(out.astype(np.float64) - ref) / np.maximum(np.abs(ref), 1.0) / EPS32


def _tyre_args(tyres):
    if tyres is None:
        return None, 0.0, None, 0.0, ()
    (af, Fzf), (ar, Fzr) = tyres
    af, ar = np.asarray(af, np.float64), np.asarray(ar, np.float64)
    return af.ctypes.data_as(_PD), float(Fzf), ar.ctypes.data_as(_PD), float(Fzr), (af, ar)


def _v(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


# ---- device ----
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(lib, rc):
    assert rc == 0, lib.mrp_last_error().decode()


def dev_math(op, a, b=None):
    import torch
    lib = abi.load_probe()
    a = np.ascontiguousarray(a, np.float32)
    A = _dev(a)
    B = _dev(np.ascontiguousarray(b, np.float32)) if b is not None else None
    out = torch.zeros(a.size, dtype=torch.float32, device="cuda")
    _ok(lib, lib.mrp_math_f32(abi.MRP_OP[op], a.size, _ptr(A), _ptr(B), _ptr(out), _stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def dev_dynamics(cfg, tyres, x, u, nu, jac=True):
    """Dyn<float, MODEL> on the device: (f, J, H) as float32 [n][6 | 48 | 36]; jac=False: value only, (f, None, None)."""
    import torch
    lib = abi.load_probe()
    n = x.shape[0]
    X, U, NU = (_dev(np.ascontiguousarray(t, np.float32)) for t in (x, u, nu))
    f = torch.zeros((n, 6), dtype=torch.float32, device="cuda")
    J = torch.zeros((n, 48), dtype=torch.float32, device="cuda") if jac else None
    H = torch.zeros((n, 36), dtype=torch.float32, device="cuda") if jac else None
    pa, Fa, pb, Fb, keep = _tyre_args(tyres)
    _ok(lib, lib.mrp_eval_dynamics_f32(ctypes.byref(cfg), pa, Fa, pb, Fb, n, _ptr(X), _ptr(U), _ptr(NU), _ptr(f),
                                       _ptr(J), _ptr(H), _stream()))
    torch.cuda.synchronize()
    del keep
    return tuple(t.cpu().numpy() if t is not None else None for t in (f, J, H))


def dev_chol3(R, b):
    import torch
    lib = abi.load_probe()
    n = R.shape[0]
    Rd, bd = _dev(np.ascontiguousarray(R, np.float32)), _dev(np.ascontiguousarray(b, np.float32))
    ok = torch.zeros(n, dtype=torch.int32, device="cuda")
    L, iv, x = (torch.zeros((n, m), dtype=torch.float32, device="cuda") for m in (6, 3, 3))
    _ok(lib, lib.mrp_chol3_f32(n, _ptr(Rd), _ptr(bd), _ptr(ok), _ptr(L), _ptr(iv), _ptr(x), _stream()))
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (ok, L, iv, x))


# ---- host ----
def host_dynamics_f32(cfg, tyres, x, u, nu, jac=True):
    n = x.shape[0]
    x, u, nu = (np.ascontiguousarray(t, np.float32) for t in (x, u, nu))
    f = np.zeros((n, 6), np.float32)
    J = np.zeros((n, 48), np.float32) if jac else None
    H = np.zeros((n, 36), np.float32) if jac else None
    pa, Fa, pb, Fb, keep = _tyre_args(tyres)
    assert ht.lib().mrh_eval_dynamics_f32(ctypes.byref(cfg), pa, Fa, pb, Fb, n, _v(x), _v(u), _v(nu), _v(f), _v(J),
                                          _v(H)) == 0
    del keep
    return f, J, H


def host_dynamics_f64(cfg, tyres, x, u, nu):
    """The fp64 host evaluation (mrh_eval_dynamics, pinned to autograd by tests/test_host_twin.py), point by point."""
    n = x.shape[0]
    x, u, nu = (np.ascontiguousarray(t, np.float64) for t in (x, u, nu))
    f, J, H = np.zeros((n, 6)), np.zeros((n, 48)), np.zeros((n, 36))
    pa, Fa, pb, Fb, keep = _tyre_args(tyres)
    P = lambda a: a.ctypes.data_as(_PD)  # noqa: E731
    fn = ht.lib().mrh_eval_dynamics
    for i in range(n):
        assert fn(ctypes.byref(cfg), pa, Fa, pb, Fb, P(x[i]), P(u[i]), P(nu[i]), P(f[i]), P(J[i]), P(H[i])) == 0
    del keep
    return f, J, H


def host_chol3(R, b):
    n = R.shape[0]
    R, b = np.ascontiguousarray(R, np.float32), np.ascontiguousarray(b, np.float32)
    ok = np.zeros(n, np.int32)
    L, iv, x = (np.zeros((n, m), np.float32) for m in (6, 3, 3))
    assert ht.lib().mrh_chol3_f32(n, _v(R), _v(b), _v(ok), _v(L), _v(iv), _v(x)) == 0
    return ok, L, iv, x
