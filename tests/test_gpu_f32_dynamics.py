"""Dyn<float, MODEL>::f / ::fjh as compiled for gfx950, against the fp64 evaluation of the same points.

The fp32 solve evaluates these at every stage of every iteration, with the hardware sine, cosine, square root,
reciprocal and the polynomial atan2 of csrc/mr_common.h; the host build runs libm instead, and the fp64
mr_eval_dynamics is the only evaluation the other tests compare.  The probe (csrc/mr_probe.hip) builds
ProbParams<float> as mr_create / mr_set_tyres do and calls the model once per lane.

Reference: the device's fp64 mr_eval_dynamics on the float-rounded inputs (pinned to the host build and to
autograd by tests/test_gpu.py and tests/test_host_twin.py).  Yardstick: mrh_eval_dynamics_f32, the libm float
build.  Per output index j of f (6), J (48), H (36): e_j = max over the batch of |out - ref| over max over the
batch of |ref_j|, and e_dev_j <= max(8 e_host_j, 16 eps32).  For the columns where the host's own fp32 error
exceeds 64 eps32 (tests/test_f32_dynamics.py CANCELLING) the yardstick is the fp64 evaluation's change under one
fp32 ulp of each input, summed over the inputs, by central differences.

Measured on an MI355X (profiles/f32_accuracy.json "dynamics"), device / host maxima in eps32: f 2.7 / 2.3, J 3.8 /
3.8, H 5.6 / 5.0 over the five models at the learned coefficients; with the default coefficients at Fz = 1, f 2.5 /
1.2, J 3.1 / 2.9, H 2.4 / 2.4, slip angles down to 1e-6 included.  The last case found a defect, since fixed:
pacejka_jet's direct form past its 1e-3 series switch cancelled to ~ eps / x^2 in fp32, H[26] / H[30] 286 / 487
eps32 on the device (541 / 559 on the host) where one input ulp moves the fp64 value by 4; atanc_m1_jet and sinc_jet
(csrc/mr_common.h) replace it for fp32.
"""
import ctypes

import numpy as np
import pytest
import torch

import f32_dynamics_cases as dc
import f32_probe as fp
from mpcracing.batch import BatchSolver
from test_f32_dynamics import CANCELLING

pytestmark = pytest.mark.gpu

_solvers = {}


def dev_dynamics_f64(model, tyre_name, x, u, nu):
    """The product's fp64 mr_eval_dynamics on the device (batched)."""
    key = (model, tyre_name)
    if key not in _solvers:
        _solvers[key] = BatchSolver(20, model, "fp64", max_batch=1, tyres=dc.tyres(tyre_name))
    s = _solvers[key]
    n = x.shape[0]
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()  # noqa: E731
    X, U, NU = d(x), d(u), d(nu)
    f, J, H = (torch.zeros((n, m), dtype=torch.float64, device="cuda") for m in (6, 48, 36))
    rc = s.lib.mr_eval_dynamics(s.h, n, *[ctypes.c_void_p(t.data_ptr()) for t in (X, U, NU, f, J, H)],
                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    return f.cpu().numpy(), J.cpu().numpy(), H.cpu().numpy()


def ulp_sensitivity(model, tyre_name, x, u, nu):
    """Sum over the 14 inputs of |out(in + ulp) - out(in - ulp)| / 2 in fp64, ulp the fp32 spacing at the input."""
    ins = [x.astype(np.float64), u.astype(np.float64), nu.astype(np.float64)]
    tot = None
    for a, src in zip(ins, (x, u, nu)):
        for k in range(a.shape[1]):
            h = np.spacing(np.abs(src[:, k])).astype(np.float64)
            res = []
            for sgn in (1.0, -1.0):
                b = a.copy()
                b[:, k] += sgn * h
                args = [b if t is a else t for t in ins]
                res.append(dev_dynamics_f64(model, tyre_name, *args))
            d = [np.abs(p - m) / 2 for p, m in zip(*res)]
            tot = d if tot is None else [t + q for t, q in zip(tot, d)]
    return tot


@pytest.mark.parametrize("cid,model,tyre_name,kind", dc.CASES, ids=[c[0] for c in dc.CASES])
def test_device_f32_dynamics(cid, model, tyre_name, kind):
    x, u, nu = dc.points(kind)
    cfg, ty = dc.config(model), dc.tyres(tyre_name)
    if kind == "range":  # both precisions pick the same blend region
        s = dc.speed64(x)
        assert (np.abs(s - dc.VMIN) >= dc.MARGIN).all() and (np.abs(s - dc.VMAX) >= dc.MARGIN).all()
    ref = dev_dynamics_f64(model, tyre_name, x, u, nu)
    host = fp.host_dynamics_f32(cfg, ty, x, u, nu)
    dev = fp.dev_dynamics(cfg, ty, x, u, nu)
    sens = ulp_sensitivity(model, tyre_name, x, u, nu) if any(c[0] == cid for c in CANCELLING) else None
    fig, failed = {}, []
    for q, (name, o, h, r) in enumerate(zip("fJH", dev, host, ref)):
        assert np.isfinite(o).all(), (cid, name)
        e_dev, scale = dc.column_errors(o, r)
        e_host, _ = dc.column_errors(h, r)
        yard = e_host.copy()
        for (c_id, c_name, col) in CANCELLING:
            if c_id == cid and c_name == name:
                yard[col] = sens[q][:, col].max() / scale[col]
        bar = np.maximum(8 * yard, 16 * dc.EPS32)
        fig[name] = {"device_max_eps32": float(e_dev.max() / dc.EPS32), "host_max_eps32": float(e_host.max() / dc.EPS32),
                     "worst_device_over_bar": float((e_dev / bar).max()), "worst_column": int(np.argmax(e_dev / bar))}
        # structural zeros of the reference are exact zeros on the device
        assert (o[:, scale == 0] == 0).all(), (cid, name, "structural zero not zero")
        for c in np.flatnonzero(e_dev > bar):
            failed.append((name, int(c), "device %.1f host %.1f yardstick %.1f eps32" % (
                e_dev[c] / dc.EPS32, e_host[c] / dc.EPS32, yard[c] / dc.EPS32)))
    fp.record("dynamics_" + cid, fig)
    assert not failed, (cid, failed)
    # the value-only variant (line search, rollouts) against fjh's value
    f_only = fp.dev_dynamics(cfg, ty, x, u, nu, jac=False)[0]
    scale = np.abs(ref[0]).max(0)
    assert (np.abs(f_only.astype(np.float64) - dev[0]) <= 4 * dc.EPS32 * scale).all(), cid


@pytest.mark.parametrize("model", ["blend", "blend_pacejka"])
def test_blend_thresholds_value_only(model):
    """vy = 0 and vx exactly at Vblendmin / Vblendmax: the approximate square root may land on either side; the law is
    continuous there, so f still agrees (its derivatives need not, and are not compared)."""
    x, u, nu = dc.threshold_points()
    tyre_name = "pacejka-2" if "pacejka" in model else None
    cfg, ty = dc.config(model), dc.tyres(tyre_name)
    ref = dev_dynamics_f64(model, tyre_name, x, u, nu)[0]
    host = fp.host_dynamics_f32(cfg, ty, x, u, nu, jac=False)[0]
    for jac in (False, True):
        dev = fp.dev_dynamics(cfg, ty, x, u, nu, jac=jac)[0]
        e_dev, _ = dc.column_errors(dev, ref)
        e_host, _ = dc.column_errors(host, ref)
        print(model, "jac" if jac else "value", "device", (e_dev / dc.EPS32).round(1), "host", (e_host / dc.EPS32).round(1))
        assert (e_dev <= np.maximum(8 * e_host, 16 * dc.EPS32)).all(), (model, jac, e_dev / dc.EPS32)
