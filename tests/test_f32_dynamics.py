"""CPU-side guard of the fp32 dynamics yardstick: mrh_eval_dynamics_f32 (Dyn<float, MODEL> with libm) stays
within 64 eps32 of the fp64 host evaluation, per output index of f (6), J (48) and H (36), in column-scale units
(max over the batch of |out - ref| over max over the batch of |ref|).

tests/test_gpu_f32_dynamics.py allows the device 8 x the host's fp32 error; this keeps that yardstick from being
so bad that 8 x of it hides a device error.  Measured maxima (eps32): f 2.3, J 3.8, H 5.0 over the five models at
the learned coefficients; f 1.2, J 2.9, H 2.6 with the default coefficients at Fz = 1, slip angles down to 1e-6
included.

A column that exceeds the bar would be cancellation in the model: it is named in CANCELLING, and the GPU test then
measures it against the fp64 evaluation's sensitivity to one ulp of each input instead.  None is named now.  Before
pacejka_jet got its fp32 forms past the 1e-3 series switch (atanc_m1_jet, sinc_jet in csrc/mr_common.h), the direct
form's (q x - atan x) / x^2 cancelled to ~ eps / x^2 there and H[26], H[30] reached 558.6 eps32 with the default
coefficients (64.8 - 68.0 on H[29], H[32], H[35]); the device showed the same (486.6).
"""
import numpy as np
import pytest

import f32_dynamics_cases as dc
import f32_probe as fp

BAR = 64 * dc.EPS32
# (case id, output, column) of columns whose host fp32 error exceeds the bar by cancellation in the model: none
CANCELLING = set()


@pytest.mark.parametrize("cid,model,tyre_name,kind", dc.CASES, ids=[c[0] for c in dc.CASES])
def test_host_f32_dynamics_within_64_eps(cid, model, tyre_name, kind):
    x, u, nu = dc.points(kind)
    cfg, ty = dc.config(model), dc.tyres(tyre_name)
    ref = fp.host_dynamics_f64(cfg, ty, x, u, nu)
    out = fp.host_dynamics_f32(cfg, ty, x, u, nu)
    for name, o, r in zip("fJH", out, ref):
        e, scale = dc.column_errors(o, r)
        print(cid, name, "max %.1f eps32" % (e.max() / dc.EPS32))
        over = {(cid, name, int(c)) for c in np.flatnonzero(e > BAR)}
        assert over <= CANCELLING, sorted(over - CANCELLING)
        assert (o[:, scale == 0] == 0).all()  # structural zeros stay exact zeros


def test_regions_are_unambiguous():
    """Every point of the range set is at least 1e-3 m/s from Vblendmin / Vblendmax in fp64, a third in each region."""
    x, _, _ = dc.points("range")
    s = dc.speed64(x)
    assert (np.abs(s - dc.VMIN) >= dc.MARGIN).all() and (np.abs(s - dc.VMAX) >= dc.MARGIN).all()
    counts = [(s < dc.VMIN).sum(), ((s > dc.VMIN) & (s < dc.VMAX)).sum(), (s > dc.VMAX).sum()]
    assert min(counts) >= dc.N // 3
    assert x[:, 3].min() >= 0.5 and x[:, 3].max() <= 45.0


def test_value_only_matches_fjh_on_host():
    for cid, model, tyre_name, kind in dc.CASES:
        x, u, nu = dc.points(kind, 128)
        cfg, ty = dc.config(model), dc.tyres(tyre_name)
        f1 = fp.host_dynamics_f32(cfg, ty, x, u, nu, jac=False)[0]
        f2 = fp.host_dynamics_f32(cfg, ty, x, u, nu)[0]
        scale = np.abs(f2).max(0)
        assert (np.abs(f1.astype(np.float64) - f2) <= 4 * dc.EPS32 * scale).all(), cid


def test_fp32_tyre_jet_across_the_switches():
    """pacejka_jet<float> (value, d/dalpha, d2/dalpha2) with the default coefficients at Fz = 1 for |alpha| from 1e-4
    to 1.5: |B alpha| runs from 3e-5 through the 1e-3 series switch, the 0.25 switch of atanc_m1_jet and the 0.5
    switch of sinc_jet.  Each stays within 16 eps32 of the fp64 jet in units of its largest value over the range
    (the floor of the device bar); measured 1.0, 1.2, 1.7, and at most 2.7 eps32 of the value itself point by point
    (558.6 in H before the fp32 forms)."""
    import ctypes
    import host_twin as ht
    PD = ctypes.POINTER(ctypes.c_double)
    a, Fz = dc.DEFAULT_FZ1
    pa = np.asarray(a, np.float64)
    al = np.exp(np.linspace(np.log(1e-4), np.log(1.5), 400))
    al = np.concatenate([al, -al]).astype(np.float32)
    o = np.zeros((2, al.size, 3))
    for i, t in enumerate(al):
        for fp32 in (0, 1):
            assert ht.lib().mrh_pacejka(pa.ctypes.data_as(PD), Fz, float(t), fp32, o[fp32, i].ctypes.data_as(PD)) == 0
    e = np.abs(o[1] - o[0]).max(0) / np.abs(o[0]).max(0) / dc.EPS32
    print("fp32 tyre jet, eps32 of the column scale:", e.round(2))
    assert (e <= 16).all(), e
