"""The fp32 scalar functions and 3 x 3 pivots of the gfx950 build, one by one, against numpy fp64.

On the device mr_tan / mr_atan2 / mr_log / mr_rsqrt are hardware forms (csrc/mr_common.h) and the library is
built with approximate transcendentals, reciprocal-based division and flushed denormals (mpcracing/build.py),
so none of this code runs in the host build.  The probe library (csrc/mr_probe.hip) compiles the same headers
with the same flags and evaluates one function per lane.

Reference: numpy fp64 of the fp32 input.  Yardstick: the same function in numpy float32 on the same inputs,
measured here.  Bar: device error <= 8 x max(host error, 1 ulp) -- 8 is the project's factor for device against
host fp32, the floor stands in where libm is exact.  Errors are in ulps of the reference for sqrt,
exp, rsqrt, atan, / and 1/x, and |err| / max(|ref|, 1) in units of eps32 for sin, cos, tan and log, whose hardware
forms are accurate absolutely, not relatively, near their zeros.

mr_atan2 is held to bounds derived from its form instead: 5.5e-7 rad absolutely over the plane (6.5e-8 of the
polynomial, 2.8e-7 for three relative ulps on r <= pi/4, 0.9e-7 for pi in fp32, 1.2e-7 for the last rounding) and
9.0e-7 relatively for |angle| < 0.1 (5.4e-7 of the polynomial's leading coefficient, 3 ulp).

Measured on an MI355X (profiles/f32_accuracy.json "math", "atan2", "chol3"), device / host: sin 4.0 / 0.5, cos
3.7 / 0.5, tan 4.0 / 0.8, log 1.3 / 0.7 eps32; atan 1.5 / 1.3, sqrt 0.9 / 0.5, exp 0.7 / 2.0, rsqrt 0.8 / 1.4,
a / b 1.6 / 0.5, 1 / a 0.8 / 0.5 ulp.  mr_atan2: 2.77e-7 rad absolute at (y, x) = (2.44e-3, -3.17e-3), 6.81e-7
relative for |angle| < 0.1 (numpy's atan2f: 2.65e-7 and 1.58e-7); 10.6 ulp at worst.  3 x 3 solves: 1 834 eps32
against the host's 3 467, 1.5 / 2.4 when divided by the condition number.
"""
import numpy as np
import pytest

import f32_probe as fp

pytestmark = pytest.mark.gpu

N = 4096
F32 = np.float32
PI = np.pi


def _logu(rng, lo, hi, n=N):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def _cases():
    """op -> (a, b or None, fp64 reference function, numpy float32 yardstick function, error measure)."""
    rng = np.random.default_rng(42)
    sc = np.concatenate([rng.uniform(-2 * PI, 2 * PI, N), [0.0, PI, -PI, PI / 2, -PI / 2]]).astype(F32)
    tn = np.concatenate([rng.uniform(-1.3, 1.3, N), [1e-6, -1e-6, 1.3, -1.3]]).astype(F32)
    at = (np.where(rng.random(N) < 0.5, -1, 1) * _logu(rng, 1e-4, 1e4)).astype(F32)
    ex = np.concatenate([rng.uniform(-87, 20, N), [-60.0, -87.0, 20.0, 0.0]]).astype(F32)
    lg = np.concatenate([_logu(rng, 1e-30, 1e6), [1 + 2.0 ** -23, 1 - 2.0 ** -23, 1 + 1e-3, 1 - 1e-3]]).astype(F32)
    rs = _logu(rng, 1e-12, 1e12).astype(F32)
    num, den = _logu(rng, 1e-6, 1e6).astype(F32), _logu(rng, 1e-6, 1e6).astype(F32)
    one = F32(1)
    return {
        "sin": (sc, None, np.sin, np.sin, fp.abs_err_eps),
        "cos": (sc, None, np.cos, np.cos, fp.abs_err_eps),
        "tan": (tn, None, np.tan, np.tan, fp.abs_err_eps),
        "log": (lg, None, np.log, np.log, fp.abs_err_eps),
        "atan": (at, None, np.arctan, np.arctan, fp.ulp_err),
        "sqrt": (rs, None, np.sqrt, np.sqrt, fp.ulp_err),
        "exp": (ex, None, np.exp, np.exp, fp.ulp_err),
        "rsqrt": (rs, None, lambda a: 1.0 / np.sqrt(a), lambda a: one / np.sqrt(a), fp.ulp_err),
        "div": (num, den, lambda a, b: a / b, lambda a, b: a / b, fp.ulp_err),
        "rcp": (den, None, lambda a: 1.0 / a, lambda a: one / a, fp.ulp_err),
    }


CASES = _cases()


@pytest.mark.parametrize("op", list(CASES))
def test_scalar_function(op):
    a, b, ref_fn, host_fn, measure = CASES[op]
    args64 = [a.astype(np.float64)] + ([b.astype(np.float64)] if b is not None else [])
    args32 = [a] + ([b] if b is not None else [])
    ref = ref_fn(*args64)
    host = host_fn(*args32)
    assert host.dtype == np.float32
    dev = fp.dev_math(op, a, b)
    keep = ref != 0 if measure is fp.ulp_err else np.ones(ref.shape, bool)
    e_dev, e_host = measure(dev, ref)[keep], measure(host, ref)[keep]
    i = int(np.argmax(e_dev))
    fig = {"unit": "ulp" if measure is fp.ulp_err else "eps32 of max(|ref|, 1)", "device_max": float(e_dev.max()),
           "host_max": float(e_host.max()), "bar": 8.0 * max(float(e_host.max()), 1.0),
           "worst_input": [float(t[keep][i]) for t in args32]}
    fp.record("math_" + op, fig)
    assert np.isfinite(dev).all()
    assert fig["device_max"] <= fig["bar"], fig


def test_log_edges():
    """0 -> -inf, a negative -> NaN (as logf); a denormal input is flushed: -inf."""
    out = fp.dev_math("log", np.array([0.0, -0.0, -1.5, 1e-40, 1.0], F32))
    assert out[0] == -np.inf and out[1] == -np.inf and np.isnan(out[2]) and out[3] == -np.inf and out[4] == 0.0


def test_zero_arguments():
    """sin(0), tan(0), atan(0) are 0 and cos(0) is 1 to the last bit: the zero-slip point of the model."""
    z = np.zeros(1, F32)
    assert fp.dev_math("sin", z)[0] == 0 and fp.dev_math("tan", z)[0] == 0 and fp.dev_math("atan", z)[0] == 0
    assert fp.dev_math("cos", z)[0] == 1


# ---- mr_atan2 ----
ATAN2_ABS = 5.5e-7
ATAN2_REL = 9.0e-7


def _atan2_points():
    rng = np.random.default_rng(43)
    th = rng.uniform(-PI, PI, N)
    r = _logu(rng, 1e-3, 1e2)
    ys, xs = [r * np.sin(th)], [r * np.cos(th)]
    # the solver's range: x = vx + 0.1, y = vy +- l r, slip angles down to 1e-6
    xs.append(rng.uniform(0.6, 45.1, N))
    ys.append(np.where(rng.random(N) < 0.5, -1, 1) * np.where(rng.random(N) < 0.5, rng.uniform(0, 3, N), _logu(rng, 1e-6, 3)))
    m = _logu(rng, 1e-3, 1e2, 64)
    for sy, sx in ((1, 1), (1, -1), (-1, 1), (-1, -1)):  # the diagonals |x| == |y| in the four quadrants
        ys.append(sy * m)
        xs.append(sx * m)
    for sy, sx in ((0, 1), (0, -1), (1, 0), (-1, 0)):  # the axes
        ys.append(sy * m)
        xs.append(sx * m)
    return np.concatenate(ys).astype(F32), np.concatenate(xs).astype(F32)


def test_atan2_derived_bounds():
    y, x = _atan2_points()
    ref = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    host = np.arctan2(y, x)
    dev = fp.dev_math("atan2", y, x)
    assert np.isfinite(dev).all()
    e_dev, e_host = np.abs(dev - ref), np.abs(host - ref)
    small = (np.abs(ref) < 0.1) & (ref != 0)
    assert small.sum() > 1000
    r_dev, r_host = e_dev[small] / np.abs(ref[small]), e_host[small] / np.abs(ref[small])
    i, j = int(np.argmax(e_dev)), int(np.argmax(r_dev))
    fig = {"abs_max_rad": float(e_dev.max()), "abs_max_at_yx": [float(y[i]), float(x[i])], "abs_bound": ATAN2_ABS,
           "rel_max_small_angle": float(r_dev.max()), "rel_max_at_yx": [float(y[small][j]), float(x[small][j])],
           "rel_bound": ATAN2_REL, "host_abs_max_rad": float(e_host.max()), "host_rel_max_small_angle": float(r_host.max()),
           "abs_max_in_ulp": float(fp.ulp_err(dev, ref)[ref != 0].max())}
    fp.record("atan2", fig)
    assert fig["abs_max_rad"] <= ATAN2_ABS, fig
    assert fig["rel_max_small_angle"] <= ATAN2_REL, fig
    assert (np.sign(dev) == np.sign(host)).all()  # every quadrant


def test_atan2_special_points():
    """Zeros: finite and signed as atan2f; (-0.0, x < 0) -> -pi."""
    y = np.array([0.0, -0.0, 0.0, -0.0, 2.0, -2.0, 2.0, -2.0, 0.0, -0.0, 0.0, -0.0], F32)
    x = np.array([3.0, 3.0, -3.0, -3.0, 0.0, 0.0, -0.0, -0.0, 0.0, 0.0, 45.1, 0.6], F32)
    dev = fp.dev_math("atan2", y, x)
    lib = np.arctan2(y, x)
    assert np.isfinite(dev).all()
    # (+-0, 0): atan2f gives +-0 for x = +0; the branch-free form returns the same
    assert (np.signbit(dev) == np.signbit(lib)).all(), (dev, lib)
    assert np.abs(dev - lib.astype(np.float64)).max() <= ATAN2_ABS
    assert dev[3] == F32(-PI) and dev[2] == F32(PI) and dev[0] == 0 and dev[1] == 0 and dev[8] == 0


# ---- 3 x 3 pivots ----
def _spd(n=1024):
    rng = np.random.default_rng(44)
    R6, b = np.zeros((n, 6), F32), rng.normal(0, 1, (n, 3)).astype(F32)
    cond = _logu(rng, 1.0, 1e4, n)
    scale = _logu(rng, 1e-3, 1e3, n)
    for i in range(n):
        Q, _ = np.linalg.qr(rng.normal(0, 1, (3, 3)))
        d = scale[i] * np.array([1.0, np.sqrt(cond[i]) ** rng.uniform(0, 2), cond[i]]) / cond[i]
        M = (Q * d) @ Q.T
        R6[i] = [M[0, 0], M[1, 0], M[2, 0], M[1, 1], M[2, 1], M[2, 2]]
    return R6, b, cond


def _full(R6):
    M = np.zeros((R6.shape[0], 3, 3))
    for q, (i, j) in enumerate(((0, 0), (1, 0), (2, 0), (1, 1), (2, 1), (2, 2))):
        M[:, i, j] = M[:, j, i] = R6[:, q]
    return M


def test_chol3_solve():
    R6, b, cond = _spd()
    ref = np.linalg.solve(_full(R6.astype(np.float64)), b.astype(np.float64)[:, :, None])[:, :, 0]
    ok_d, L_d, iv_d, x_d = fp.dev_chol3(R6, b)
    ok_h, L_h, iv_h, x_h = fp.host_chol3(R6, b)
    assert ok_d.all() and ok_h.all()
    nrm = np.abs(ref).max(1)
    e_d = np.abs(x_d - ref).max(1) / nrm / fp.EPS32
    e_h = np.abs(x_h - ref).max(1) / nrm / fp.EPS32
    fig = {"unit": "eps32, normwise relative error of the solution", "device_max": float(e_d.max()),
           "host_max": float(e_h.max()), "device_max_over_cond": float((e_d / cond).max()),
           "host_max_over_cond": float((e_h / cond).max())}
    fp.record("chol3", fig)
    assert fig["device_max"] <= 8 * max(fig["host_max"], 1.0), fig
    assert fig["device_max_over_cond"] <= 8 * max(fig["host_max_over_cond"], 1.0), fig
    # the factor itself: L L^T = R to 8 eps of the diagonal scale
    Lm = np.zeros((R6.shape[0], 3, 3))
    Lm[:, 1, 0], Lm[:, 2, 0], Lm[:, 2, 1] = L_d[:, 1], L_d[:, 3], L_d[:, 4]
    for k in range(3):
        Lm[:, k, k] = 1.0 / iv_d[:, k].astype(np.float64)
    M = _full(R6.astype(np.float64))
    back = np.abs(Lm @ Lm.transpose(0, 2, 1) - M).max((1, 2)) / np.abs(M).max((1, 2))
    assert back.max() <= 8 * 3 * fp.EPS32, back.max()  # three products per entry, 8 x the host's rounding


def test_chol3_failed_pivots_stay_finite():
    """A zero or negative pivot in each of the three positions: ok is false, and the branch-free replacement of the
    pivot by 1 keeps L, iv and x free of NaN and inf."""
    R6 = np.array([[0, 1, 2, 3, 1, 4], [-1, 1, 2, 3, 1, 4],          # first pivot zero / negative
                   [4, 0, 0, 0, 0, 1], [4, 2, 0, 0.5, 0, 1],          # second
                   [1, 0, 0, 1, 0, 0], [1, 0, 0, 1, 0, -2], [4, 2, 2, 5, 1, 0.5]], F32)  # third
    b = np.tile(np.array([1.0, -2.0, 3.0], F32), (R6.shape[0], 1))
    for who, (ok, L, iv, x) in (("device", fp.dev_chol3(R6, b)), ("host", fp.host_chol3(R6, b))):
        assert not ok.any(), (who, ok)
        assert np.isfinite(L).all() and np.isfinite(iv).all() and np.isfinite(x).all(), who
    ok, *_ = fp.dev_chol3(np.array([[4, 2, 2, 5, 1, 3]], F32), b[:1])
    assert ok.all()
