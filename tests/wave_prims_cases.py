"""Inputs of the wave-primitive probes and runners for the host emulation and the device (TEST-ONLY).

Shared by tests/test_wave_prims.py (CPU) and tests/test_gpu_wave_prims.py, so both see the same data.
"""
import ctypes

import numpy as np

import host_twin as ht
import wave_prims_ref as R

WL = 64
DTYPES = {"f32": np.float32, "f64": np.float64, "i32": np.int32}
MFMA_W = {"A": 5 * WL, "B": WL, "C": 4 * WL, "D": 8 * WL}


def _random_bits(rng, shape, dt):
    """Arbitrary bit patterns (NaNs, infinities and denormals included) for values that are only moved."""
    it = np.dtype(dt).itemsize
    raw = rng.integers(0, 2 ** 32, size=shape + ((it // 4),), dtype=np.uint64).astype(np.uint32)
    return np.ascontiguousarray(raw).view(dt).reshape(shape)


def prims_inputs(kind, nan=False):
    """[3][7][64]: three workgroups with different data.
    0: distinct positive values, a -0.0 and (f64) a denormal;  1: magnitudes over 12 decades with mixed signs, whose
    sum depends on the association;  2: distinct negative values.
    nan=True (floating types) puts one NaN into a single, different lane of each workgroup; the f64 one of
    workgroup 0 carries a payload in both 32-bit halves."""
    dt = np.dtype(DTYPES[kind])
    rng = np.random.default_rng({"f32": 11, "f64": 12, "i32": 13}[kind] + (100 if nan else 0))
    x = np.zeros((3, 7, WL), dt)
    lanes = np.arange(WL)
    if dt.kind == "f":
        x[0, 0] = (rng.permutation(WL) + 1) * 1.25 + 0.0625 * lanes
        x[0, 0, 7] = -0.0
        if dt == np.float64:
            x[0, 0, 21] = 3e-310  # denormal
        sign = np.where(rng.random(WL) < 0.5, -1.0, 1.0)
        x[1, 0] = sign * 10.0 ** rng.uniform(-6, 6, WL)
        x[2, 0] = -(rng.permutation(WL) + 1) * 0.37 - 1e-3 * lanes
        if nan:
            if dt == np.float64:
                x[0, 0, 33] = np.array([0x7FF8DEAD0BADBEEF], np.uint64).view(np.float64)[0]
            else:
                x[0, 0, 33] = np.array([0x7FC12345], np.uint32).view(np.float32)[0]
            x[1, 0, 0] = np.nan
            x[2, 0, 63] = np.nan
        for g in range(3):
            x[g, 1:7] = _random_bits(rng, (6, WL), dt)
        x[0, 1] = 1e30   # wany(v > a_0): false
        x[1, 1] = 0.0    # true
    else:
        x[0, 0] = rng.permutation(WL) * 1000 + 17
        x[1, 0] = rng.integers(-2 ** 24, 2 ** 24, WL)
        x[2, 0] = -(rng.permutation(WL) * 37 + 1)
        x[:, 1:7] = rng.integers(-2 ** 31, 2 ** 31, (3, 6, WL)).astype(np.int32)
        x[0, 1] = 2 ** 30
        x[1, 1] = 0
    return x


def mfma_inputs(kind):
    """A [3][5][64], B [3][64], C [3][4][64] per lane.  Workgroup 0: integer-valued matrices (every product and
    sum exact); 1: random; 2: identity pattern -- each lane's a and b hold its own lane number, C = 0, so that a
    wrong lane map shows as a wrong index."""
    dt = np.dtype(DTYPES[kind])
    rng = np.random.default_rng(21 if dt == np.float32 else 22)
    A = np.zeros((3, 5, WL), dt)
    B = np.zeros((3, WL), dt)
    C = np.zeros((3, 4, WL), dt)
    A[0] = rng.integers(-9, 10, (5, WL))
    B[0] = rng.integers(-9, 10, WL)
    C[0] = rng.integers(-99, 100, (4, WL))
    A[1] = rng.normal(0, 1, (5, WL)) * 10.0 ** rng.uniform(-2, 2, (5, WL))
    B[1] = rng.normal(0, 1, WL)
    C[1] = rng.normal(0, 3, (4, WL))
    A[2, 0] = np.arange(WL)
    A[2, 1:] = rng.integers(-3, 4, (4, WL))
    B[2] = np.arange(WL)
    return A, B, C


def second_matrix(A5):
    """The 16x16 left factor of the probe's second product: k-block s (columns 4 s .. 4 s + 3) from A5[1 + s]."""
    A2 = np.empty((16, 16), A5.dtype)
    for s in range(4):
        A2[:, 4 * s:4 * s + 4] = R.mfma_matrices(A5[1 + s], A5[0])[0]
    return A2


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_prims(x):
    kind = {v: k for k, v in DTYPES.items()}[x.dtype.type]
    x = np.ascontiguousarray(x)
    out = np.zeros((x.shape[0], R.N_SLOT, WL), x.dtype)
    lay = (ctypes.c_int32 * 8)()
    ht.lib().mrh_probe_layout(lay)
    assert (lay[0], lay[1], lay[6]) == (R.PRIMS_IN_W, R.N_SLOT * WL, R.N_SLOT)
    assert getattr(ht.lib(), "mrh_wave_prims_" + kind)(x.shape[0], _p(x), _p(out)) == 0
    return out


def host_mfma(A, B, C):
    kind = "f32" if A.dtype == np.float32 else "f64"
    A, B, C = (np.ascontiguousarray(t) for t in (A, B, C))
    D = np.zeros((A.shape[0], 8, WL), A.dtype)
    assert getattr(ht.lib(), "mrh_wave_mfma_" + kind)(A.shape[0], _p(A), _p(B), _p(C), _p(D)) == 0
    return D


def _dev_call(fn, n, ins, out_shape, dt):
    import torch
    from mpcracing import abi
    lib = abi.load_probe()
    dev = [torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in ins]
    out = torch.zeros(out_shape, dtype=getattr(torch, np.dtype(dt).name), device="cuda")
    rc = getattr(lib, fn)(n, *[ctypes.c_void_p(t.data_ptr()) for t in dev], ctypes.c_void_p(out.data_ptr()),
                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.mrp_last_error().decode()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def device_prims(x):
    kind = {v: k for k, v in DTYPES.items()}[x.dtype.type]
    return _dev_call("mrp_wave_prims_" + kind, x.shape[0], [x], (x.shape[0], R.N_SLOT, WL), x.dtype)


def device_mfma(A, B, C):
    kind = "f32" if A.dtype == np.float32 else "f64"
    return _dev_call("mrp_wave_mfma_" + kind, A.shape[0], [A, B, C], (A.shape[0], 8, WL), A.dtype)


# ---- checks against the restatement, shared by the host and the device tests ----
_REDUCE = ("sum", "max", "min")


def check_prims(out, x, who):
    """Every slot of every workgroup equals the restatement bit for bit; reductions are lane-uniform unless the
    input holds a NaN (then max / min follow the restated butterfly lane by lane and the sum is NaN on every lane)."""
    for g in range(x.shape[0]):
        exp, have = R.prims_expected(x[g], g)
        has_nan = x.dtype.kind == "f" and bool(np.isnan(x[g, 0]).any())
        for name, s0 in R.SLOT.items():
            n = {"xor": 32, "bcast": 6, "gather": 6, "transpose": 4}.get(name, 1)
            for k in range(n):
                s = s0 + k
                if not have[s]:
                    continue
                if name == "sum" and has_nan:
                    assert np.isnan(out[g, s]).all(), (who, g, name)
                    continue
                bad = np.flatnonzero(R.bits(out[g, s]) != R.bits(exp[s]))
                assert bad.size == 0, (who, x.dtype.name, "workgroup", g, name, k, "lanes", bad.tolist()[:8],
                                       out[g, s][bad][:4], exp[s][bad][:4])
        if not has_nan:
            for name in _REDUCE:
                s = R.SLOT[name]
                assert (R.bits(out[g, s]) == R.bits(out[g, s])[0]).all(), (who, g, name, "not lane-uniform")
            if x.dtype.kind == "f":
                tot, bound = R.fsum_bound(x[g, 0])
                assert abs(float(out[g, R.SLOT["sum"], 0]) - tot) <= bound, (who, g, out[g, R.SLOT["sum"], 0], tot, bound)


def check_mfma(D, A, B, C, who):
    """Workgroups 0 and 2 (integer-valued) exact; workgroup 1 within 4 eps (|C| + |A| |B|) of the fp64 product; the
    second product A2 (A B) exact on 0 and 2 and within 20 eps |A2| (|A| |B|) on 1 (16 + 4 rounded terms)."""
    dt = A.dtype
    eps = float(np.finfo(dt).eps)
    res = {}
    for g in range(A.shape[0]):
        Am, Bm = R.mfma_matrices(A[g, 0], B[g])
        Cm = R.d_matrix(C[g])
        A2 = second_matrix(A[g])
        D1, D2 = R.d_matrix(D[g, :4]), R.d_matrix(D[g, 4:])
        hi = lambda t: t.astype(np.longdouble)  # noqa: E731
        P = hi(Am) @ hi(Bm)
        ref1, ref2 = hi(Cm) + P, hi(A2) @ P
        if g != 1:
            assert (hi(D1) == ref1).all(), (who, dt.name, g, "C + A B not exact", np.argwhere(hi(D1) != ref1)[:4].tolist())
            assert (hi(D2) == ref2).all(), (who, dt.name, g, "A2 (A B) not exact", np.argwhere(hi(D2) != ref2)[:4].tolist())
        else:
            b1 = 4 * eps * (np.abs(hi(Cm)) + np.abs(hi(Am)) @ np.abs(hi(Bm)))
            b2 = 20 * eps * (np.abs(hi(A2)) @ (np.abs(hi(Am)) @ np.abs(hi(Bm))))
            e1, e2 = np.abs(hi(D1) - ref1), np.abs(hi(D2) - ref2)
            res = {"err1_over_bound": float((e1 / b1).max()), "err2_over_bound": float((e2 / b2).max())}
            assert (e1 <= b1).all() and (e2 <= b2).all(), (who, dt.name, res)
    return res


def fma_chain_expected(A, B, C):
    """[n_wg][8][64] fp32: the registers a k-ordered fmaf chain gives (k = 0 .. 3 for C + A B; from zero over the 16
    columns of A2 in order for the second product, whose B fragments are the chain's own A B)."""
    out = np.zeros((A.shape[0], 8, WL), np.float32)
    for g in range(A.shape[0]):
        Am, Bm = R.mfma_matrices(A[g, 0], B[g])
        out[g, :4] = R.d_regs(R.mfma_fma_chain32(Am, Bm, R.d_matrix(C[g])))
        P = R.mfma_fma_chain32(Am, Bm, np.zeros((16, 16), np.float32))
        A2 = second_matrix(A[g])
        Q = np.zeros((16, 16), np.float32)
        for s in range(4):
            Q = R.mfma_fma_chain32(A2[:, 4 * s:4 * s + 4], P[4 * s:4 * s + 4], Q)
        out[g, 4:] = R.d_regs(Q)
    return out
