"""A numpy restatement of the wave primitives (csrc/mr_wave_prims.h) and of pick6 (csrc/mr_wave.h).

TEST-ONLY.  Written from the header's prose, not from its code: index permutations over the 64
lanes, the six-level reduction butterfly, the 16x16x4 MFMA lane maps and the 4x4 row transpose.
Every function takes and returns arrays indexed by lane (last axis of length 64) in the element
type of the input, so results can be compared bit for bit (``bits``).

``prims_expected`` lays the results out as the probe bodies of csrc/mr_probe.h store them.
"""
import math

import numpy as np

WL = 64
LANES = np.arange(WL)

# slots of the primitive probe (csrc/mr_probe.h PrimSlot), 64 words each
SLOT = {"shfl_const": 0, "shfl_uni": 1, "shfl_lane": 2, "shfl_rev": 3, "xor": 4, "next": 36, "prev": 37,
        "row_next": 38, "bcast": 39, "gather": 45, "sum": 51, "max": 52, "min": 53, "any_neg": 54, "all_neg": 55,
        "all_ord": 56, "any_big": 57, "uni": 58, "wu": 59, "transpose": 60, "buf_ld": 64, "buf_st": 65, "pick6": 66,
        "pick6_mod": 67}
N_SLOT = 68
PRIMS_IN_W = 7 * WL
BCAST_SRC = (0, 15, 16, 31, 32, 63)


def bits(a):
    """Integer view of an array: equality of bit patterns (-0.0, NaN payloads, denormals)."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---- moves ----
def shfl(v, src):
    """Lane l receives the value of lane src[l] (src taken mod 64)."""
    return v[..., np.asarray(src) % WL]


def xor(v, m):
    return v[..., LANES ^ m]


def nxt(v):
    """Value of lane (l + 1) mod 64."""
    return v[..., (LANES + 1) % WL]


def prv(v):
    """Value of lane (l - 1) mod 64."""
    return v[..., (LANES - 1) % WL]


def row_next(v):
    """Value of lane l + 1 within the lane's row of 16; 0 for the row's last lane."""
    out = v[..., np.minimum(LANES + 1, WL - 1)].copy()
    out[..., (LANES & 15) == 15] = 0
    return out


def bcast(v, s):
    return np.repeat(v[..., s:s + 1], WL, axis=-1)


def pick6(l, a):
    """a[l] for l < 5, a[5] for every l >= 5; a is [6][64] (lane's own arguments)."""
    l = np.asarray(l)
    return a[np.minimum(l, 5), LANES]


def transpose4(d):
    """d is [4][64]: register v of lane (g, c), g = lane >> 4, c = lane & 15, holds M[g][v] of column c's
    4x4 matrix; on exit register s of lane (g, c) holds M[s][g]."""
    out = np.empty_like(d)
    g, c = LANES >> 4, LANES & 15
    for s in range(4):
        out[s] = d[g, s * 16 + c]
    return out


# ---- reductions ----
def butterfly_partners():
    """The six levels' partner lanes: l^1, l^2, mirror within the half row of 8, mirror within the row of 16,
    l^16, l^32."""
    l = LANES
    return [l ^ 1, l ^ 2, (l & ~7) | (7 - (l & 7)), (l & ~15) | (15 - (l & 15)), l ^ 16, l ^ 32]


def butterfly(v, op):
    """Each level computes op(own, partner) on every lane, in the element type of v."""
    v = np.array(v, copy=True)
    for p in butterfly_partners():
        v = op(v, v[..., p])
    return v


def op_sum(a, b):
    return a + b


def op_max(a, b):
    """b > a ? b : a (a NaN compares false, so op(own, NaN) = own and op(NaN, partner) = NaN)."""
    return np.where(b > a, b, a)


def op_min(a, b):
    return np.where(b < a, b, a)


def fsum_bound(v):
    """(exact sum, 6 eps sum|v|): six additions per lane's tree, each within eps/2 of its partial sum."""
    v = np.asarray(v)
    eps = np.finfo(v.dtype).eps
    return math.fsum(float(x) for x in v), 6.0 * float(eps) * math.fsum(abs(float(x)) for x in v)


# ---- MFMA 16x16x4 ----
def mfma_operands(A, B):
    """Per-lane operands of D += A B, A [16][4], B [4][16]: lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15]."""
    return A[LANES & 15, LANES >> 4], B[LANES >> 4, LANES & 15]


def mfma_matrices(a, b):
    """Inverse of ``mfma_operands``: the matrices that per-lane operands a, b [64] stand for."""
    A = np.empty((16, 4), a.dtype)
    B = np.empty((4, 16), b.dtype)
    A[LANES & 15, LANES >> 4] = a
    B[LANES >> 4, LANES & 15] = b
    return A, B


def d_rows(dtype):
    """Row of D that register v of lane l holds, [4][64]: 4 (l >> 4) + v for f32, (l >> 4) + 4 v for f64."""
    v = np.arange(4)[:, None]
    g = (LANES >> 4)[None, :]
    return 4 * g + v if np.dtype(dtype).itemsize == 4 else g + 4 * v


def d_regs(M):
    """Registers [4][64] that hold the 16x16 matrix M (column l & 15)."""
    return M[d_rows(M.dtype), (LANES & 15)[None, :]]


def d_matrix(regs):
    M = np.empty((16, 16), regs.dtype)
    M[d_rows(regs.dtype), np.broadcast_to((LANES & 15)[None, :], (4, WL))] = regs
    return M


def fma32(a, b, c):
    """Correctly rounded fp32 a*b + c: the fp64 product of two fp32 numbers is exact, and the fp64 sum rounded to
    fp32 can differ from the single rounding only on a fp64 half-way case, which is detected and left to exact
    rational arithmetic."""
    from fractions import Fraction
    a, b, c = np.float32(a), np.float32(b), np.float32(c)
    s = np.float64(a) * np.float64(b) + np.float64(c)
    r = np.float32(s)
    if not np.isfinite(s) or np.float64(r) == s:
        return r
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    lo, hi = sorted((np.float32(r), np.nextafter(np.float32(r), np.float32(np.inf if exact > Fraction(float(r)) else -np.inf))))
    dl, dh = abs(exact - Fraction(float(lo))), abs(Fraction(float(hi)) - exact)
    if dl != dh:
        return lo if dl < dh else hi
    return lo if (int(np.float32(lo).view(np.uint32)) & 1) == 0 else hi


def mfma_fma_chain32(A, B, C):
    """C + A B in fp32 as a k-ordered chain of fused multiply-adds, k = 0 .. 3, per element."""
    D = np.array(C, dtype=np.float32, copy=True)
    for i in range(16):
        for j in range(16):
            acc = D[i, j]
            for k in range(4):
                acc = fma32(A[i, k], B[k, j], acc)
            D[i, j] = acc
    return D


# ---- the probe's expected output ----
def prims_expected(inp, wg):
    """Expected output [N_SLOT][64] of workgroup ``wg`` of the primitive probe, and the mask of the slots it
    writes for this element type.  inp is the workgroup's input [7][64]: v, a_0 .. a_5."""
    dt = inp.dtype
    v, a = inp[0], inp[1:7]
    out = np.zeros((N_SLOT, WL), dt)
    have = np.zeros(N_SLOT, bool)

    def put(name, x, k=0):
        out[SLOT[name] + k] = x
        have[SLOT[name] + k] = True

    put("shfl_const", shfl(v, np.full(WL, 37)))
    put("shfl_uni", shfl(v, np.full(WL, (wg * 5 + 11) & 63)))
    put("shfl_lane", shfl(v, (7 * LANES + 3) & 63))
    put("shfl_rev", shfl(v, 63 - LANES))
    for m in range(1, 33):
        put("xor", xor(v, m), m - 1)
    for k, s in enumerate(BCAST_SRC):
        put("bcast", bcast(v, s), k)
    for k in range(6):
        put("gather", bcast(v, k), k)
    put("sum", butterfly(v, op_sum))
    put("max", butterfly(v, op_max))
    put("min", butterfly(v, op_min))
    flag = lambda b: np.full(WL, 1 if b else 0, dt)  # noqa: E731
    put("any_neg", flag((v < 0).any()))
    put("all_neg", flag((v < 0).all()))
    put("all_ord", flag((v == v).all()))
    put("any_big", flag((v > a[0]).any()))
    put("uni", flag(v[3] > 0))
    put("wu", bcast(v, 9))
    put("pick6", pick6(LANES, a))
    put("pick6_mod", pick6(LANES & 7, a))
    if dt.kind == "f":
        put("next", nxt(v))
        put("prev", prv(v))
        put("row_next", row_next(v))
        put("buf_ld", a[1][(5 * LANES + 2) & 63])
        st = np.empty(WL, dt)
        st[(11 * LANES + 7) & 63] = v
        put("buf_st", st)
    if dt == np.float32:
        t = transpose4(a[:4])
        for s in range(4):
            put("transpose", t[s], s)
    return out, have
