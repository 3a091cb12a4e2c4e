"""Test helper: the PID agent of csrc/mr_pid.h built for the host (libmpcracing_host.so), on a
track_twin.HostTrack's tables.  TEST-ONLY -- the product path runs it on the GPU (mpcracing.pid)."""
import ctypes

import numpy as np

import host_twin as ht
from mpcracing import abi

NG, NM, NO, NL = abi.MR_PID_NGAIN, abi.MR_PID_NMEM, abi.MR_PID_NOUT, abi.MR_PID_NLOG


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _track_args(tr):
    return [_p(tr.blob), tr.nt, tr.L, tr.nr]


def gains_default():
    g = np.zeros(NG)
    assert ht.lib().mrh_pid_gains_default(g.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == 0
    return g


def control(tr, state, mem, gains, dt):
    """mrh_pid_control: state [6][n], mem [4][n], gains [G][8] -> (rc, out [8][n], new mem [4][n])."""
    state = np.ascontiguousarray(state, np.float64).reshape(6, -1)
    n = state.shape[1]
    mem = np.array(mem, np.float64).reshape(NM, n)
    gains = np.ascontiguousarray(np.atleast_2d(gains), np.float64)
    out = np.full((NO, n), np.nan)
    rc = ht.lib().mrh_pid_control(*_track_args(tr), n, _p(state), _p(mem), gains.shape[0], _p(gains), float(dt),
                                  _p(out))
    return rc, out, mem


def drive(tr, model, state, mem, gains, params, T, dt, mask=(1 << NL) - 1, G=None, P=None, log="auto", nthreads=16):
    """mrh_pid_drive: (rc, log [popcount(mask)][T][n] or None, state, mem, ticks_done); G / P / log override
    what the arrays imply (for the argument checks)."""
    state = np.array(state, np.float64).reshape(6, -1)
    n = state.shape[1]
    mem = np.array(mem, np.float64).reshape(NM, n)
    gains = np.ascontiguousarray(np.atleast_2d(gains), np.float64)
    params = np.ascontiguousarray(np.atleast_2d(params), np.float64)
    rows = bin(mask & ((1 << NL) - 1)).count("1")
    if isinstance(log, str):
        log = np.full((rows, max(T, 0), n), -7.0) if rows else None
    done = np.full(n, -1, np.int32)
    rc = ht.lib().mrh_pid_drive(*_track_args(tr), int(model), n, int(T), float(dt), _p(state), _p(mem),
                                gains.shape[0] if G is None else G, _p(gains), params.shape[0] if P is None else P,
                                _p(params), mask, _p(log), _p(done), nthreads)
    return rc, log, state, mem, done
