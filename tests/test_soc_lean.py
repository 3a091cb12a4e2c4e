"""The lean second-order correction (mr_wave.h: the costate recursion's constants staged in LDS, the forward
recursion on two lane groups without a per-step store, the dual side of the direction -- DLAM, DY, DNU and the
dual step size -- finished by soc_commit for an accepted correction only) takes the same decisions as the
untouched scalar solver (mr_solver.h Solver): the emulated wave against the scalar build, fp64, at the C4 options
of test_ls_restructure.py.

Trace column 7 (the line-search marker) must be equal exactly, columns 0..6 (kkt, mu, alpha -- with the dual step
size soc_commit derives --, delta, theta, phi, ...) to rtol 1e-6 / atol 1e-12.  Worst error of the build before
this change as a fraction of that tolerance: instance 4341 0.033, instance 3049 0.074.

The final multipliers lam_g (duals=True): the scalar build exports none (its lam_g stays zero; only the wave
solver has write_lam_g), so there is no wave-against-scalar figure to measure.  The wave's lam_g is compared with
the recording of the emulated wave of the build before this change instead (tests/golden/soc_lean_lam_g_parent.npz,
the same two solves).  The change moves where the dual steps are computed, not how: the host build contracts
nothing, so the difference on the recording machine is exactly 0.  LAM_G_BAR = 1e-9 max|lam_g| only leaves room
for another libm's last-bit differences carried through 150 iterations (the trace's own agreement with the scalar
solver is about 1e-7 relative); a dual step formed from a wrong operand misses it by orders of magnitude."""
import os

import numpy as np
import pytest

import host_twin as ht
from mpcracing import workload as wl

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "soc_lean_lam_g_parent.npz")
LAM_G_BAR = 1e-9


def _solve_pair(i, max_iter):
    """(scalar outputs, wave outputs) of C4 instance i, each with its trace, the wave's with lam_g."""
    cfg = wl.CONFIGS["C4"]
    b = wl.make_batch("C4", limit=i + 1)
    sub = {k: (v[..., i:i + 1].copy() if v is not None else None) for k, v in b.items()}
    c = ht.config(cfg["N"], cfg["model"], "fp64", cfg["lane"], cfg["Ts"], tol=1e-4, acceptable_iter=15,
                  acceptable_tol=1e-2, max_iter=max_iter)
    kw = dict(nthreads=1, trace_instance=0, trace_cap=max_iter + 50)
    return ht.solve(c, sub, scalar=True, **kw), ht.solve(c, sub, scalar=False, duals=True, **kw)


@pytest.fixture(scope="module")
def parent_lam_g():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("inst,n_soc,n_short", [(4341, 61, 22), (3049, 31, 56)])
def test_wave_matches_scalar(inst, n_soc, n_short, parent_lam_g):
    a, w = _solve_pair(inst, 150)
    n = int(a["iters"][0])
    assert int(w["iters"][0]) == n and int(w["status"][0]) == int(a["status"][0])
    ta, tw = a["trace"][:n], w["trace"][:n]
    m = ta[:, 7]
    assert (m >= 100).sum() == n_soc               # accepted corrections: soc_commit's DLAM, DY, DNU and ad
    assert ((m > 0) & (m < 100)).sum() == n_short  # shortened steps (rejected corrections among them)
    np.testing.assert_array_equal(ta[:, 7], tw[:, 7])
    np.testing.assert_allclose(tw[:, :7], ta[:, :7], rtol=1e-6, atol=1e-12)
    g, lam = parent_lam_g[f"lam_g_{inst}"], w["lam_g"][:, 0]
    assert np.isfinite(lam).all() and np.abs(g).max() > 0
    d = float(np.abs(lam - g).max() / np.abs(g).max())
    print(f"instance {inst}: lam_g against the recording {d:.3e} of max|lam_g| (bar {LAM_G_BAR:.0e})")
    assert d <= LAM_G_BAR
