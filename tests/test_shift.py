"""Both host builds against the dense IPOPT oracle where the inertia shift is large at once.

tests/test_ipopt_trajectory.py and tests/test_config_grid.py compare only rows on which BOTH host builds already
sit within 1e-8 of the oracle, so a loss of accuracy of the wave path alone shortens their prefix and fails nothing.
tests/golden/shift_golden.npz (generator make_shift_golden.py) holds the oracle's first 12 iterations on twelve
slow C3 cars under braking that accept delta = 100 (two: 1) in their first iteration, two of them again without
lane rows, and two controls; its rows were selected by the scalar build alone (within 1e-7 of the oracle, at
least 8 rows per case).  Here the scalar Solver and the emulated wavefront -- the kernel's own source -- are held to
those rows at the bars of tests/ipopt_trace_cases.py: alpha, theta, kkt to 1e-6 relative, mu and delta to 1e-12.
tests/test_gpu_shift.py holds the gfx950 build to the same fixture.
"""
import os

import numpy as np
import pytest

import shift_cases as sc
from mpcracing import workload as wl

G = sc.GEN
_solves = {}


def _host(case, scalar):
    """One host solve per (case, build), shared by the tests below."""
    if (case, scalar) not in _solves:
        _solves[case, scalar] = G.host_solve(case, scalar)
    return _solves[case, scalar]


def test_shift_fixture():
    """The fixture itself: its inputs are what mpcracing.workload makes today, every case keeps at least 8 rows on
    which the scalar build was within 1e-7 of the oracle, every case starts with an accepted shift of at least 1,
    and the kkt / theta columns are the oracle's own wherever it scaled no row."""
    arrays, index = sc.fixture()
    assert sorted(index) == sorted(G.CASES)
    assert os.path.getsize(G.NPZ) + os.path.getsize(G.INDEX) < G.MAX_BYTES
    assert G.OPT == dict(tol=1e-8, acceptable_tol=1e-6, acceptable_iter=15, max_iter=12)
    last = max(s["instance"] for s in G.CASES.values())
    b = wl.make_batch("C3", limit=last + 1)
    assert wl.CONFIGS["C3"]["model"] == "dyn" and wl.CONFIGS["C3"]["N"] == 40 and wl.CONFIGS["C3"]["lane"]
    for case, s in G.CASES.items():
        e = index[case]
        assert (e["config"], e["instance"], e["lane_bounds"], e["kind"], e["options"]) == \
            ("C3", s["instance"], s["lane"], s["kind"], G.OPT)
        i = s["instance"]
        for k in G.IN_KEYS:
            if b[k] is None:
                assert f"{case}/in_{k}" not in arrays, (case, k)
            else:
                assert np.array_equal(arrays[f"{case}/in_{k}"], b[k][..., i:i + 1]), (case, k)
        log, scaled = arrays[f"{case}/log"], arrays[f"{case}/log_scaled"]
        assert log.shape == (G.K_SHIFT, 7) == (e["rows"], 7) and np.isfinite(log).all()
        assert G.MIN_N_CMP <= e["n_cmp"] <= e["rows"]
        assert not log[:, sc.LOG_COL["in_resto"]].any()
        assert log[0, sc.LOG_COL["delta"]] == e["delta0"] >= 1.0
        assert max(e["scalar_worst_dev"][c] for c in ("alpha", "theta", "kkt")) <= G.N_CMP_RTOL
        assert max(e["scalar_worst_dev"][c] for c in ("mu", "delta")) <= 1e-12
        both = log[:, [sc.LOG_COL["kkt"], sc.LOG_COL["theta"]]]
        if e["min_row_scale"] == 1.0:  # no row scaled: the restated columns are the oracle's own
            assert e["max_row_gradient"] <= 100.0
            np.testing.assert_allclose(both, scaled, rtol=1e-12, atol=0.0, err_msg=case)
        else:  # rows scaled down: the oracle's theta is the smaller, and row 0 (a rollout) is the same
            assert e["max_row_gradient"] > 100.0 and (scaled[:, 1] <= both[:, 1]).all()
            np.testing.assert_allclose(both[0], scaled[0], rtol=1e-9, err_msg=case)
    assert sum(index[c]["min_row_scale"] < 1.0 for c in index) >= 4
    assert sum(index[c]["delta0"] == 100.0 for c in index) >= 12


@pytest.mark.parametrize("case", sc.cases("shift", "control"))
def test_scalar_iterates_match_oracle_log(case):
    """The scalar build: alpha, theta, kkt to 1e-6, mu and delta to 1e-12 over the case's n_cmp rows."""
    sc.check_rows(case, _host(case, True)["trace"], "scalar")


@pytest.mark.parametrize("case", sc.cases("shift", "control"))
def test_wave_iterates_match_oracle_log(case):
    """The emulated wavefront on the same rows at the same bars."""
    sc.check_rows(case, _host(case, False)["trace"], "wave")
