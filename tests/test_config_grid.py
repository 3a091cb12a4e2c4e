"""Both host builds of the solver source against the dense IPOPT oracle's committed log over the configuration grid.

tests/test_ipopt_trajectory.py holds the builds to the oracle at five configurations with default parameters.
tests/golden/config_grid_golden.npz (generator make_config_grid_golden.py, checks in tests/config_grid_cases.py)
covers what those leave out: horizons N = 1 .. 63 around every 16-lane group and the top slots, the dynamic +
Pacejka model, lane rows on every model, every controller field, the runtime row (n = 4, d_max), the vehicle block,
Ts = 0.1 / 0.02, absent state0 controls at N = 33, and batches whose runtime columns differ.  A swapped pair of
bounds, a constant left hard-coded or a runtime row read at the wrong column changes alpha, theta or kkt of some
iteration by far more than 1e-6; final-point tests at the default parameters cannot see any of them.

* fp64 rows, every prefix / whole case and every column of the mixed batches, scalar and emulated-wave builds: the
  bars of ipopt_trace_cases.check_rows over the case's n_cmp rows; whole solves also iterations / status /
  objective where compared to the end, and the final X, U, S, eC, eL to 1e-6 (U[0, N-1] and vx_N excepted).
* lam_g of the whole solves without lane rows (wave build; the scalar build exports none).
* mixed batch: five runtime columns, two of them with NaN state0 controls, in one batch of 5; traced at instance j
  it gives the B = 1 solve of column j bit for bit (trace and every output), which in turn meets the oracle's rows.
* fp32 rows of the host wave build within the recorded deviation (the same build: a change detector).
tests/test_gpu_config_grid.py holds the gfx950 build to the same fixture.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "mpc-racing_amd"))

import config_grid_cases as cg  # noqa: E402

G = cg.GEN
_solves = {}


def _host(case, scalar, precision="fp64"):
    """One host solve per (case, build, precision), shared by the tests below."""
    key = (case, scalar, precision)
    if key not in _solves:
        _solves[key] = G.host_solve(case, scalar, precision)
    return _solves[key]


def test_config_grid_fixture():
    """The fixture itself: its inputs are what mpcracing.workload makes today, its index states the generator's
    cases, and every condition the generator asserted still reads true of the committed files."""
    arrays, index = cg.fixture()
    assert sorted(index) == sorted(G.CASES)
    assert os.path.getsize(G.NPZ) + os.path.getsize(G.INDEX) < G.MAX_BYTES
    lane_delta = 0.0
    for case, s in G.CASES.items():
        e = index[case]
        assert {k: e[k] for k in s} == s, case
        assert tuple(e["runtime"]) == tuple(G.case_runtime(case)), case
        assert np.array_equal(arrays[f"{case}/in"], G.pack_inputs(G.case_inputs(case)), equal_nan=True), case
        log = arrays[f"{case}/log"]
        assert log.shape == (e["log_rows"], 7) and np.isfinite(log).all()
        assert e["log_rows"] == (e["rows"] if (s["kind"] != "whole" or e["whole"]) else e["n_cmp"])
        assert e["whole"] == (e["status"] == 0 and e["n_cmp"] == e["rows"] == e["iters"])
        assert not log[:e["n_cmp"], cg.LOG_COL["in_resto"]].any()
        assert max(e["host_worst_dev"][c] for c in ("alpha", "theta", "kkt")) <= G.T.N_CMP_RTOL
        assert max(e["host_worst_dev"][c] for c in ("mu", "delta")) <= 1e-12
        N = s["N"]
        if s["kind"] == "whole":
            assert e["whole"] if case in G.WHOLE_TO_END else G.K_PREFIX <= e["n_cmp"] <= e["rows"]
            assert arrays[f"{case}/sol"].shape == (6 * (N + 1) + 2 * N + N + 1 + 2 * N,)
            assert (f"{case}/lam_g" in arrays) == (not s["lane"])
            if not s["lane"]:
                assert arrays[f"{case}/lam_g"].shape == (13 * N + 9,)
        else:
            assert e["n_cmp"] == e["rows"] >= 1
        if s["kind"] == "fp32":
            assert e["rows"] == G.K_FP32 and arrays[f"{case}/fp32"].shape == (G.K_FP32 + len(G.FP32_COLS),)
        if s["veh"]:
            assert e["vehicle"] == G.VEH and e["dynamics_dev"] <= 1e-12
            assert G.VEH["C_wheel"] == 2 * 3.14 * G.VEH["r_wheel"]
        if s["nan"]:
            assert np.isnan(arrays[f"{case}/in"][6:8]).all()
        if case in G.VMAX_CASES:  # the speed-limit term exp(q_v_max (vx - v_max)) is observed, not negligible
            assert s["par"] and e["vmax_term"] >= G.VMAX_TERM_MIN
        if "blend" in s["model"] and (s["lane"] or "pacejka" in s["model"]) and not s["veh"]:
            v = np.hypot(*arrays[f"{case}/in"][3:5])  # starts inside the blend region: the blend law is exercised
            assert 2.0 < v < 15.0, (case, v)
        if s["lane"]:
            lane_delta = max(lane_delta, e["max_delta"])
    assert lane_delta >= 1e2  # the inertia correction is exercised off N = 40
    assert all(index[c]["whole"] for c in G.WHOLE_TO_END)
    for group in G.MIX_GROUPS.values():
        rts = [tuple(index[c]["runtime"]) for c in group]
        assert len(set(rts)) == 5 and {rt[3] for rt in rts} == {2.0, 4.0}
        assert [index[c]["nan"] for c in group] == [j in G.MIX_NAN for j in range(5)]


@pytest.mark.parametrize("scalar", [True, False], ids=["scalar", "wave"])
@pytest.mark.parametrize("case", cg.cases("prefix", "whole", mix=True))
def test_host_build_iterates_match_oracle_log(case, scalar):
    label = "scalar" if scalar else "wave"
    o = _host(case, scalar)
    cg.check_rows(case, o["trace"], label)
    if G.CASES[case]["kind"] == "whole":
        cg.check_whole(case, o["status"][0], o["iters"][0], o["obj"][0], label)
        cg.check_point(case, o, label)


@pytest.mark.parametrize("case", [c for c in cg.cases("whole") if not G.CASES[c]["lane"]])
def test_wave_lam_g_matches_oracle_log(case):
    o = _host(case, False)
    lam = o["lam_g"][:, 0]
    assert not np.isnan(lam).any()
    cg.check_lam_g(case, lam, "wave")


@pytest.mark.parametrize("scalar", [True, False], ids=["scalar", "wave"])
@pytest.mark.parametrize("group", sorted(G.MIX_GROUPS))
def test_mixed_runtime_batch(group, scalar):
    """Five different runtime columns (and NaN state0 controls in two) in one batch: instance j is the B = 1 solve
    of column j bit for bit -- nothing of a neighbour's row, and nothing of column 0's, reaches it."""
    label = "scalar" if scalar else "wave"
    cols = G.MIX_GROUPS[group]
    batch = G.stack_inputs(cols)
    assert batch["runtime"].shape == (5, 5) and len({tuple(c) for c in batch["runtime"].T}) == 5
    for j, case in enumerate(cols):
        one = _host(case, scalar)
        o = G.host_solve(case, scalar, batch=batch, trace_instance=j, nthreads=5)
        assert np.array_equal(o["trace"].view(np.uint64), one["trace"].view(np.uint64)), (group, j)
        for k, v in one.items():
            if k != "trace":
                mine = np.ascontiguousarray(o[k][..., j:j + 1])
                assert mine.dtype == v.dtype and np.array_equal(mine.view(np.uint8), v.view(np.uint8)), (group, j, k)
        cg.check_rows(case, o["trace"], f"{label} batch[{j}]")


@pytest.mark.parametrize("case", cg.cases("fp32"))
def test_wave_fp32_first_rows_match_oracle_log(case):
    """The host wave fp32 build: markers those of the fp64 build on the oracle's trajectory, every column within
    the deviation the generator recorded for this same build (x 1.0: a change detector)."""
    _log, marker, host_dev = cg.fp32_reference(case)
    tr = _host(case, False, "fp32")["trace"]
    assert np.array_equal(tr[:G.K_FP32, cg.TRACE_COL["marker"]], marker)
    assert np.array_equal(_host(case, False)["trace"][:G.K_FP32, cg.TRACE_COL["marker"]], marker)
    dev = cg.fp32_dev(case, tr)
    for c, h in zip(G.FP32_COLS, host_dev):
        assert dev[c] <= h, (case, c, dev[c], h)
