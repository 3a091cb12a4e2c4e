"""One horizon per instance in one batched solve (mr_solve_batch_horizons), both host builds of the solver source.

The horizon N of the reference is chosen per call from the car's speed (script/test_mpc.py:32-33); a batch of
vehicles at different speeds therefore needs a different N per instance.  The check is exact: instance i of a mixed
batch under the layout horizon 63 is, bit for bit, the solve of that instance alone by the existing entry point at
N = N_i -- the same code on the same inputs -- and NaN beyond its rows.  The instances are those of the committed
oracle log (tests/config_grid_cases.py), which holds the uniform solves to IPOPT at exactly these horizons; the
whole-solve columns are also checked against the log directly.  tests/test_gpu_horizons.py holds the gfx950 build
to the same.
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

import horizon_cases as hc  # noqa: E402
import host_twin as ht  # noqa: E402

G = hc.G
BUILDS = pytest.mark.parametrize("scalar", [True, False], ids=["scalar", "wave"])
# family x precision: the blend family in both precisions
FAMILY_PREC = [("kin", "fp64"), ("dyn_lane", "fp64"), ("blend_par", "fp64"), ("blend_par", "fp32")]
_cache = {}


def _config(cases, N, precision="fp64", options="prefix"):
    model, lane, Ts, over, _tyres = hc.family_config(cases)
    return ht.config(N, model, precision, lane, Ts, **G.OPTIONS[options], **over)


def _duals(cases, scalar):
    return not scalar and not G.CASES[cases[0]]["lane"]  # (the scalar build exports no lam_g)


def _mixed(cases, scalar, precision="fp64", options="prefix", u_init=None, tag=""):
    """The mixed batch of ``cases`` solved once per (cases, build, precision, u_init tag)."""
    key = ("mixed", tuple(cases), scalar, precision, options, tag)
    if key not in _cache:
        batch = hc.mixed_inputs(cases, u_init)
        _cache[key] = (batch, hc.host_solve(_config(cases, hc.NL, precision, options), batch, hc.horizons(cases),
                                            scalar=scalar, duals=_duals(cases, scalar)))
    return _cache[key]


def _uniform(cases, i, batch, scalar, precision="fp64", options="prefix", tag=""):
    """Instance i of ``batch`` alone through the EXISTING entry point (tests/host_twin.solve) at cfg.N = N_i."""
    key = ("one", cases[i], scalar, precision, options, tag)
    if key not in _cache:
        N = G.CASES[cases[i]]["N"]
        _cache[key] = ht.solve(_config(cases, N, precision, options), hc.one_instance(batch, i, N), nthreads=1,
                               scalar=scalar, duals=_duals(cases, scalar))
    return _cache[key]


@BUILDS
@pytest.mark.parametrize("family,precision", FAMILY_PREC, ids=[f"{f}-{p}" for f, p in FAMILY_PREC])
def test_mixed_batch_equals_uniform_solves(family, precision, scalar):
    cases = hc.FAMILIES[family]
    batch, o = _mixed(cases, scalar, precision)
    assert o["X"].shape == (6, hc.NL + 1, len(cases))
    for i, case in enumerate(cases):
        N = G.CASES[case]["N"]
        one = _uniform(cases, i, batch, scalar, precision)
        assert one["iters"][0] > 0
        hc.assert_column_is_uniform_solve(hc.column(o, i), one, N, f"{family} {precision} [{i}] N={N}")


@BUILDS
def test_u_init_is_read_with_the_layout_stride(scalar):
    """u_init [2][63][14] whose column i is NaN from row N_i on: row r of instance i is u_init[(r * 63 + k)], k <
    N_i.  A read at stride N_i, or of a row beyond N_i, meets a NaN and poisons the solve."""
    cases = hc.FAMILIES["kin"]
    Ns = hc.horizons(cases)
    u = hc.nan_padded_u_init(Ns)
    assert u.shape == (2, 63, 14) and all(np.isnan(u[:, N:, i]).all() and np.isfinite(u[:, :N, i]).all()
                                          for i, N in enumerate(Ns))
    batch, o = _mixed(cases, scalar, u_init=u, tag="u_init")
    for i, case in enumerate(cases):
        one = _uniform(cases, i, batch, scalar, tag="u_init")
        assert np.isfinite(one["X"]).all() and np.isfinite(one["U"]).all()
        hc.assert_column_is_uniform_solve(hc.column(o, i), one, int(Ns[i]), f"kin u_init [{i}] N={Ns[i]}")
    plain = _mixed(cases, scalar)[1]  # the warm start is used: some instance differs from the default start's
    assert any(not hc.bit_equal(o["U"][:, :N, i], plain["U"][:, :N, i]) for i, N in enumerate(Ns) if N >= 2)


@BUILDS
def test_instance_order_does_not_matter(scalar):
    cases = hc.FAMILIES["kin"]
    batch, o = _mixed(cases, scalar)
    perm = np.random.default_rng(5).permutation(len(cases))
    assert not np.array_equal(perm, np.arange(len(cases)))
    p = hc.host_solve(_config(cases, hc.NL), hc.permuted(batch, perm), hc.horizons(cases)[perm], scalar=scalar,
                      duals=_duals(cases, scalar))
    for k, v in o.items():
        assert hc.bit_equal(p[k], v[..., perm]), k


@BUILDS
@pytest.mark.parametrize("name", sorted(hc.WHOLE_BATCHES))
def test_mixed_batch_against_oracle(name, scalar):
    """The whole-solve columns of a mixed batch against the IPOPT oracle log directly, at OPTIONS["whole"]."""
    cases = hc.WHOLE_BATCHES[name]
    _batch, o = _mixed(cases, scalar, options="whole")
    checked = 0
    for i, case in enumerate(cases):
        if G.CASES[case]["kind"] == "whole":
            hc.check_against_oracle(case, hc.column(o, i), ("scalar" if scalar else "wave") + f" mixed[{i}]")
            checked += 1
    assert checked == {"kin": 2, "blend_par": 1}[name]


@BUILDS
def test_out_of_range_horizons_are_not_solved(scalar):
    """Horizons [0, 17, 64, -3] under cfg.N = 63: instances 0, 2, 3 fail without being solved, instance 1 is bitwise
    its uniform solve.  The buffers are pre-filled with a sentinel and followed by a guard band: every element of
    the four columns is written by its own instance (NaN for the three), so no sentinel is left inside, instance
    1's finite values are exactly its own rows, and nothing is written behind the arrays (a horizon of 64 used as
    a row index would land there or in a neighbouring row)."""
    cases = ["kin_N17"] * 4
    hz = np.array([0, 17, 64, -3], np.int32)
    batch = hc.mixed_inputs(cases)
    duals = _duals(cases, scalar)
    o = hc.host_solve(_config(cases, hc.NL), batch, hz, scalar=scalar, duals=duals, prefill=hc.SENTINEL, guard=256)
    for i in (0, 2, 3):
        hc.assert_not_solved(hc.column(o, i), f"instance {i}")
    hc.assert_column_is_uniform_solve(hc.column(o, 1), _uniform(cases, 1, batch, scalar), 17, "instance 1")
    want = {"X": 6 * 18, "U": 2 * 17, "S": 18, "eC": 17, "eL": 17, "obj": 1, "kkt": 1, "constr_viol": 1}
    if duals:
        want["lam_g"] = 13 * 17 + 9  # (state0 carries both controls: no NaN row inside)
    for k, n in want.items():
        assert int(np.isfinite(o[k]).sum()) == n == int(np.isfinite(o[k][..., 1]).sum()), k
        assert not (o[k] == hc.SENTINEL).any(), k
    for k, tail in o["guard"].items():
        assert (tail == (hc.SENTINEL if tail.dtype.kind == "f" else -1)).all(), k


@BUILDS
@pytest.mark.parametrize("case", ["kin_N17", "dyn_lane_N17", "blend_N16_par"])
def test_null_horizon_is_the_existing_entry_point(case, scalar):
    cases = [case]
    N = G.CASES[case]["N"]
    batch = hc.mixed_inputs(cases)
    duals = _duals(cases, scalar)
    new = hc.host_solve(_config(cases, N), batch, None, scalar=scalar, duals=duals)
    old = ht.solve(_config(cases, N), batch, nthreads=1, scalar=scalar, duals=duals)
    for k, v in old.items():
        assert hc.bit_equal(new[k], v), k
    assert old["iters"][0] > 0
