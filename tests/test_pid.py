"""The PID agent (csrc/mr_pid.h, mpcracing/pid.py) on the host build of the source.

* teacher-forced: mrh_pid_control and tests/pid_ref.py on every tick of the reference's own drives
  (tests/golden/pid_golden.npz: agent_pid.Agent.run_step driving the reference's models/ plant on t4), every
  output within rtol = atol = 1e-12, the steer against the reference's clipped to [-1, 1];
* free-running: the host drive against pid_ref + oracle.plant over 200 ticks on Shanghai from s0 = 1500 and
  2600 with the three plants, every row within rtol = atol = 1e-6;
* bitwise: fused drive = iterated one-tick entry + plant step, 40 ticks = 25 + 15, a vehicle alone = in a
  batch of 70, shared gains / parameters = n copies, any row subset = those rows of the full log;
* the drive's log rolled out again by plant_rollout_errors: errors exactly 0;
* edges: steer saturation, command ranges, kappa = 0, a NaN gain, a NaN start progress, every argument check;
* the pdGA fitness against the ga.segment_times formula, and the steps.csv round trip.
"""
import numpy as np
import pytest

import pid_cases as pc
import pid_twin
import track_twin
from mpcracing import ga, pid, rollout

KW = dict(host_twin=True)


def test_default_gains():
    pc.check_defaults(KW, pid_twin.gains_default)


@pytest.mark.parametrize("drive", pc.DRIVES)
def test_teacher_forced_host_twin_matches_reference(drive):
    pc.check_teacher_forced(drive, KW)


@pytest.mark.parametrize("drive", pc.DRIVES)
def test_teacher_forced_checker_matches_reference(drive):
    pc.check_ref_teacher_forced(drive)


@pytest.mark.parametrize("model", pc.MODELS)
def test_free_running_matches_checker(model):
    pc.check_free_running(model, KW)


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("model", pc.MODELS)
def test_fused_drive_is_iterated_ticks_bitwise(model, shared):
    pc.check_fused_equals_stepwise(model, shared, KW)


def test_raw_entries_match_the_package():
    """the helper's direct calls of mrh_pid_control / mrh_pid_drive and mrh_plant_step_params, iterated"""
    x0, s0, g, q = pc.batch()
    tr = track_twin.HostTrack(pc.G, pc.SHANGHAI, rows=0)
    mem = np.zeros((4, pc.N))
    mem[0], mem[3] = s0, np.nan
    rc, log, state, memT, done = pid_twin.drive(tr, 2, x0, mem, g, q, 10, pc.DT)
    assert rc == 0 and np.all(done == 10)
    x, m = x0.copy(), mem.copy()
    for t in range(10):
        rc, out, m = pid_twin.control(tr, x, m, g, pc.DT)
        assert rc == 0
        assert pc.same(log[:6, t], x) and pc.same(log[6, t], out[7]) and pc.same(log[7:, t], out[:7])
        x = rollout.plant_step(x, np.stack([out[2] - out[4], out[3]]), pc.DT, "blend", q, **KW)
    assert pc.same(state, x) and pc.same(memT, m)
    whole = pc.run(KW, "blend", ticks=10)
    assert all(pc.same(whole.rows[k], log[j]) for j, k in enumerate(pid.LOG_ROWS))


def test_continuation_is_bitwise():
    pc.check_continuation(KW)


def test_vehicle_alone_equals_vehicle_in_batch():
    pc.check_alone_equals_batch(KW)


def test_shared_gains_and_parameters_equal_copies():
    pc.check_shared_equals_copies(KW)


def test_row_subsets_equal_rows_of_the_full_log():
    pc.check_mask_subsets(KW)


def test_drive_log_rolls_out_exactly():
    pc.check_exact_rollouts(KW)


def test_steer_saturates_at_one():
    pc.check_steer_saturates(KW)


def test_throttle_and_brake_ranges():
    pc.check_command_ranges(KW)


def test_zero_curvature_gives_the_speed_cap():
    pc.check_straight_track(KW)


def test_nan_gain_stops_its_vehicle_only():
    pc.check_nan_gain_stops_one_vehicle(KW)


def test_nan_start_progress_projects_globally():
    pc.check_global_first_projection(KW)


def test_argument_checks():
    x0, s0, g, q = pc.batch()
    tr = track_twin.HostTrack(pc.G, pc.SHANGHAI, rows=0)
    n = 3
    x, g3, q3 = x0[:, :n], g[:n], q[:n]
    mem = np.zeros((4, n))
    mem[0], mem[3] = s0[:n], np.nan
    ok = dict(model=2, state=x, mem=mem, gains=g3, params=q3, T=2, dt=pc.DT, mask=1 << 7)
    assert pid_twin.drive(tr, **ok)[0] == 0
    bad = [dict(T=0), dict(T=-1), dict(T=4097), dict(dt=0.0), dict(dt=-0.05), dict(dt=np.nan), dict(dt=np.inf),
           dict(G=2), dict(G=0), dict(P=2), dict(P=0), dict(model=3), dict(model=-1), dict(mask=1 << 14),
           dict(mask=(1 << 14) | 1), dict(mask=1 << 31), dict(log=None), dict(mask=0, log=np.zeros((1, 2, n)))]
    for change in bad:
        rc, _, state, m, done = pid_twin.drive(tr, **{**ok, **change})
        assert rc == -1, change
        assert pc.same(state, x) and pc.same(m, mem) and np.all(done == -1), change  # nothing was written
    # the cap itself is accepted (NaN gains: every vehicle stops at tick 0 and the loop ends there)
    rc, _, _, _, done = pid_twin.drive(tr, **{**ok, "T": 4096, "mask": 0, "log": None, "gains": g3 * np.nan})
    assert rc == 0 and np.all(done == 0)
    for change in (dict(dt=0.0), dict(dt=np.nan), dict(gains=g[:2])):
        args = {**dict(state=x, mem=mem, gains=g3, dt=pc.DT), **change}
        assert pid_twin.control(tr, **args)[0] == -1, change
    with pytest.raises(ValueError, match="unknown row"):
        pid.drive(pc.track(pc.SHANGHAI, KW), x, 2, rows=["speed"], **KW)
    with pytest.raises(ValueError, match="gains: expected"):
        pid.drive(pc.track(pc.SHANGHAI, KW), x, 2, gains=g[:2], **KW)
    with pytest.raises(ValueError, match="kept no"):
        pid.drive(pc.track(pc.SHANGHAI, KW), x, 2, rows=["progress"], progress0=s0[:n], **KW).log(0)


def test_long_drive_is_chunked(monkeypatch):
    """more ticks than one call takes: the chunks continue each other bit for bit"""
    monkeypatch.setattr(pid, "T_MAX", 16)
    chunked = pc.run(KW, "dyn", n=slice(0, 4))
    monkeypatch.undo()
    pc.result_same(pc.run(KW, "dyn", n=slice(0, 4)), chunked)


def test_segment_times_helper_keeps_segment_times():
    import torch
    rng = np.random.default_rng(3)
    prog = np.cumsum(rng.uniform(0.2, 1.0, (50, 4)), 0) + np.array([0.0, 10.0, 1890.0, 5.0])
    L = 1899.0
    s0, s1 = np.array([0.0, 10.0, 1890.0, 5.0]), np.array([20.0, 25.0, 8.0, 500.0])
    a = ga.segment_times([{"progress": torch.from_numpy(np.mod(r, L))} for r in prog], s0, s1, L, 0.05)
    assert pc.same(a, ga.crossing_times(np.mod(prog, L), s0, s1, L, 0.05))
    assert np.isfinite(a[:3]).all() and np.isinf(a[3])


def test_evaluate_gains_is_the_segment_time_formula():
    pc.check_evaluate_gains(KW)


def test_steps_csv_round_trip(tmp_path):
    pc.check_csv_round_trip(KW, tmp_path)
