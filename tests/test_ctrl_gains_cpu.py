"""Per-env PID gains of the control loop, CPU tier: the model tests/test_ctrl_gains.py holds the kernels to
(tests/ctrl_pid_model.py) is checked against the project's oracle and against the numbers that motivate the feature, the numpy
restatement of the rule against the model's controller, and the fixtures of the GPU tests are qualified on the model alone --
they must be able to tell a kernel that drops a gain, or keeps the last error across a reset, from a right one."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctrl_pid_model as pm
import ctrl_tiers as ct
from ctrl_tiers import PID
from test_control_loop import STREAMS, model_streams
from util import private_segments


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


# ---- the model -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plant", [None, "dense"])
def test_default_gains_give_the_oracle_snapshot_for_snapshot(plant):
    K, seed, start, period = 70, 1, 20, 10
    dev, dur, want = model_streams(plant, K, seed, start, period)
    dev2, dur2, got, _ = ct.step_streams(PID, plant, K, seed, start, period, gains=(pm.DEFAULT_GAINS,))
    assert (dev == dev2).all() and (dur == dur2).all()
    for k in range(K):
        for f, w in want[k].items():
            g = got[k][f][0]
            same = bits(g) == bits(w) if w.dtype == np.float64 else g == w
            assert np.all(same), (plant, k, f)
    assert (got[-1]["last_error"] != 0.0).any() and (got[-1]["commands"] > 0).all()     # the rule did run


def cost_of(gains, schedule, steps=120):
    m = pm.PidControlLoopModel(gains=gains)
    cost = 0.0
    for k in range(steps):
        d, u = schedule[k % len(schedule)]
        cost = cost + math.fabs(m.step(d, u)[3]["Sensor angle"])
    return cost


def test_the_gain_decides_more_than_the_schedule_does():
    """The table that motivates the feature, default plant, 120 steps, sum of |angle in degrees|: pinned to 4 significant
    digits on the alternating schedule, and the orderings the README draws from the other rows."""
    alt = [(0, 19), (1, 19)]
    for kp, want in ((1.0, "1.098e+09"), (0.1, "77.44"), (0.05, "65.58")):
        c = cost_of((kp, 0.0, 0.0), alt)
        assert "%.4g" % c == want, (kp, c)
    assert "%.3g" % cost_of((0.05, 0.01, 0.0), alt) == "60.1"                            # ki moves the best point again
    short = [(0, 8), (1, 8)]
    assert cost_of((0.1, 0.0, 0.0), short) < cost_of((0.05, 0.0, 0.0), short)           # the best gain moves with the schedule
    assert cost_of((57.0, 26.0, 12.0), alt) > 1e30                                       # the reference author's other gains


def test_numpy_rule_agrees_with_the_models_controller():
    rng = np.random.default_rng(7)
    n = 120
    gains = rng.normal(0.0, 2.0, (n, 3))
    ang = rng.normal(0.0, 40.0, n)
    last = np.abs(rng.normal(0.0, 40.0, n))
    ang[:6] = [0.0, -0.0, -1e-300, 1e-300, -90.0, 90.0]
    gains[6:9] = [[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [57.0, 26.0, 12.0]]
    last[9:12] = 0.0
    assert (ang < 0).sum() > 20 and (ang > 0).sum() > 20
    from gymwipe_amd import actions
    value, send, new_last = actions.ctrl_pid_numpy(gains, ang, last)
    value2, send2, new_last2 = actions.ctrl_pid_numpy(gains, ang, new_last)             # the tick after, same angle
    for i in range(n):
        m = pm.PidControlLoopModel(start=0, period=1, gains=gains[i], keep_last_err=last[i])
        m.angle_deg = float(ang[i])
        m.step(0, 0)                                     # an empty window: two control ticks, nothing reaches the controller
        assert m.tick == 2 and bits(m.angle_deg) == bits(ang[i]), i
        sent = [pkt.payload.payload.value for pkt in m.devs[1].mac.queue]
        assert len(sent) == m.n_cmd == (2 if send[i] else 0), i
        assert bool(send[i]) == bool(send2[i]) == (ang[i] != 0.0)
        if send[i]:
            assert bits(sent[0]) == bits(value[i]) and bits(sent[1]) == bits(value2[i]), i
        assert bits(m.last_err) == bits(new_last2[i]) == bits(new_last[i]) == bits(math.fabs(ang[i])), i
    one = actions.ctrl_pid_numpy((1.0, 0.0, 0.0), ang, last)                            # one set is broadcast; the default commands -ang
    assert (bits(one[0][ang != 0]) == bits(-ang[ang != 0])).all()


def test_make_ctrl_gains_lays_sets_across_envs():
    from gymwipe_amd import actions
    sets = pm.GAIN_SETS
    g = actions.make_ctrl_gains(sets, 512)
    assert g.shape == (512, 3) and g.dtype == np.float64 and (g == np.array(sets)[np.arange(512) // 64]).all()
    g = actions.make_ctrl_gains(sets, pm.N_FUSED, pm.PER_SET)
    assert (g == np.array(sets)[pm.fused_layout()[1]]).all()
    assert len({tuple(r) for r in g[:64].tolist()}) == 4                                 # one 64-env block holds several sets
    assert (actions.make_ctrl_gains([(2.0, 1.0, 0.5)], 3) == [2.0, 1.0, 0.5]).all()
    for bad in (lambda: actions.make_ctrl_gains(sets, 100), lambda: actions.make_ctrl_gains(sets, 512, 48),
                lambda: actions.make_ctrl_gains(sets, 512, 0), lambda: actions.make_ctrl_gains([(1.0, 0.0)], 8),
                lambda: actions.make_ctrl_gains([], 8)):
        with pytest.raises(ValueError):
            bad()


# ---- the fixtures of the GPU tests ------------------------------------------------------------------------------------------------------
def test_step_fixture_is_bounded_and_commands_of_both_signs_are_delivered():
    steps = ct.step_streams(PID, None, 70, 1, 20, 10).steps
    x = np.array([w["x"] for w in steps])
    ang = np.array([w["ang"] for w in steps])
    assert np.isfinite(x).all() and np.isfinite(ang).all() and np.abs(ang).max() < 2000.0, np.abs(ang).max()
    u = np.array([w["u"] for w in steps])                # [K][G][8]
    got = np.array([w["received"][..., 1] for w in steps])
    delivered = np.diff(got, axis=0, prepend=0) > 0      # the actuator took a command in this step: u is a command's value
    assert (u[delivered] > 0).sum() > 50 and (u[delivered] < 0).sum() > 50
    last = steps[-1]
    assert (last["commands"] > 0).all() and (last["last_error"] != 0).all()
    assert len({last["x"][g, s].tobytes() for g in range(pm.G) for s in range(STREAMS)}) == pm.G * STREAMS    # every pair differs


@pytest.mark.parametrize("max_steps", [pm.MAX_STEPS, pm.SHORT_MAX_STEPS])
def test_fused_fixtures_are_bounded_and_end_by_both_causes(max_steps):
    sch, fb, ep = ct.schedule_streams(PID, max_steps), ct.feedback_streams(PID, max_steps), ct.episode_streams(PID, max_steps)
    tally, fb_tally = sch.tally, fb.tally
    for what, a, e, f in (("schedules", sch.ang, sch.ended, sch.final), ("feedback", fb.rows["angle"], fb.rows["ended"], fb.final),
                          ("staged", ep.ang, ep.ended, ep.final)):
        assert np.isfinite(a).all() and np.abs(a).max() < 2000.0, (what, np.abs(a).max())
        assert np.isfinite(f["x"]).all() and np.isfinite(f["last_error"]).all(), what
        assert ((e & 1) != 0).sum() >= 20 and ((e & 2) != 0).sum() >= 20, what           # the step limit, and the failure angle
        assert (f["u"] > 0).any() and (f["u"] < 0).any(), what                           # commands of both signs were applied
    assert (tally[..., 0] > 0).all() and (fb_tally[..., 0] > 0).all()


def _models():
    """(p, gain set index, b) of the schedule case, sets with the gain in question first."""
    return [(p, g, b) for g in range(pm.G) for p in range(pm.P) for b in range(2)]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_each_gain_alone_changes_where_the_fixtures_end(which):
    """A kernel that ignored kp, ki or kd would be caught: zeroing that one gain moves the final x of at least 3 (gain set,
    stream) pairs of the schedule case."""
    final = ct.schedule_streams(PID, pm.MAX_STEPS).final
    moved = 0
    for p, g, b in _models():
        gains = list(pm.GAIN_SETS[g])
        if gains[which] == 0.0:
            continue
        gains[which] = 0.0
        _, _, _, env = ct.run_schedule(PID, p, g, b, pm.MAX_STEPS, gains=tuple(gains))
        moved += bits(env.state()["x"]).tolist() != bits(final["x"][p, g, b]).tolist()
        if moved >= 3:
            break
    assert moved >= 3, (which, moved)


@pytest.mark.parametrize("case", ["schedules", "staged"])
def test_a_reset_that_kept_the_last_error_would_be_caught(case):
    moved = 0
    if case == "schedules":
        final = ct.schedule_streams(PID, pm.MAX_STEPS).final
        for p, g, b in _models():
            if pm.GAIN_SETS[g][1] == 0.0 and pm.GAIN_SETS[g][2] == 0.0:
                continue                                 # kp alone never reads the last error
            _, _, _, env = ct.run_schedule(PID, p, g, b, pm.MAX_STEPS, keep_last=True)
            moved += bits(env.state()["x"]).tolist() != bits(final["x"][p, g, b]).tolist()
            if moved >= 3:
                break
    else:
        final = ct.episode_streams(PID, pm.SHORT_MAX_STEPS).final
        where = {(g, pm.fused_stream(p, g, b)): (p, b) for p, g, b in _models()}      # the staged case is laid out by (set, stream)
        for g in range(pm.G):
            if pm.GAIN_SETS[g][1] == 0.0 and pm.GAIN_SETS[g][2] == 0.0:
                continue
            for s in range(STREAMS):
                p, b = where[g, s]
                _, env = ct.run_episodes(PID, p, g, b, pm.SHORT_MAX_STEPS, keep_last=True)
                moved += bits(env.state()["x"]).tolist() != bits(final["x"][g, s]).tolist()
                if moved >= 3:
                    break
            if moved >= 3:
                break
    assert moved >= 3, (case, moved)


# ---- the PID instantiations use no scratch memory -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("source,kernels", [("ctrl_step.hip", ("ctrl_step_kernel", "ctrl_step_pid_kernel")),
                                            ("ctrl_rollout_feedback.hip", ("ctrl_rollout_fb_pid_kernel", "ctrl_rollout_fb_rows_pid_kernel"))])
def test_the_pid_kernels_use_no_scratch_memory(tmp_path, source, kernels):
    """Every kernel of the two files that hold the PID instantiations beside ctrl_rollout.hip has a private segment of 0 bytes
    (ctrl_rollout.hip's, the PID instantiations included, are held to it by tests/test_ctrl_rollout_cpu.py)."""
    found = private_segments(tmp_path, source)
    for want in kernels:
        assert any(want in n for n in found), (want, sorted(found))
    assert all(v == 0 for v in found.values()), found
