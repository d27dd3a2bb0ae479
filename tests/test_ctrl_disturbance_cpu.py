"""Seeded plant disturbances of the control loop, CPU tier: the numpy restatement of the draw against the pure-Python one the
model uses (tests/ctrl_dist_model.py), the draw's law, the model at zero weights against the undisturbed one, the numbers that
motivate the feature, ``actions.make_ctrl_disturbance``, and the fixtures of the GPU tests qualified on the model alone -- they
must be able to tell a kernel that drops a weight, or restarts the count at a reset, from a right one."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctrl_dist_model as dm
import ctrl_pid_model as pm
import ctrl_tiers as ct
from ctrl_fixtures import STREAMS
from ctrl_tiers import DIST, PID
from util import private_segments


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


# ---- the draw ------------------------------------------------------------------------------------------------------------------------------
KEYS = (0, 1, 2, 0x8000000000000000, 0xFFFFFFFFFFFFFFFF, 0x9E3779B97F4A7C15, 0xC0FFEE0DDF00D5EE, 0x8000000000000001)
COUNTS = (0, 1, 2, 63, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 12345, 2 ** 63, 2 ** 64 - 1)


def test_numpy_draw_equals_the_pure_python_restatement():
    from gymwipe_amd import actions
    key = np.array(KEYS, np.uint64)[:, None]
    n = np.array(COUNTS, np.uint64)[None, :]
    got = actions.ctrl_noise_numpy(key, n)
    assert got.shape == (len(KEYS), len(COUNTS)) and got.dtype == np.float64
    for i, k in enumerate(KEYS):
        for j, c in enumerate(COUNTS):
            assert bits(got[i, j]) == bits(dm.noise(k, c)), (hex(k), c)
    assert len(set(got.ravel().tolist())) > 0.9 * got.size       # (a few pairs meet by design: 2^63 times an odd number is 2^63)
    assert actions.ctrl_noise_numpy(np.uint64(7), np.uint64(9)).shape == ()     # scalars in, a scalar out
    # two values written out by hand from the rule, so that both restatements cannot be wrong together: key 0, n 0 is the
    # mixer's output for z = 0x9E3779B97F4A7C15, whose top 32 bits are 0xE220A839 (splitmix64's first output for state 0)
    assert dm.noise(0, 0) == float(0xE220A839 - 2 ** 32) * 2.0 ** -31
    assert dm.noise(0x9E3779B97F4A7C15 ^ 0xD1B54A32D192ED03, 1) == float(0x6E789E6A) * 2.0 ** -31   # z = 2 * 0x9E37...: the second


def test_every_draw_lies_in_the_half_open_interval_and_on_the_grid():
    from gymwipe_amd import actions
    w = actions.ctrl_noise_numpy(np.array(KEYS, np.uint64)[:, None], np.arange(20000, dtype=np.uint64)[None, :])
    assert (w >= -1.0).all() and (w < 1.0).all()
    scaled = w * 2.0 ** 31
    assert (scaled == np.rint(scaled)).all()
    assert (w < 0).any() and (w > 0).any()


@pytest.mark.parametrize("key", [1, 0xC0FFEE0DDF00D5EE])
def test_mean_and_variance_of_one_keys_draws_are_the_uniform_laws(key):
    """10^5 draws of one key.  For U uniform on [-1, 1): E U = 0, Var U = 1/3, E U^4 = 1/5, so the mean of M draws has standard
    error sqrt(1 / (3 M)) and the mean of their squares sqrt((1/5 - 1/9) / M).  (The grid of 2^-31 moves these by 2^-31 at most.)"""
    from gymwipe_amd import actions
    M = 100000
    w = actions.ctrl_noise_numpy(np.uint64(key), np.arange(M, dtype=np.uint64))
    se_mean = math.sqrt(1.0 / (3.0 * M))
    se_var = math.sqrt((1.0 / 5.0 - 1.0 / 9.0) / M)
    print("mean %.6f (se %.6f)  mean square %.6f (1/3 = %.6f, se %.6f)" % (w.mean(), se_mean, (w * w).mean(), 1 / 3, se_var))
    assert abs(w.mean()) < 5.0 * se_mean
    assert abs((w * w).mean() - 1.0 / 3.0) < 5.0 * se_var


# ---- the model -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plant", [None, "dense"])
def test_zero_weights_give_the_undisturbed_model_snapshot_for_snapshot(plant):
    """Weight set 0 of the step fixture is (0, 0, 0, 0) under gains (1, 0, 0): the PID model, and through it the oracle.  The
    rule as written may turn a -0.0 of the plant into +0.0; the fixture holds no -0.0, which is asserted, so bits are compared."""
    K, seed, start, period = 70, 1, 20, 10
    assert dm.G_SETS[0] == (0.0, 0.0, 0.0, 0.0) and pm.GAIN_SETS[0] == pm.DEFAULT_GAINS
    dev, dur, want, _ = ct.step_streams(PID, plant, K, seed, start, period)
    dev2, dur2, got, _ = ct.step_streams(DIST, plant, K, seed, start, period)
    assert (dev == dev2).all() and (dur == dur2).all()
    for k in range(K):
        for f, w in want[k].items():
            g = got[k][f][0]
            same = bits(g) == bits(w[0]) if w.dtype == np.float64 else g == w[0]
            assert np.all(same), (plant, k, f)
        assert not np.signbit(want[k]["x"][0][want[k]["x"][0] == 0.0]).any(), k
        assert (got[k]["noise_count"] == got[k]["substeps"]).all()              # nothing resets here: one draw per substep
    assert (got[-1]["noise_count"] > 500).all()


PREMISE_SCHEDULES = ([(0, 19), (1, 19)], [(0, 8), (1, 8)], [(0, 3), (1, 3)], [(0, 19), (1, 5)])
PREMISE_KEYS = (1, 2, 3, 4)


def mean_abs_angle(schedule, a, key, steps=120):
    """Time-weighted mean |angle| in degrees of the default model from x0 = 0 under gains (0.1, 0, 0), g = (0, 0, 0, a)."""
    m = pm.PidControlLoopModel(x0=(0.0, 0.0, 0.0, 0.0), gains=(0.1, 0.0, 0.0))
    if a is not None:
        dm.disturb(m, (0.0, 0.0, 0.0, a), key)
    area = elapsed = 0.0
    for k in range(steps):
        d, u = schedule[k % len(schedule)]
        before = m.sim.now
        deg = m.step(d, u)[3]["Sensor angle"]
        dt = m.sim.now - before
        area, elapsed = area + math.fabs(deg) * dt, elapsed + dt
    return area / elapsed


def test_the_disturbance_changes_which_schedule_wins_and_comparisons_must_be_paired():
    """The table that motivates the feature, pinned to 3 significant digits, and the three things drawn from it."""
    calm = [mean_abs_angle(s, None, 0) for s in PREMISE_SCHEDULES]
    noisy = np.array([[mean_abs_angle(s, 0.01, k) for k in PREMISE_KEYS] for s in PREMISE_SCHEDULES])
    assert ["%.3g" % v for v in calm] == ["0.0341", "0.0709", "0.0993", "0.15"], calm
    assert [["%.3g" % v for v in row] for row in noisy] == [["0.814", "0.919", "0.952", "0.963"], ["0.602", "0.811", "0.958", "0.96"],
                                                           ["0.677", "0.315", "0.784", "0.408"], ["1.44", "2.44", "2.42", "2.18"]], noisy
    means = noisy.mean(1)
    assert np.argsort(calm).tolist() == [0, 1, 2, 3] and np.argsort(means).tolist() == [2, 1, 0, 3]      # the ranking changes
    spread = noisy[2].max() - noisy[2].min()                                    # one schedule over four noise sequences ...
    assert spread > abs(means[0] - means[1]) and spread > abs(means[2] - means[1])        # ... against the gaps between means
    paired = noisy[2] - noisy[0]                                                # the same key for both candidates:
    assert (paired < 0).all()                                                   # every sequence says the same
    assert bits(mean_abs_angle(PREMISE_SCHEDULES[0], 0.0, 1)) == bits(calm[0])  # a = 0 on a disturbed plant is the calm row


# ---- make_ctrl_disturbance -----------------------------------------------------------------------------------------------------------------
def test_make_ctrl_disturbance_lays_sets_and_keys_across_envs():
    from gymwipe_amd import actions
    g, key = actions.make_ctrl_disturbance(dm.G_SETS, 512)
    assert g.shape == (512, 4) and g.dtype == np.float64 and key.shape == (512,) and key.dtype == np.uint64
    assert (g == dm.g_array()[np.arange(512) // 64]).all()
    assert key.tolist() == [dm.key_of(0, e) for e in range(512)]                # the streams default: arange(N), seed 0
    g, key = actions.make_ctrl_disturbance(dm.G_SETS, pm.N_FUSED, seed=dm.SEED, envs_per_set=pm.PER_SET)
    assert (g == dm.g_array()[pm.fused_layout()[1]]).all()
    assert key.tolist() == [dm.key_of(dm.SEED64, e) for e in range(512)] and len(set(key.tolist())) == 512
    g, key = actions.make_ctrl_disturbance((0.0, 0.0, 0.0, 0.01), 6, seed=5, streams=np.array([0, 1, 2 ** 63, 2 ** 64 - 1, 7, 7], np.uint64))
    assert g.shape == (6, 4) and (g == [0.0, 0.0, 0.0, 0.01]).all()             # one vector is broadcast
    assert key.tolist() == [5, dm.key_of(5, 1), dm.key_of(5, 2 ** 63), dm.key_of(5, 2 ** 64 - 1), dm.key_of(5, 7), dm.key_of(5, 7)]
    assert actions.make_ctrl_disturbance(np.zeros(4), 2, seed=5, streams=np.array([-1, 3]))[1].tolist() == [dm.key_of(5, 2 ** 64 - 1), dm.key_of(5, 3)]
    # common random numbers: 4 policies of 128 envs, env j of every policy on stream j
    _, key = actions.make_ctrl_disturbance(np.zeros(4), 512, seed=9, streams=np.arange(512) % 128)
    assert (key.reshape(4, 128) == key[:128]).all() and len(set(key[:128].tolist())) == 128
    p, gi, b, _ = pm.fused_layout()                                             # the fused fixture's keys through the helper
    _, key = actions.make_ctrl_disturbance(np.zeros(4), 512, seed=dm.SEED, streams=(p * dm.G + gi) * 2 + b)
    assert (key == ct.fused_keys(dm.SEED64)).all()
    for bad in (lambda: actions.make_ctrl_disturbance(dm.G_SETS, 100), lambda: actions.make_ctrl_disturbance(dm.G_SETS, 512, envs_per_set=48),
                lambda: actions.make_ctrl_disturbance(dm.G_SETS, 512, envs_per_set=0), lambda: actions.make_ctrl_disturbance([(1.0, 0.0, 0.0)], 8),
                lambda: actions.make_ctrl_disturbance([], 8), lambda: actions.make_ctrl_disturbance(np.zeros(4), 8, streams=np.arange(7)),
                lambda: actions.make_ctrl_disturbance(np.zeros(4), 8, streams=np.zeros(8))):
        with pytest.raises(ValueError):
            bad()


# ---- the fixtures of the GPU tests ---------------------------------------------------------------------------------------------------------
def test_step_fixture_is_bounded_and_every_pair_walks_its_own_way():
    steps = ct.step_streams(DIST, None, 70, 1, 20, 10).steps
    x = np.array([w["x"] for w in steps])
    ang = np.array([w["ang"] for w in steps])
    assert np.isfinite(x).all() and np.isfinite(ang).all() and np.abs(ang).max() < 2000.0, np.abs(ang).max()      # nothing the
    last = steps[-1]                                                            # int32 observation would have to clamp
    assert (last["commands"] > 0).all() and (last["noise_count"] == last["substeps"]).all()
    assert len({last["x"][g, s].tobytes() for g in range(dm.G) for s in range(STREAMS)}) == dm.G * STREAMS
    calm = ct.step_streams(PID, None, 70, 1, 20, 10).steps
    assert (bits(last["x"][1:]) != bits(calm[-1]["x"][1:])).any(axis=-1).all()  # every disturbed pair left the calm trajectory


def test_fused_fixtures_are_bounded_and_end_by_both_causes_under_the_noise():
    sch, fb, ep = ct.schedule_streams(DIST, dm.MAX_STEPS), ct.feedback_streams(DIST, dm.MAX_STEPS), ct.episode_streams(DIST, dm.SHORT_MAX_STEPS)
    tally, fb_tally = sch.tally, fb.tally
    for what, a, e, f in (("schedules", sch.ang, sch.ended, sch.final), ("feedback", fb.rows["angle"], fb.rows["ended"], fb.final),
                          ("staged", ep.ang, ep.ended, ep.final)):
        assert np.isfinite(a).all() and np.abs(a).max() < 2000.0, (what, np.abs(a).max())
        assert np.isfinite(f["x"]).all() and np.isfinite(f["last_error"]).all(), what
        assert ((e & 1) != 0).sum() >= 20 and ((e & 2) != 0).sum() >= 20, what           # the step limit, and the failure angle
        assert (f["noise_count"] > f["substeps"]).sum() >= 32, what             # the count ran on across resets
        assert (f["disturbance"] == dm.g_array()[None, :, None, :]).all() and len(set(f["noise_key"].ravel().tolist())) == 64
    assert (tally[..., 0] > 0).all() and (fb_tally[..., 0] > 0).all()


def test_the_noise_changes_actions_the_feedback_fixture_takes():
    rows = ct.feedback_streams(DIST, dm.MAX_STEPS).rows
    calm = ct.feedback_streams(DIST, dm.MAX_STEPS, g=(0.0, 0.0, 0.0, 0.0)).rows       # the same models with all weights 0
    moved = (rows["device"] != calm["device"]) | (rows["duration"] != calm["duration"])
    assert moved[:, :, 1:].any() and not moved[:, :, 0].any()                   # (weight set 0 is the calm one)
    assert moved.reshape(dm.STEPS, -1).any(0).sum() >= 8, moved.sum()           # in at least 8 of the 56 disturbed models


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_each_weight_alone_changes_where_the_fixtures_end(which):
    """A kernel that ignored one component of g would be caught: zeroing it moves the final x of at least 3 models of the
    schedule case."""
    final = ct.schedule_streams(DIST, dm.MAX_STEPS).final
    moved = 0
    for gi in range(dm.G):
        g = list(dm.G_SETS[gi])
        if g[which] == 0.0:
            continue
        g[which] = 0.0
        for p in range(dm.P):
            _, _, _, env = ct.run_schedule(DIST, p, gi, 0, dm.MAX_STEPS, g=tuple(g))
            moved += bits(env.state()["x"]).tolist() != bits(final["x"][p, gi, 0]).tolist()
        if moved >= 3:
            break
    assert moved >= 3, (which, moved)


@pytest.mark.parametrize("case", ["schedules", "staged"])
def test_a_reset_that_restarted_the_count_would_be_caught(case):
    moved = 0
    final = ct.schedule_streams(DIST, dm.MAX_STEPS).final if case == "schedules" else ct.episode_streams(DIST, dm.SHORT_MAX_STEPS).final
    for gi in range(1, dm.G):
        for p in range(dm.P):
            if case == "schedules":
                env = ct.run_schedule(DIST, p, gi, 1, dm.MAX_STEPS, restart_n=True)[3]
            else:
                env = ct.run_episodes(DIST, p, gi, 1, dm.SHORT_MAX_STEPS, restart_n=True)[1]
            st = env.state()
            assert st["noise_count"] <= st["substeps"]
            moved += bits(st["x"]).tolist() != bits(final["x"][p, gi, 1]).tolist()
        if moved >= 3:
            break
    assert moved >= 3, (case, moved)


# ---- the disturbance instantiations use no scratch memory -----------------------------------------------------------------------------------
_VARIANTS = ("", "_pid", "_dist", "_loss")                                # of every step and rollout kernel: default, + gains, + disturbance, + loss


@pytest.mark.parametrize("source,kernels", [
    ("ctrl_step.hip", tuple("ctrl_step%s_kernel" % v for v in _VARIANTS) + ("ctrl_init_kernel",)),
    ("ctrl_rollout.hip", tuple("ctrl_rollout%s%s_kernel" % (shape, v) for shape in ("", "_sched") for v in _VARIANTS)
     + ("ctrl_fill_initial_kernel", "ctrl_set_initial_kernel", "ctrl_set_gains_kernel", "ctrl_set_disturbance_kernel",
        "ctrl_set_loss_kernel", "ctrl_reset_pid_kernel", "ctrl_reset_kernel")),
    ("ctrl_rollout_feedback.hip", tuple("ctrl_rollout_fb%s%s_kernel" % (shape, v) for shape in ("", "_rows") for v in _VARIANTS))])
def test_the_disturbance_kernels_use_no_scratch_memory(tmp_path, source, kernels):
    """Every kernel of the three files that hold the control loop -- the disturbance instantiations and, since they share their
    files, every other variant (the loss instantiations included) and the small kernels -- has a private segment of 0 bytes,
    compiled as the product build compiles them; and the files hold exactly the kernels listed."""
    found = private_segments(tmp_path, source)
    assert len(found) == len(kernels)
    for want in kernels:
        assert any(want in n for n in found), (want, sorted(found))
    assert all(v == 0 for v in found.values()), found
