"""Seeded plant disturbances of the control loop on the GPU (gw_ctrl_set_disturbance): the disturbance instantiations of the step
kernel and of the fused rollout kernels against the event-driven model of tests/ctrl_dist_model.py, bit for bit, over every
state field, the controller's two and the disturbance's three (``disturbance``, ``noise_key``, ``noise_count``).  A reset env is
a freshly constructed model whose plant goes on drawing where the old one stopped.  The fixtures are defined in
tests/ctrl_dist_model.py and qualified on the model alone in tests/test_ctrl_disturbance_cpu.py (every weight matters, a count
restarted at a reset would show, both ending causes occur, the noise changes actions the feedback policies take).  Every test
calls ``set_disturbance``: none passes without it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctrl_dist_model as dm
import ctrl_pid_model as pm
import test_ctrl_rollout as g
from test_control_loop import DENSE_CTRL, stream_of
from test_ctrl_rollout import ALL_FIELDS, FIELDS, T, assert_same

NEW_FIELDS = ("gains", "last_error", "disturbance", "noise_key", "noise_count")
DIST_FIELDS = ALL_FIELDS + NEW_FIELDS
MODEL_FIELDS = FIELDS + NEW_FIELDS
GAINS, WEIGHTS = pm.gains_array(), dm.g_array()


def state_of(env, fields=DIST_FIELDS):
    return {f: env.get_state(f) for f in fields}


def assert_states_equal(a, b, what, fields=DIST_FIELDS):
    for f in fields:
        assert_same(a[f], b[f], (what, f))


def step_layout(N):
    """The step cases' envs: action stream ``stream_of(e)``, weight and gain set ``(e // 8) % 8`` -- the first 64 envs are the
    64 pairs -- and the pair's own noise key."""
    from gymwipe_amd import actions
    gi, so = (np.arange(N) // 8) % dm.G, stream_of(N)
    _, key = actions.make_ctrl_disturbance(np.zeros(4), N, seed=dm.SEED, streams=gi * 8 + so)
    return gi, so, key


def step_env(N, start, period, plant=None):
    from gymwipe_amd import VecControlLoopEnv
    gi, _, key = step_layout(N)
    kw = {} if plant is None else {"A": DENSE_CTRL["A"], "B": DENSE_CTRL["B"], "x0": DENSE_CTRL["x0"], "u0": DENSE_CTRL["u0"]}
    env = VecControlLoopEnv(N, ctrl_start_tick=start, ctrl_period_ticks=period, gains=T(GAINS[gi]), **kw)
    env.set_disturbance(T(WEIGHTS[gi]), key)
    return env


def fused_env():
    """512 envs on the fused cases' layout: every env starts from its stream's X0S / U0S under its gain set, its weights and its
    model's key."""
    from gymwipe_amd import VecControlLoopEnv, actions
    _, gi, _, so = pm.fused_layout()
    env = VecControlLoopEnv(pm.N_FUSED, ctrl_start_tick=g.START, ctrl_period_ticks=g.PERIOD)
    env.set_initial_state(T(g.X0S[so]), T(g.U0S[so]))
    env.reset_envs()
    env.set_gains(actions.make_ctrl_gains(pm.GAIN_SETS, pm.N_FUSED, pm.PER_SET))
    env.set_disturbance(actions.make_ctrl_disturbance(dm.G_SETS, pm.N_FUSED, envs_per_set=pm.PER_SET)[0], dm.fused_keys())
    return env


def check_final(st, final, index, what):
    for f in MODEL_FIELDS + ("age", "cost"):
        assert_same(st[f], final[f][index], (what, f))
    assert not (st["flags"] & 3).any(), what


# ---- 1. step -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("plant", [None, "dense"])
@pytest.mark.parametrize("seed,start,period", [(1, 20, 10), (2, 0, 3), (3, 50, 1)])
def test_step_with_per_env_disturbances_matches_the_model(seed, start, period, plant):
    N, K = 70, 70                                        # one full block and a partial one
    gi, so, key = step_layout(N)
    dev, dur, steps = dm.step_streams(plant, K, seed, start, period)
    env = step_env(N, start, period, plant)
    assert_same(env.get_state("disturbance"), WEIGHTS[gi], "weights as set")
    assert_same(env.get_state("noise_key"), key, "keys as set")
    assert (env.get_state("noise_count") == 0).all()
    for k in range(K):
        obs, rew, done, info = env.step({"device": T(dev[k][so]), "duration": T(dur[k][so])})
        want = steps[k]
        got = {"obs": obs.cpu().numpy(), "rew": rew.cpu().numpy(), "ang": info["Sensor angle"].cpu().numpy()}
        got.update(state_of(env, MODEL_FIELDS))
        for f, w in want.items():
            assert_same(got[f], w[gi, so], (f, k))
        assert_same(got["noise_count"], got["substeps"], ("one draw per substep", k))
        assert not done.any()
    assert not (env.get_state("flags") & 3).any()
    assert (env.get_state("commands") > 0).all() and (env.get_state("noise_count") > 500).all()
    env.close()


# ---- 2. the fused rollouts, and K / 2 + K / 2 = K ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rollout_with_episodes_under_disturbance_matches_the_wrapper_and_splits():
    K, max_steps = dm.STEPS, dm.SHORT_MAX_STEPS
    pi, gi, bi, so = pm.fused_layout()
    dev, dur = pm.episode_actions()
    w_obs, w_rew, w_ang, w_ended, final = dm.episode_streams(max_steps)
    d, u = T(dev[:, so]), T(dur[:, so])
    env = fused_env()
    obs, rew, ended, info = env.rollout(d, u, episodes=(max_steps, dm.FAIL_DEG))
    assert_same(ended.cpu().numpy(), w_ended[:, pi, gi, bi], "ended")
    assert_same(obs.cpu().numpy(), w_obs[:, pi, gi, bi], "obs") and assert_same(rew.cpu().numpy(), w_rew[:, pi, gi, bi], "reward")
    assert_same(info["Sensor angle"].cpu().numpy(), w_ang[:, pi, gi, bi], "angle")
    st = state_of(env)
    check_final(st, final, (pi, gi, bi), "rollout")
    assert (st["noise_count"] > st["substeps"]).sum() > 256                     # resets happened, and the count ran on
    halves = fused_env()                                 # two calls of K / 2: the count is handle state, as age and cost are
    a = halves.rollout(d[:K // 2], u[:K // 2], episodes=(max_steps, dm.FAIL_DEG))
    assert (halves.get_state("noise_count") > 0).all()
    b = halves.rollout(d[K // 2:], u[K // 2:], episodes=(max_steps, dm.FAIL_DEG))
    assert_same(np.concatenate([a[3]["Sensor angle"].cpu().numpy(), b[3]["Sensor angle"].cpu().numpy()]), w_ang[:, pi, gi, bi], "halves")
    assert_states_equal(state_of(halves), st, "halves")
    env.close(), halves.close()


@pytest.mark.gpu
def test_rollout_schedules_under_disturbance_matches_the_wrapper_and_splits():
    K, max_steps = dm.STEPS, dm.MAX_STEPS
    pi, gi, bi, _ = pm.fused_layout()
    sch, w_tally, final, _, _ = dm.schedule_streams(max_steps)
    env = fused_env()
    tally, sums = env.rollout_schedules(T(sch), (max_steps, dm.FAIL_DEG), K)
    tally = tally.cpu().numpy()
    assert_same(tally, w_tally[pi, gi, bi], "tally")
    assert sums.shape == (pm.P, 4)
    st = state_of(env)
    check_final(st, final, (pi, gi, bi), "schedules")
    halves = fused_env()
    a, _ = halves.rollout_schedules(T(sch), (max_steps, dm.FAIL_DEG), K // 2)
    b, _ = halves.rollout_schedules(T(sch), (max_steps, dm.FAIL_DEG), K // 2)
    assert_same((a + b).cpu().numpy()[:, :3], tally[:, :3], "halves' counts")
    assert_states_equal(state_of(halves), st, "halves")
    env.close(), halves.close()


@pytest.mark.gpu
def test_rollout_feedback_under_disturbance_matches_the_wrapper_with_and_without_rows():
    K, max_steps = dm.STEPS, dm.MAX_STEPS
    pi, gi, bi, _ = pm.fused_layout()
    sched, edges = pm.feedback_policies()
    w_tally, w_rows, final = dm.feedback_streams(max_steps)
    env = fused_env()
    tally, sums, rows = env.rollout_feedback(T(sched), T(edges), (max_steps, dm.FAIL_DEG), K, abs_key=True, record=True)
    assert_same(tally.cpu().numpy(), w_tally[pi, gi, bi], "tally")
    for f in ("device", "duration", "obs", "reward", "angle", "ended"):
        assert_same(rows[f].cpu().numpy(), w_rows[f][:, pi, gi, bi], ("rows", f))
    st = state_of(env)
    check_final(st, final, (pi, gi, bi), "feedback")
    halves = fused_env()                                 # without rows: the other kernel, in two calls of K / 2
    a, _ = halves.rollout_feedback(T(sched), T(edges), (max_steps, dm.FAIL_DEG), K // 2)
    b, _ = halves.rollout_feedback(T(sched), T(edges), (max_steps, dm.FAIL_DEG), K // 2)
    assert_same((a + b).cpu().numpy()[:, (0, 1, 2, 4, 7)], w_tally[pi, gi, bi][:, (0, 1, 2, 4, 7)], "halves' counts")
    assert_states_equal(state_of(halves), st, "halves")
    env.close(), halves.close()


# ---- 3. a partial block in the fused kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rollout_at_seventy_envs_matches_the_model_step_for_step():
    N, K, seed, start, period = 70, 70, 1, 20, 10
    gi, so, _ = step_layout(N)
    dev, dur, steps = dm.step_streams(None, K, seed, start, period)
    env = step_env(N, start, period)
    obs, rew, done, info = env.rollout(T(dev[:, so]), T(dur[:, so]))
    assert_same(obs.cpu().numpy(), np.array([w["obs"][gi, so] for w in steps]), "obs")
    assert_same(rew.cpu().numpy(), np.array([w["rew"][gi, so] for w in steps]), "reward")
    assert_same(info["Sensor angle"].cpu().numpy(), np.array([w["ang"][gi, so] for w in steps]), "angle")
    assert not done.any()
    st = state_of(env, MODEL_FIELDS)
    for f in MODEL_FIELDS:
        assert_same(st[f], steps[-1][f][gi, so], f)
    env.close()


# ---- 4. zero weights on a switched handle are the gains' handle --------------------------------------------------------------------------
@pytest.mark.gpu
def test_zero_weights_equal_a_handle_that_only_set_the_default_gains():
    from gymwipe_amd import VecControlLoopEnv
    _, _, _, so = pm.fused_layout()

    def make():
        env = VecControlLoopEnv(pm.N_FUSED, ctrl_start_tick=g.START, ctrl_period_ticks=g.PERIOD, gains=(1.0, 0.0, 0.0))
        env.set_initial_state(T(g.X0S[so]), T(g.U0S[so]))
        env.reset_envs()
        return env
    one, two = make(), make()
    one.set_disturbance(np.zeros(4))                     # default keys; `two` stays on the gains' kernels
    dev, dur = pm.episode_actions()
    d, u = T(dev[:, so]), T(dur[:, so])
    fields = tuple(f for f in DIST_FIELDS if f not in ("noise_key", "noise_count"))

    def same_state(what):
        a, b = state_of(one), state_of(two)
        assert_states_equal(a, b, what, fields)
        assert (b["noise_count"] == 0).all() and (b["noise_key"] == 0).all(), what       # never read, never written
        assert not np.signbit(b["x"][b["x"] == 0.0]).any(), what                        # (no -0.0 for the rule to turn)
        return a["noise_count"]

    for k in range(12):
        a, b = one.step({"device": d[k], "duration": u[k]}), two.step({"device": d[k], "duration": u[k]})
        for x, y in ((a[0], b[0]), (a[1], b[1]), (a[3]["Sensor angle"], b[3]["Sensor angle"])):
            assert_same(x.cpu().numpy(), y.cpu().numpy(), ("step", k))
    moved = same_state("step")
    assert_same(moved, one.get_state("substeps"), "one draw per substep")
    assert (moved > 0).all()
    a, b = one.rollout(d[12:], u[12:], episodes=(pm.SHORT_MAX_STEPS, pm.FAIL_DEG)), two.rollout(d[12:], u[12:], episodes=(pm.SHORT_MAX_STEPS, pm.FAIL_DEG))
    for x, y in ((a[0], b[0]), (a[1], b[1]), (a[2], b[2]), (a[3]["Sensor angle"], b[3]["Sensor angle"])):
        assert_same(x.cpu().numpy(), y.cpu().numpy(), "rollout")
    assert a[2].any()
    after = same_state("rollout")
    assert (after > moved).all()
    sch = T(g.schedules_of(pm.P, pm.ROLLOUT_L))
    a, b = one.rollout_schedules(sch, (pm.MAX_STEPS, pm.FAIL_DEG), 40), two.rollout_schedules(sch, (pm.MAX_STEPS, pm.FAIL_DEG), 40)
    assert_same(a[0].cpu().numpy(), b[0].cpu().numpy(), "schedules")
    moved, after = after, same_state("schedules")
    assert (after > moved).all()
    sched, edges = pm.feedback_policies()
    a = one.rollout_feedback(T(sched), T(edges), (pm.MAX_STEPS, pm.FAIL_DEG), 40, record=True)
    b = two.rollout_feedback(T(sched), T(edges), (pm.MAX_STEPS, pm.FAIL_DEG), 40, record=True)
    assert_same(a[0].cpu().numpy(), b[0].cpu().numpy(), "feedback")
    for f in a[2]:
        assert_same(a[2][f].cpu().numpy(), b[2][f].cpu().numpy(), ("feedback", f))
    moved, after = after, same_state("feedback")
    assert (after > moved).all()
    a, b = one.rollout_feedback(T(sched), T(edges), (pm.MAX_STEPS, pm.FAIL_DEG), 20), two.rollout_feedback(T(sched), T(edges), (pm.MAX_STEPS, pm.FAIL_DEG), 20)
    assert_same(a[0].cpu().numpy(), b[0].cpu().numpy(), "feedback without rows")
    moved, after = after, same_state("feedback without rows")
    assert (after > moved).all()
    one.close(), two.close()


# ---- 5. common random numbers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_equal_keys_walk_equal_trajectories_wherever_the_envs_sit():
    from gymwipe_amd import VecControlLoopEnv, actions
    N, K = 256, 40
    A, B, C = 3, 200, 70                                 # lanes 3, 8 and 6 of blocks 0, 3 and 1
    rng = np.random.default_rng(11)
    dev = rng.integers(0, 2, (K, N)).astype(np.int32)
    dur = rng.integers(0, 20, (K, N)).astype(np.int32)
    x0 = rng.uniform(-0.3, 0.3, (N, 4))
    gains = np.tile([0.1, 0.0, 0.05], (N, 1)) * rng.uniform(0.5, 1.5, (N, 1))
    weights, key = actions.make_ctrl_disturbance((0.001, 0.0, 0.0005, 0.01), N, seed=77)
    for e in (B, C):
        dev[:, e], dur[:, e], x0[e], gains[e], key[e] = dev[:, A], dur[:, A], x0[A], gains[A], key[A]
    weights[C] = (0.001, 0.0, 0.0005, 0.02)              # C: the same key, other weights
    env = VecControlLoopEnv(N, ctrl_start_tick=g.START, ctrl_period_ticks=g.PERIOD, gains=T(gains))
    env.set_initial_state(T(x0))
    env.reset_envs()
    env.set_disturbance(T(weights), key)
    obs, rew, ended, info = env.rollout(T(dev), T(dur), episodes=(pm.SHORT_MAX_STEPS, pm.FAIL_DEG))
    ang = info["Sensor angle"].cpu().numpy()
    assert_same(ang[:, B], ang[:, A], "angles of the pair")
    assert ended[:, A].any()
    st = state_of(env)
    for f in DIST_FIELDS:
        assert_same(st[f][B], st[f][A], ("the pair", f))
    assert (ang[:, C] != ang[:, A]).any() and (st["x"][C] != st["x"][A]).any()
    assert st["noise_count"][C] == st["noise_count"][A] and st["noise_key"][C] == st["noise_key"][A]
    others = [e for e in range(N) if e not in (A, B, C)]
    assert len({st["x"][e].tobytes() for e in others}) == len(others)
    env.close()


# ---- 6. set_disturbance with a mask, mid-run; reset ----------------------------------------------------------------------------------------
MASKED = (13, 22, 31, 40, 63, 64, 69)               # sets 1, 2, 3, 5, 7 in the full block, its last lane, the partial block's first and last
NEW_WEIGHTS = (0.003, -0.001, 0.0, 0.015)


def _new_keys(N):
    from gymwipe_amd import actions
    return actions.make_ctrl_disturbance(np.zeros(4), N, seed=1234567)[1]


def _masked_models(K0, K, start, period, reset=False):
    """The masked envs' models after K0 steps and K - K0 more under NEW_WEIGHTS and a new key, the count from 0 (``reset``: as
    fresh models instead, whose plants keep weights, key and count).  Returns {field: [len(MASKED)]...}."""
    gi, so, _ = step_layout(70)
    keys = _new_keys(70)
    dev, dur, _ = dm.step_streams(None, K, 1, start, period)
    states = []
    for e in MASKED:
        m = dm.step_model(None, start, period, gi[e], so[e])
        for k in range(K):
            if k == K0:
                if reset:
                    m = dm.disturb(pm.PidControlLoopModel(start=start, period=period, gains=pm.GAIN_SETS[gi[e]]), m.plant.g, m.plant.key, m.plant.n)
                else:
                    dm.disturb(m, NEW_WEIGHTS, int(keys[e]), 0)
            m.step(int(dev[k, so[e]]), int(dur[k, so[e]]))
        states.append(dm.snapshot_of(m))
    out = {f: np.array([s[f] for s in states], np.float64) for f in ("now", "x", "u", "angle_deg", "rx_power", "gains", "last_error", "disturbance")}
    out["qlen"] = np.array([s["qlen"][:2] for s in states], np.int64)
    out["received"] = np.array([s["received"][1:] for s in states], np.int64)
    for f in ("n_tx", "commands", "substeps"):
        out[f] = np.array([s[f] for s in states], np.int64)
    for f in ("noise_key", "noise_count"):
        out[f] = np.array([s[f] for s in states], np.uint64)
    return out


@pytest.mark.gpu
def test_set_disturbance_with_a_mask_mid_run_touches_the_masked_records_and_nothing_else():
    N, K0, K, start, period = 70, 35, 70, 20, 10
    gi, so, _ = step_layout(N)
    dev, dur, steps = dm.step_streams(None, K, 1, start, period)
    env = step_env(N, start, period)
    for k in range(K0):
        env.step({"device": T(dev[k][so]), "duration": T(dur[k][so])})
    before = state_of(env)
    assert (before["noise_count"] > 0).all()
    mask = np.zeros(N, np.uint8)
    mask[list(MASKED)] = 1
    m = mask.astype(bool)
    keys = _new_keys(N)
    env.set_disturbance(NEW_WEIGHTS, keys, mask=T(mask))
    after = state_of(env)
    for f in DIST_FIELDS:
        if f not in ("disturbance", "noise_key", "noise_count"):
            assert_same(after[f], before[f], ("running state", f))
        else:
            assert_same(after[f][~m], before[f][~m], ("other envs", f))
    assert_same(after["disturbance"][m], np.tile(NEW_WEIGHTS, (m.sum(), 1)), "masked weights")
    assert_same(after["noise_key"][m], keys[m], "masked keys")
    assert (after["noise_count"][m] == 0).all()
    for k in range(K0, K):
        env.step({"device": T(dev[k][so]), "duration": T(dur[k][so])})
    st = state_of(env, MODEL_FIELDS)
    want = _masked_models(K0, K, start, period)
    for f in MODEL_FIELDS:
        assert_same(st[f][~m], steps[-1][f][gi, so][~m], ("other envs", f))       # as if nothing had happened
        assert_same(st[f][m], want[f], ("masked envs", f))                         # their own past, the new record from K0 on
    assert (st["noise_count"][m] < st["substeps"][m]).all()
    env.close()


@pytest.mark.gpu
def test_reset_leaves_weights_key_and_count_and_the_plant_draws_on():
    N, K0, K, start, period = 70, 35, 70, 20, 10
    gi, so, _ = step_layout(N)
    dev, dur, steps = dm.step_streams(None, K, 1, start, period)
    env = step_env(N, start, period)
    for k in range(K0):
        env.step({"device": T(dev[k][so]), "duration": T(dur[k][so])})
    before = state_of(env)
    mask = np.zeros(N, np.uint8)
    mask[list(MASKED)] = 1
    m = mask.astype(bool)
    env.reset_envs(T(mask))
    after = state_of(env)
    for f in DIST_FIELDS:
        assert_same(after[f][~m], before[f][~m], ("untouched", f))
    for f in ("disturbance", "noise_key", "noise_count", "gains"):
        assert_same(after[f], before[f], ("survives a reset", f))
    assert (after["now"][m] == 0).all() and (after["substeps"][m] == 0).all() and (after["noise_count"][m] > 0).all()
    for k in range(K0, K):
        env.step({"device": T(dev[k][so]), "duration": T(dur[k][so])})
    st = state_of(env, MODEL_FIELDS)
    want = _masked_models(K0, K, start, period, reset=True)
    for f in MODEL_FIELDS:
        assert_same(st[f][~m], steps[-1][f][gi, so][~m], ("other envs", f))
        assert_same(st[f][m], want[f], ("reset envs: fresh models, the old plants' records", f))
    env.close()


# ---- 7. refusals and surface --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_set_disturbance_refusals_come_before_any_launch_and_the_env_has_the_new_verbs():
    import torch
    import gymwipe_amd
    from gymwipe_amd import _native as nat
    from gymwipe_amd import actions
    N = 128
    env = gymwipe_amd.make("VecControlLoop-v0", num_envs=N)
    assert callable(env.set_disturbance)
    for f, shape, dt in (("disturbance", (N, 4), np.float64), ("noise_key", (N,), np.uint64), ("noise_count", (N,), np.uint64)):
        assert env.get_state(f).shape == shape and env.get_state(f).dtype == dt and (env.get_state(f) == 0).all()
    L = nat.lib()
    some = torch.zeros((N, 4), dtype=torch.float64, device="cuda")
    keys = torch.zeros(N, dtype=torch.int64, device="cuda")
    before = state_of(env)
    assert L.gw_ctrl_set_disturbance(None, some.data_ptr(), keys.data_ptr(), None, None) == nat.EINVAL
    assert L.gw_ctrl_set_disturbance(env._h, None, keys.data_ptr(), None, None) == nat.EINVAL
    assert L.gw_ctrl_set_disturbance(env._h, some.data_ptr(), None, None, None) == nat.EINVAL
    for args, word in (((env._h, None, keys.data_ptr(), None, None), "g_dev"), ((env._h, some.data_ptr(), None, None, None), "key_dev")):
        with pytest.raises(nat.NativeError) as err:
            nat.check(L.gw_ctrl_set_disturbance(*args))
        assert err.value.code == nat.EINVAL and word in str(err.value)
    for bad_g, bad_key in (([1.0, 0.0, 0.0], None), (np.zeros((N - 1, 4)), None), (np.zeros(4), np.zeros(N, np.int64)),
                           (np.zeros(4), np.zeros(N - 1, np.uint64)), (np.zeros(4), torch.zeros(N, dtype=torch.int32))):
        with pytest.raises(ValueError):
            env.set_disturbance(bad_g, bad_key)
    assert_states_equal(state_of(env), before, "refused")
    top = np.full(N, 0x8000000000000001, np.uint64)      # keys with the top bit set, both ways in
    env.set_disturbance((0.0, 0.0, 0.0, 0.5), top, mask=torch.arange(N) < 64)
    env.set_disturbance(torch.full((N, 4), 2.0, dtype=torch.float64, device="cuda"), T(top.view(np.int64) + 1).cuda(), mask=np.arange(N) >= 96)
    lo, hi = (np.arange(N) < 64), (np.arange(N) >= 96)
    assert_same(env.get_state("disturbance"), np.where(lo[:, None], [0.0, 0.0, 0.0, 0.5], np.where(hi[:, None], 2.0, 0.0)), "weights")
    assert_same(env.get_state("noise_key"), np.where(lo, top, np.where(hi, top + np.uint64(1), np.uint64(0))), "keys")
    buf = np.empty(N * 2)                                 # a wrong size is refused, as for every field
    for f in (b"disturbance", b"noise_key", b"noise_count"):
        assert L.gw_ctrl_get_state(env._h, f, buf.ctypes.data, buf.nbytes) == nat.EFIELD
    env.close()
    env = gymwipe_amd.make("VecControlLoop-v0", num_envs=N, disturbance=(0.0, 0.0, 0.0, 0.01))
    assert (env.get_state("disturbance") == [0.0, 0.0, 0.0, 0.01]).all()
    assert_same(env.get_state("noise_key"), actions.make_ctrl_disturbance(np.zeros(4), N)[1], "the default keys")
    env.step({"device": torch.zeros(N, dtype=torch.int32), "duration": torch.full((N,), 19, dtype=torch.int32)})
    x = env.get_state("x")
    assert len({r.tobytes() for r in x}) == N             # every env a noise sequence of its own
    assert_same(env.get_state("noise_count"), env.get_state("substeps"), "count")
    env.close()
