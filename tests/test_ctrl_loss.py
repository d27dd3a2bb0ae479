"""Seeded packet erasures of the control loop on the GPU (gw_ctrl_set_loss): the loss instantiations of the step kernel and of the
fused rollout kernels against the event-driven model of tests/ctrl_loss_model.py, bit for bit, over every state field, the
controller's two, the disturbance's three and the loss's four (``loss``, ``loss_key``, ``loss_count``, ``lost``).  Loss set i
runs under disturbance set i and gain set i, so all three rules run together.  A reset env is a freshly constructed model that
goes on drawing where the old one stopped.  The fixtures are defined in tests/ctrl_loss_model.py and qualified on the model
alone in tests/test_ctrl_loss_cpu.py (every link loses decoded packets and delivers others, both ending causes occur, draws
fall on transmissions the PHY rejected, four wrong rules are told apart).  Every test calls ``set_loss``: none passes without
it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctrl_dist_model as cd
import ctrl_loss_model as lm
import ctrl_pid_model as pm
import test_ctrl_rollout as g
from test_control_loop import DENSE_CTRL, stream_of
from test_ctrl_rollout import ALL_FIELDS, FIELDS, T, assert_same

NEW_FIELDS = ("gains", "last_error", "disturbance", "noise_key", "noise_count") + lm.LOSS_FIELDS
LOSS_STATE = ALL_FIELDS + NEW_FIELDS
MODEL_FIELDS = FIELDS + NEW_FIELDS
GAINS, WEIGHTS, THR = pm.gains_array(), cd.g_array(), lm.thr_array()
PROBS = np.array(lm.P_SETS, np.float64)


def state_of(env, fields=LOSS_STATE):
    return {f: env.get_state(f) for f in fields}


def assert_states_equal(a, b, what, fields=LOSS_STATE):
    for f in fields:
        assert_same(a[f], b[f], (what, f))


def step_layout(N):
    """The step cases' envs: action stream ``stream_of(e)``, loss, weight and gain set ``(e // 8) % 8`` -- the first 64 envs are
    the 64 pairs -- and the pair's own noise key and loss key."""
    from gymwipe_amd import actions
    gi, so = (np.arange(N) // 8) % lm.G, stream_of(N)
    _, nkey = actions.make_ctrl_disturbance(np.zeros(4), N, seed=cd.SEED, streams=gi * 8 + so)
    _, lkey = actions.make_ctrl_loss(np.zeros(4), N, seed=lm.SEED, streams=gi * 8 + so)
    return gi, so, nkey, lkey


def step_env(N, start, period, plant=None, layout=None):
    from gymwipe_amd import VecControlLoopEnv
    gi, _, nkey, lkey = step_layout(N)
    kw = {} if plant is None else {"A": DENSE_CTRL["A"], "B": DENSE_CTRL["B"], "x0": DENSE_CTRL["x0"], "u0": DENSE_CTRL["u0"]}
    if layout is not None:
        from test_control_loop_edges import LAYOUTS
        pos, rrm = LAYOUTS[layout]
        kw["positions"] = pos + (rrm,)
    env = VecControlLoopEnv(N, ctrl_start_tick=start, ctrl_period_ticks=period, gains=T(GAINS[gi]), **kw)
    env.set_disturbance(T(WEIGHTS[gi]), nkey)
    env.set_loss(PROBS[gi], lkey)
    return env


def fused_env():
    """512 envs on the fused cases' layout: every env starts from its stream's X0S / U0S under its gain set, its weights, its loss
    set and its model's two keys."""
    from gymwipe_amd import VecControlLoopEnv, actions
    _, gi, _, so = pm.fused_layout()
    env = VecControlLoopEnv(pm.N_FUSED, ctrl_start_tick=g.START, ctrl_period_ticks=g.PERIOD)
    env.set_initial_state(T(g.X0S[so]), T(g.U0S[so]))
    env.reset_envs()
    env.set_gains(actions.make_ctrl_gains(pm.GAIN_SETS, pm.N_FUSED, pm.PER_SET))
    env.set_disturbance(actions.make_ctrl_disturbance(cd.G_SETS, pm.N_FUSED, envs_per_set=pm.PER_SET)[0], cd.fused_keys())
    thr, _ = actions.make_ctrl_loss(lm.P_SETS, pm.N_FUSED, envs_per_set=pm.PER_SET)
    assert_same(thr, THR[gi], "the helper's thresholds are the model's")
    env.set_loss(PROBS[gi], lm.fused_keys())
    return env


def check_final(st, final, index, what):
    for f in MODEL_FIELDS + ("age", "cost"):
        assert_same(st[f], final[f][index], (what, f))
    assert not (st["flags"] & 3).any(), what


def run_steps(env, dev, dur, steps, gi, so, k0, k1, every=True):
    """Steps k0 .. k1 - 1 of the step fixture through ``env.step``, compared with the model after every step."""
    for k in range(k0, k1):
        obs, rew, done, info = env.step({"device": T(dev[k][so]), "duration": T(dur[k][so])})
        if not every:
            continue
        got = {"obs": obs.cpu().numpy(), "rew": rew.cpu().numpy(), "ang": info["Sensor angle"].cpu().numpy()}
        got.update(state_of(env, MODEL_FIELDS))
        for f, w in steps[k].items():
            assert_same(got[f], w[gi, so], (f, k))
        assert_same(got["loss_count"], got["n_tx"], ("one draw per transmission", k))
        assert not done.any()


# ---- 1. step -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("plant", [None, "dense"])
@pytest.mark.parametrize("seed,start,period", [(1, 20, 10), (2, 0, 3), (3, 50, 1)])
def test_step_with_per_env_loss_matches_the_model(seed, start, period, plant):
    N, K = 70, 70                                        # one full block and a partial one
    gi, so, _, lkey = step_layout(N)
    dev, dur, steps, _ = lm.step_streams(plant, K, seed, start, period)
    env = step_env(N, start, period, plant)
    assert_same(env.get_state("loss"), THR[gi], "thresholds as set")
    assert_same(env.get_state("loss_key"), lkey, "keys as set")
    assert (env.get_state("loss_count") == 0).all() and (env.get_state("lost") == 0).all()
    run_steps(env, dev, dur, steps, gi, so, 0, K)
    assert not (env.get_state("flags") & 3).any()
    lost = env.get_state("lost")
    assert (lost[gi == 0] == 0).all() and (lost[gi == 5] > 0).all()
    env.close()


@pytest.mark.gpu
def test_step_where_the_phy_rejects_commands_still_draws_for_them():
    """tests/test_control_loop_edges.LAYOUTS["same_distance"]: no command decodes at the actuator; each takes its draw."""
    from test_control_loop_edges import K, PERIOD, SEED, START
    N = 70
    gi, so, _, _ = step_layout(N)
    dev, dur, steps, _ = lm.step_streams(None, K, SEED, START, PERIOD, layout=lm.FAILING_LAYOUT)
    env = step_env(N, START, PERIOD, layout=lm.FAILING_LAYOUT)
    run_steps(env, dev, dur, steps, gi, so, 0, K)
    st = state_of(env, ("received", "lost", "loss_count", "n_tx"))
    assert (st["received"][:, 1] == 0).all() and (st["lost"][:, 3] > 0).any()          # nothing arrived; commands were erased too
    env.close()


# ---- 2. - 4. the fused rollouts, and K / 2 + K / 2 = K ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rollout_with_episodes_under_loss_matches_the_wrapper_and_splits():
    K, max_steps = lm.STEPS, lm.SHORT_MAX_STEPS
    pi, gi, bi, so = pm.fused_layout()
    dev, dur = pm.episode_actions()
    w_obs, w_rew, w_ang, w_ended, final, _ = lm.episode_streams(max_steps)
    d, u = T(dev[:, so]), T(dur[:, so])
    env = fused_env()
    obs, rew, ended, info = env.rollout(d, u, episodes=(max_steps, lm.FAIL_DEG))
    assert_same(ended.cpu().numpy(), w_ended[:, pi, gi, bi], "ended")
    assert_same(obs.cpu().numpy(), w_obs[:, pi, gi, bi], "obs") and assert_same(rew.cpu().numpy(), w_rew[:, pi, gi, bi], "reward")
    assert_same(info["Sensor angle"].cpu().numpy(), w_ang[:, pi, gi, bi], "angle")
    st = state_of(env)
    check_final(st, final, (pi, gi, bi), "rollout")
    assert (st["loss_count"] > st["n_tx"]).sum() > 256                          # resets happened, and the count ran on
    halves = fused_env()                                 # two calls of K / 2: the record is handle state, as age and cost are
    a = halves.rollout(d[:K // 2], u[:K // 2], episodes=(max_steps, lm.FAIL_DEG))
    assert (halves.get_state("loss_count") > 0).all()
    b = halves.rollout(d[K // 2:], u[K // 2:], episodes=(max_steps, lm.FAIL_DEG))
    assert_same(np.concatenate([a[3]["Sensor angle"].cpu().numpy(), b[3]["Sensor angle"].cpu().numpy()]), w_ang[:, pi, gi, bi], "halves")
    assert_states_equal(state_of(halves), st, "halves")
    env.close(), halves.close()


@pytest.mark.gpu
def test_rollout_schedules_under_loss_matches_the_wrapper_and_splits():
    K, max_steps = lm.STEPS, lm.MAX_STEPS
    pi, gi, bi, _ = pm.fused_layout()
    sch, w_tally, final, _, _, _ = lm.schedule_streams(max_steps)
    env = fused_env()
    tally, sums = env.rollout_schedules(T(sch), (max_steps, lm.FAIL_DEG), K)
    tally = tally.cpu().numpy()
    assert_same(tally, w_tally[pi, gi, bi], "tally")
    assert sums.shape == (pm.P, 4)
    st = state_of(env)
    check_final(st, final, (pi, gi, bi), "schedules")
    halves = fused_env()
    a, _ = halves.rollout_schedules(T(sch), (max_steps, lm.FAIL_DEG), K // 2)
    b, _ = halves.rollout_schedules(T(sch), (max_steps, lm.FAIL_DEG), K // 2)
    assert_same((a + b).cpu().numpy()[:, :3], tally[:, :3], "halves' counts")
    assert_states_equal(state_of(halves), st, "halves")
    env.close(), halves.close()


@pytest.mark.gpu
def test_rollout_feedback_under_loss_matches_the_wrapper_with_and_without_rows():
    K, max_steps = lm.STEPS, lm.MAX_STEPS
    pi, gi, bi, _ = pm.fused_layout()
    sched, edges = pm.feedback_policies()
    w_tally, w_rows, final, _ = lm.feedback_streams(max_steps)
    env = fused_env()
    tally, sums, rows = env.rollout_feedback(T(sched), T(edges), (max_steps, lm.FAIL_DEG), K, abs_key=True, record=True)
    assert_same(tally.cpu().numpy(), w_tally[pi, gi, bi], "tally")
    for f in ("device", "duration", "obs", "reward", "angle", "ended"):
        assert_same(rows[f].cpu().numpy(), w_rows[f][:, pi, gi, bi], ("rows", f))
    st = state_of(env)
    check_final(st, final, (pi, gi, bi), "feedback")
    halves = fused_env()                                 # without rows: the other kernel, in two calls of K / 2
    a, _ = halves.rollout_feedback(T(sched), T(edges), (max_steps, lm.FAIL_DEG), K // 2)
    b, _ = halves.rollout_feedback(T(sched), T(edges), (max_steps, lm.FAIL_DEG), K // 2)
    assert_same((a + b).cpu().numpy()[:, (0, 1, 2, 4, 7)], w_tally[pi, gi, bi][:, (0, 1, 2, 4, 7)], "halves' counts")
    assert_states_equal(state_of(halves), st, "halves")
    env.close(), halves.close()


# ---- 5. a partial block in the fused kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rollout_at_seventy_envs_matches_the_model_step_for_step():
    N, K, seed, start, period = 70, 70, 1, 20, 10
    gi, so, _, _ = step_layout(N)
    dev, dur, steps, _ = lm.step_streams(None, K, seed, start, period)
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


# ---- 6. zero thresholds on a switched handle are the disturbance's handle ---------------------------------------------------------------------
@pytest.mark.gpu
def test_zero_thresholds_equal_a_handle_that_only_set_the_disturbance():
    from gymwipe_amd import VecControlLoopEnv, actions
    _, _, _, so = pm.fused_layout()
    weights = actions.make_ctrl_disturbance(cd.G_SETS, pm.N_FUSED, envs_per_set=pm.PER_SET)[0]

    def make():
        env = VecControlLoopEnv(pm.N_FUSED, ctrl_start_tick=g.START, ctrl_period_ticks=g.PERIOD)
        env.set_initial_state(T(g.X0S[so]), T(g.U0S[so]))
        env.reset_envs()
        env.set_gains(actions.make_ctrl_gains(pm.GAIN_SETS, pm.N_FUSED, pm.PER_SET))
        env.set_disturbance(weights, cd.fused_keys())
        return env
    one, two = make(), make()
    one.set_loss(np.zeros(4))                            # default keys; `two` stays on the disturbance's kernels
    dev, dur = pm.episode_actions()
    d, u = T(dev[:, so]), T(dur[:, so])
    fields = tuple(f for f in LOSS_STATE if f not in ("loss_key", "loss_count"))
    walked = np.zeros(pm.N_FUSED, np.uint64)             # transmissions of the episodes that have ended

    def same_state(what, ended=None):
        a, b = state_of(one), state_of(two)
        assert_states_equal(a, b, what, fields)
        assert (b["loss_count"] == 0).all() and (b["loss_key"] == 0).all() and (b["lost"] == 0).all(), what   # never read or written
        assert (a["lost"] == 0).all() and (a["loss"] == 0).all(), what
        return a

    for k in range(12):
        a, b = one.step({"device": d[k], "duration": u[k]}), two.step({"device": d[k], "duration": u[k]})
        for x, y in ((a[0], b[0]), (a[1], b[1]), (a[3]["Sensor angle"], b[3]["Sensor angle"])):
            assert_same(x.cpu().numpy(), y.cpu().numpy(), ("step", k))
    st = same_state("step")
    assert_same(st["loss_count"], st["n_tx"].astype(np.uint64), "one draw per transmission")
    assert (st["loss_count"] > 0).all()
    # the sum of n_tx over the episodes walked: one step per call from here on, n_tx read before each reset takes it away
    ep = (pm.SHORT_MAX_STEPS, pm.FAIL_DEG)
    for k in range(12, 24):
        before = one.get_state("n_tx").astype(np.uint64)
        a, b = one.rollout(d[k:k + 1], u[k:k + 1], episodes=ep), two.rollout(d[k:k + 1], u[k:k + 1], episodes=ep)
        for x, y in ((a[0], b[0]), (a[1], b[1]), (a[2], b[2]), (a[3]["Sensor angle"], b[3]["Sensor angle"])):
            assert_same(x.cpu().numpy(), y.cpu().numpy(), ("rollout", k))
        ended = a[2][0].cpu().numpy() != 0
        count = one.get_state("loss_count")
        now = one.get_state("n_tx").astype(np.uint64)
        walked[ended] = count[ended]                     # an ended env's count is everything it ever sent
        assert_same(count, walked + now, ("loss_count is the sum of n_tx over the episodes walked", k))
        assert (now[~ended] >= before[~ended]).all()
    assert (walked > 0).any()
    moved = same_state("rollout")["loss_count"]
    a, b = one.rollout(d[24:], u[24:], episodes=ep), two.rollout(d[24:], u[24:], episodes=ep)
    for x, y in ((a[0], b[0]), (a[1], b[1]), (a[2], b[2]), (a[3]["Sensor angle"], b[3]["Sensor angle"])):
        assert_same(x.cpu().numpy(), y.cpu().numpy(), "rollout")
    assert a[2].any()
    after = same_state("rollout")["loss_count"]
    assert (after > moved).all()
    sch = T(g.schedules_of(pm.P, pm.ROLLOUT_L))
    a, b = one.rollout_schedules(sch, (pm.MAX_STEPS, pm.FAIL_DEG), 40), two.rollout_schedules(sch, (pm.MAX_STEPS, pm.FAIL_DEG), 40)
    assert_same(a[0].cpu().numpy(), b[0].cpu().numpy(), "schedules")
    moved, after = after, same_state("schedules")["loss_count"]
    assert (after > moved).all()
    sched, edges = pm.feedback_policies()
    a = one.rollout_feedback(T(sched), T(edges), (pm.MAX_STEPS, pm.FAIL_DEG), 40, record=True)
    b = two.rollout_feedback(T(sched), T(edges), (pm.MAX_STEPS, pm.FAIL_DEG), 40, record=True)
    assert_same(a[0].cpu().numpy(), b[0].cpu().numpy(), "feedback")
    for f in a[2]:
        assert_same(a[2][f].cpu().numpy(), b[2][f].cpu().numpy(), ("feedback", f))
    moved, after = after, same_state("feedback")["loss_count"]
    assert (after > moved).all()
    a, b = one.rollout_feedback(T(sched), T(edges), (pm.MAX_STEPS, pm.FAIL_DEG), 20), two.rollout_feedback(T(sched), T(edges), (pm.MAX_STEPS, pm.FAIL_DEG), 20)
    assert_same(a[0].cpu().numpy(), b[0].cpu().numpy(), "feedback without rows")
    moved, after = after, same_state("feedback without rows")["loss_count"]
    assert (after > moved).all()
    one.close(), two.close()


# ---- 7. common random numbers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_equal_records_walk_equal_trajectories_wherever_the_envs_sit():
    from gymwipe_amd import VecControlLoopEnv, actions
    N, K = 256, 40
    A, B, C = 3, 200, 70                                 # lanes 3, 8 and 6 of blocks 0, 3 and 1
    rng = np.random.default_rng(11)
    dev = rng.integers(0, 2, (K, N)).astype(np.int32)
    dur = rng.integers(0, 20, (K, N)).astype(np.int32)
    x0 = rng.uniform(-0.3, 0.3, (N, 4))
    gains = np.tile([0.1, 0.0, 0.05], (N, 1)) * rng.uniform(0.5, 1.5, (N, 1))
    weights, nkey = actions.make_ctrl_disturbance((0.001, 0.0, 0.0005, 0.01), N, seed=77)
    p = np.tile([0.3, 0.2, 0.4, 0.25], (N, 1))
    _, lkey = actions.make_ctrl_loss(np.zeros(4), N, seed=78)
    for e in (B, C):
        dev[:, e], dur[:, e], x0[e], gains[e], nkey[e], lkey[e] = dev[:, A], dur[:, A], x0[A], gains[A], nkey[A], lkey[A]
    lkey[C] ^= np.uint64(1)                              # C: everything as A but the loss key
    env = VecControlLoopEnv(N, ctrl_start_tick=g.START, ctrl_period_ticks=g.PERIOD, gains=T(gains))
    env.set_initial_state(T(x0))
    env.reset_envs()
    env.set_disturbance(T(weights), nkey)
    env.set_loss(p, lkey)
    obs, rew, ended, info = env.rollout(T(dev), T(dur), episodes=(pm.SHORT_MAX_STEPS, pm.FAIL_DEG))
    ang = info["Sensor angle"].cpu().numpy()
    assert_same(ang[:, B], ang[:, A], "angles of the pair")
    assert ended[:, A].any()
    st = state_of(env)
    for f in LOSS_STATE:
        assert_same(st[f][B], st[f][A], ("the pair", f))
    assert st["lost"][A].all()
    # (the final x may agree: both envs were reset five steps before the end, face the same noise, and differ in x only once
    # a command reaches one and not the other)
    assert (ang[:, C] != ang[:, A]).any() and (st["lost"][C] != st["lost"][A]).any()
    others = [e for e in range(N) if e not in (A, B, C)]
    assert len({st["x"][e].tobytes() for e in others}) == len(others)
    env.close()


# ---- 8., 9. set_loss with a mask, mid-run; reset ------------------------------------------------------------------------------------------------
MASKED = (13, 22, 31, 40, 63, 64, 69)               # sets 1, 2, 3, 5, 7 in the full block, its last lane, the partial block's first and last
NEW_P = (0.2, 0.35, 0.15, 0.45)
NEW_THR = tuple(lm.threshold(v) for v in NEW_P)


def _new_keys(N):
    from gymwipe_amd import actions
    return actions.make_ctrl_loss(np.zeros(4), N, seed=7654321)[1]


def _masked_models(K0, K, start, period, reset=False):
    """The masked envs' models after K0 steps and K - K0 more under NEW_THR and a new key, the counts from 0 (``reset``: as
    fresh models instead, which keep the plant's and the loss's records).  Returns {field: [len(MASKED)]...}."""
    gi, so, _, _ = step_layout(70)
    keys = _new_keys(70)
    dev, dur, _, _ = lm.step_streams(None, K, 1, start, period)
    states = []
    for e in MASKED:
        m = lm.step_model(None, start, period, gi[e], so[e])
        for k in range(K):
            if k == K0:
                if reset:
                    old = m
                    m = cd.disturb(pm.PidControlLoopModel(start=start, period=period, gains=pm.GAIN_SETS[gi[e]]), old.plant.g, old.plant.key,
                                   old.plant.n)
                    lm.attach(m, old.loss.thr, old.loss.key, old.loss.n, old.loss.lost)
                else:
                    m.loss.thr, m.loss.key, m.loss.n, m.loss.lost = list(NEW_THR), int(keys[e]), 0, [0, 0, 0, 0]
            m.step(int(dev[k, so[e]]), int(dur[k, so[e]]))
        states.append(lm.snapshot_of(m))
    out = {f: np.array([s[f] for s in states], np.float64) for f in ("now", "x", "u", "angle_deg", "rx_power", "gains", "last_error", "disturbance")}
    out["qlen"] = np.array([s["qlen"][:2] for s in states], np.int64)
    out["received"] = np.array([s["received"][1:] for s in states], np.int64)
    for f in ("n_tx", "commands", "substeps"):
        out[f] = np.array([s[f] for s in states], np.int64)
    for f in ("noise_key", "noise_count", "loss_key", "loss_count"):
        out[f] = np.array([s[f] for s in states], np.uint64)
    for f in ("loss", "lost"):
        out[f] = np.array([s[f] for s in states], np.uint32)
    return out


@pytest.mark.gpu
def test_set_loss_with_a_mask_mid_run_touches_the_masked_records_and_nothing_else():
    N, K0, K, start, period = 70, 35, 70, 20, 10
    gi, so, _, _ = step_layout(N)
    dev, dur, steps, _ = lm.step_streams(None, K, 1, start, period)
    env = step_env(N, start, period)
    run_steps(env, dev, dur, steps, gi, so, 0, K0, every=False)
    before = state_of(env)
    assert (before["loss_count"] > 0).all()
    mask = np.zeros(N, np.uint8)
    mask[list(MASKED)] = 1
    m = mask.astype(bool)
    keys = _new_keys(N)
    env.set_loss(NEW_P, keys, mask=T(mask))
    after = state_of(env)
    for f in LOSS_STATE:
        if f not in lm.LOSS_FIELDS:
            assert_same(after[f], before[f], ("running state", f))
        else:
            assert_same(after[f][~m], before[f][~m], ("other envs", f))
    assert_same(after["loss"][m], np.tile(np.array(NEW_THR, np.uint32), (m.sum(), 1)), "masked thresholds")
    assert_same(after["loss_key"][m], keys[m], "masked keys")
    assert (after["loss_count"][m] == 0).all() and (after["lost"][m] == 0).all()
    run_steps(env, dev, dur, steps, gi, so, K0, K, every=False)
    st = state_of(env, MODEL_FIELDS)
    want = _masked_models(K0, K, start, period)
    for f in MODEL_FIELDS:
        assert_same(st[f][~m], steps[-1][f][gi, so][~m], ("other envs", f))       # as if nothing had happened
        assert_same(st[f][m], want[f], ("masked envs", f))                         # their own past, the new record from K0 on
    assert (st["loss_count"][m] < st["n_tx"][m]).all()
    env.close()


@pytest.mark.gpu
def test_reset_leaves_thresholds_key_and_counts_and_the_erasures_continue_the_sequence():
    N, K0, K, start, period = 70, 35, 70, 20, 10
    gi, so, _, _ = step_layout(N)
    dev, dur, steps, _ = lm.step_streams(None, K, 1, start, period)
    env = step_env(N, start, period)
    run_steps(env, dev, dur, steps, gi, so, 0, K0, every=False)
    before = state_of(env)
    mask = np.zeros(N, np.uint8)
    mask[list(MASKED)] = 1
    m = mask.astype(bool)
    env.reset_envs(T(mask))
    after = state_of(env)
    for f in LOSS_STATE:
        assert_same(after[f][~m], before[f][~m], ("untouched", f))
    for f in lm.LOSS_FIELDS + ("disturbance", "noise_key", "noise_count", "gains"):
        assert_same(after[f], before[f], ("survives a reset", f))
    assert (after["now"][m] == 0).all() and (after["n_tx"][m] == 0).all() and (after["loss_count"][m] > 0).all()
    run_steps(env, dev, dur, steps, gi, so, K0, K, every=False)
    st = state_of(env, MODEL_FIELDS)
    want = _masked_models(K0, K, start, period, reset=True)
    for f in MODEL_FIELDS:
        assert_same(st[f][~m], steps[-1][f][gi, so][~m], ("other envs", f))
        assert_same(st[f][m], want[f], ("reset envs: fresh models, the old models' records", f))
    assert (st["loss_count"][m] > st["n_tx"][m]).all()
    env.close()


# ---- 10. every announcement lost ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_with_every_announcement_erased_nothing_is_ever_received():
    K, max_steps = lm.STEPS, lm.MAX_STEPS
    _, gi, _, _ = pm.fused_layout()
    sch = g.schedules_of(pm.P, pm.ROLLOUT_L)
    env = fused_env()
    tally, _ = env.rollout_schedules(T(sch), (max_steps, lm.FAIL_DEG), K)
    st = state_of(env)
    sel = gi == lm.ALL_LOST
    assert sel.sum() == 64 and (st["loss"][sel][:, :2] == 0xFFFFFFFF).all()
    assert not (st["flags"][sel] & 3).any()                                     # no step of these envs was flagged
    assert (st["received"][sel] == 0).all()
    count = st["loss_count"][sel]
    assert_same(count, (st["lost"][sel][:, 0].astype(np.uint64) + st["lost"][sel][:, 1].astype(np.uint64)), "every draw an erased announcement")
    assert (count == K).all() and (st["lost"][sel][:, 2:] == 0).all()           # one announcement per unflagged step, no data packet
    assert (tally.cpu().numpy()[sel][:, 2] == K).all()
    assert (st["received"][gi == 0] > 0).any()
    env.close()


# ---- 11. refusals and surface ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_set_loss_refusals_come_before_any_launch_and_the_env_has_the_new_verbs():
    import torch
    import gymwipe_amd
    from gymwipe_amd import _native as nat
    from gymwipe_amd import actions
    N = 128
    env = gymwipe_amd.make("VecControlLoop-v0", num_envs=N)
    assert callable(env.set_loss)
    for f, shape, dt in (("loss", (N, 4), np.uint32), ("loss_key", (N,), np.uint64), ("loss_count", (N,), np.uint64), ("lost", (N, 4), np.uint32)):
        assert env.get_state(f).shape == shape and env.get_state(f).dtype == dt and (env.get_state(f) == 0).all()
    L = nat.lib()
    some = torch.zeros((N, 4), dtype=torch.int32, device="cuda")
    keys = torch.zeros(N, dtype=torch.int64, device="cuda")
    before = state_of(env)
    assert L.gw_ctrl_set_loss(None, some.data_ptr(), keys.data_ptr(), None, None) == nat.EINVAL
    assert L.gw_ctrl_set_loss(env._h, None, keys.data_ptr(), None, None) == nat.EINVAL
    assert L.gw_ctrl_set_loss(env._h, some.data_ptr(), None, None, None) == nat.EINVAL
    for args, word in (((env._h, None, keys.data_ptr(), None, None), "thr_dev"), ((env._h, some.data_ptr(), None, None, None), "key_dev")):
        with pytest.raises(nat.NativeError) as err:
            nat.check(L.gw_ctrl_set_loss(*args))
        assert err.value.code == nat.EINVAL and word in str(err.value)
    for bad_p, bad_key in (([0.1, 0.0, 0.0], None), (np.zeros((N - 1, 4)), None), (np.zeros(4), np.zeros(N, np.int64)),
                           (np.zeros(4), np.zeros(N - 1, np.uint64)), (np.zeros(4), torch.zeros(N, dtype=torch.int32)),
                           (np.array(["a", "b", "c", "d"]), None)):
        with pytest.raises(ValueError):
            env.set_loss(bad_p, bad_key)
    assert_states_equal(state_of(env), before, "refused")
    # the refusals switched nothing: the handle still walks with an untouched one
    twin = gymwipe_amd.make("VecControlLoop-v0", num_envs=N)
    act = {"device": torch.zeros(N, dtype=torch.int32), "duration": torch.full((N,), 19, dtype=torch.int32)}
    env.step(act), twin.step(act)
    for f in ALL_FIELDS:
        assert_same(env.get_state(f), twin.get_state(f), ("unswitched", f))
    twin.close()
    top = np.full(N, 0x8000000000000001, np.uint64)      # keys with the top bit set, both ways in; probabilities beyond [0, 1]
    env.set_loss((0.0, 0.5, 2.0, -1.0), top, mask=torch.arange(N) < 64)
    env.set_loss(torch.full((N, 4), 2.0 ** -32, dtype=torch.float64, device="cuda"), T(top.view(np.int64) + 1).cuda(), mask=np.arange(N) >= 96)
    lo, hi = (np.arange(N) < 64), (np.arange(N) >= 96)
    want = np.where(lo[:, None], np.array([0, 2 ** 31, 2 ** 32 - 1, 0], np.uint32), np.where(hi[:, None], np.uint32(1), np.uint32(0)))
    assert_same(env.get_state("loss"), want.astype(np.uint32), "thresholds")
    assert_same(env.get_state("loss_key"), np.where(lo, top, np.where(hi, top + np.uint64(1), np.uint64(0))), "keys")
    buf = np.empty(N * 3)                                 # a wrong size is refused, as for every field
    for f in (b"loss", b"loss_key", b"loss_count", b"lost"):
        assert L.gw_ctrl_get_state(env._h, f, buf.ctypes.data, buf.nbytes) == nat.EFIELD
    env.close()
    env = gymwipe_amd.make("VecControlLoop-v0", num_envs=N, loss=(0.5, 0.5, 0.5, 0.5))
    assert (env.get_state("loss") == 2 ** 31).all()
    assert_same(env.get_state("loss_key"), actions.make_ctrl_loss(np.zeros(4), N)[1], "the default keys")
    assert (env.get_state("loss_key") != actions.make_ctrl_disturbance(np.zeros(4), N)[1]).all()      # not the disturbance's
    for _ in range(4):
        env.step(act)
    assert_same(env.get_state("loss_count"), env.get_state("n_tx").astype(np.uint64), "count")
    lost = env.get_state("lost")
    assert len({r.tobytes() for r in lost}) > N // 4     # the envs do not share one sequence
    r = actions.ctrl_loss_numpy(env.get_state("loss_key"), np.uint64(0))        # the first announcement of every env, by the helper
    assert r.dtype == np.uint32 and ((r < 2 ** 31) <= (lost[:, 0] >= 1)).all() and (r < 2 ** 31).any() and (r >= 2 ** 31).any()
    env.close()
