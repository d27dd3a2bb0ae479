"""The control loop beyond one step per launch, on the GPU: per-env initial states and reset (gw_ctrl_set_initial / gw_ctrl_reset),
K steps fused into one launch with optional episodes (gw_ctrl_rollout) and P cyclic schedules with a per-env tally
(gw_ctrl_rollout_schedules).  The specification is the event-driven ControlLoopModel with the episode rules restated in
tests/ctrl_episodes_model.py -- a reset env IS a freshly constructed model -- and every comparison is bit for bit.
Env e follows stream (5 e + e // 64) % 8 (tests/test_control_loop.py): 8 models stand for N envs.  The data the cases run on is
defined here and checked on the model alone in tests/test_ctrl_rollout_cpu.py (both ending causes occur, angles stay far below
the int32 observation's range)."""
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ctrl_episodes_model import FIELDS, EpisodicControlLoop, run_schedule
from ctrl_fixtures import (ALL_FIELDS, DENSE_CTRL, EP_SEED, PERIOD, START, STREAMS, U0S, X0S, T, assert_same, same_bits, schedules_of,
                           stream_of)
from ctrl_fixtures import rows_of as _rows
from test_control_loop import model_streams

EP_STEPS, EP_MAX, EP_FAIL = 60, 7, 90.0                         # test 3: max_steps does not divide the step count
SCHED_STEPS, SCHED_MAX, SCHED_FAIL = 60, 25, 90.0               # test 4


def wrapper(s, **kw):
    return EpisodicControlLoop(x0=X0S[s], u0=U0S[s], start=START, period=PERIOD, **kw)


@functools.lru_cache(maxsize=None)
def episode_streams():
    """Test 3's reference: STREAMS random action streams through one wrapper each, started from X0S / U0S.  Returns the actions
    [K][8], per step the outputs and ``ended``, and the state after the last step.  Computed once, never modified."""
    rng = np.random.default_rng(EP_SEED)
    dev = rng.integers(0, 2, (EP_STEPS, STREAMS)).astype(np.int32)
    dur = rng.integers(0, 20, (EP_STEPS, STREAMS)).astype(np.int32)
    envs = [wrapper(s) for s in range(STREAMS)]
    obs, rew = np.empty((EP_STEPS, STREAMS), np.int64), np.empty((EP_STEPS, STREAMS), np.float32)
    ang, ended = np.empty((EP_STEPS, STREAMS), np.float64), np.empty((EP_STEPS, STREAMS), np.uint8)
    for k in range(EP_STEPS):
        for s, env in enumerate(envs):
            o, r, a, e = env.step(dev[k, s], dur[k, s], EP_MAX, EP_FAIL)
            obs[k, s], rew[k, s], ang[k, s], ended[k, s] = o, np.float32(r), a, e
    final = _rows([env.state() for env in envs])
    for v in (dev, dur, obs, rew, ang, ended) + tuple(final.values()):
        v.setflags(write=False)
    return dev, dur, obs, rew, ang, ended, final


@functools.lru_cache(maxsize=None)
def schedule_streams(P, L):
    """Test 4's reference: schedule p on stream s for every (p, s).  Returns the tally [P][8][4], the actions taken
    [K][P][8] x 2 (the schedule expanded along each env's own ages), the states after the last step and the largest |angle|."""
    sch = schedules_of(P, L)
    tally = np.empty((P, STREAMS, 4), np.float64)
    dev, dur = np.empty((SCHED_STEPS, P, STREAMS), np.int32), np.empty((SCHED_STEPS, P, STREAMS), np.int32)
    states, worst = [], 0.0
    for p in range(P):
        for s in range(STREAMS):
            env = wrapper(s)
            tally[p, s], w, taken = run_schedule(env, sch[p], SCHED_STEPS, SCHED_MAX, SCHED_FAIL)
            dev[:, p, s], dur[:, p, s] = taken[:, 0], taken[:, 1]
            worst = max(worst, w)
            states.append(env.state())
    final = _rows(states)
    for v in (tally, dev, dur) + tuple(final.values()):
        v.setflags(write=False)
    return sch, tally, dev, dur, final, worst


def state_of(env, fields=ALL_FIELDS):
    return {f: env.get_state(f) for f in fields}


def assert_states_equal(a, b, what, fields=ALL_FIELDS):
    for f in fields:
        assert_same(a[f], b[f], (what, f))


def make_env(N, plant=None, own_states=False):
    """A handle on the test's plant; ``own_states``: every env gets its stream's X0S / U0S and starts from it."""
    import torch
    from gymwipe_amd import VecControlLoopEnv
    kw = {} if plant is None else {"A": DENSE_CTRL["A"], "B": DENSE_CTRL["B"], "x0": DENSE_CTRL["x0"], "u0": DENSE_CTRL["u0"]}
    env = VecControlLoopEnv(N, ctrl_start_tick=START, ctrl_period_ticks=PERIOD, **kw)
    if own_states:
        so = stream_of(N)
        env.set_initial_state(torch.from_numpy(X0S[so]), torch.from_numpy(U0S[so]))
        env.reset_envs()
    return env


# ---- 1. reset --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_reset_gives_masked_envs_a_fresh_model_and_leaves_the_others_alone():
    N, K = 200, 10
    so = stream_of(N)
    dev, dur, steps = model_streams(None, 40, 20, START, PERIOD)        # the first 10 and the next 10 steps of these streams
    env = make_env(N)
    for k in range(K):
        env.step({"device": T(dev[k][so]), "duration": T(dur[k][so])})
    env.set_initial_state(T(X0S[so]), T(U0S[so]))
    before = state_of(env)
    assert_same(before["x_init"], X0S[so], "x_init") and assert_same(before["u_init"], U0S[so], "u_init")
    for f in FIELDS:                                                     # set_initial_state moved no running state
        assert_same(before[f], steps[K - 1][f][so], ("before", f))
    e = np.arange(N)
    mask = ((e >= 37) & (e < 171) & (e % 3 != 0)).astype(np.uint8)       # starts and ends inside a wave, holes within
    m = mask.astype(bool)
    obs = env.reset_envs(T(mask)).cpu().numpy()
    after = state_of(env)
    fresh = _rows([wrapper(s).state() for s in range(STREAMS)])
    for f in ALL_FIELDS:
        assert_same(after[f][~m], before[f][~m], ("untouched", f))
    for f in FIELDS + ("age", "cost"):
        assert_same(after[f][m], fresh[f][so][m], ("fresh", f))
    assert_same(after["wake"][m], np.zeros(m.sum()), "wake")
    assert_same(after["flags"], before["flags"], "flags are sticky")
    want_obs = np.where(m, np.array([int(math.degrees(x[2])) for x in X0S])[so], steps[K - 1]["obs"][so])
    assert (obs == want_obs).all()
    # 10 further steps of all envs: the masked ones as fresh models of their own state, the others as if nothing had happened
    cont = [wrapper(s) for s in range(STREAMS)]
    for k in range(K, 2 * K):
        o, r, _, info = env.step({"device": T(dev[k][so]), "duration": T(dur[k][so])})
        fb = [c.step(dev[k, s], dur[k, s], episodes=False) for s, c in enumerate(cont)]
        st = _rows([c.state() for c in cont])
        got = state_of(env, FIELDS)
        for name, g, fresh_w, old_w in (("obs", o.cpu().numpy(), np.array([f[0] for f in fb]), steps[k]["obs"]),
                                        ("rew", r.cpu().numpy(), np.array([np.float32(f[1]) for f in fb], np.float32), steps[k]["rew"]),
                                        ("ang", info["Sensor angle"].cpu().numpy(), np.array([f[2] for f in fb]), steps[k]["ang"])):
            assert_same(g[m], fresh_w[so][m], (name, k)) and assert_same(g[~m], old_w[so][~m], (name, k))
        for f in FIELDS:
            assert_same(got[f][m], st[f][so][m], (f, k, "reset envs"))
            assert_same(got[f][~m], steps[k][f][so][~m], (f, k, "other envs"))
    assert (env.get_state("age") == 0).all() and (env.get_state("cost") == 0).all()     # step() keeps no episode record
    env.close()


# ---- 2. rollout equals steps ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("plant,seed", [(None, 20), ("dense", 21)])
def test_rollout_without_episodes_equals_k_steps(plant, seed):
    N, K = 200, 40
    so = stream_of(N)
    dev, dur, steps = model_streams(plant, K, seed, START, PERIOD)
    d, u = T(dev[:, so]), T(dur[:, so])
    one = make_env(N, plant)
    obs, rew, done, info = one.rollout(d, u)
    assert obs.shape == (K, N) and not done.any()
    got = {"obs": obs.cpu().numpy(), "rew": rew.cpu().numpy(), "ang": info["Sensor angle"].cpu().numpy()}
    for k in range(K):
        for f in ("obs", "rew", "ang"):
            assert_same(got[f][k], steps[k][f][so], (f, k))
    st = state_of(one)
    for f in FIELDS:
        assert_same(st[f], steps[-1][f][so], f)
    assert not (st["flags"] & 3).any() and (st["age"] == 0).all() and (st["cost"] == 0).all()
    twin = make_env(N, plant)                                            # the same by K calls of env.step
    for k in range(K):
        o, r, _, i = twin.step({"device": d[k], "duration": u[k]})
        assert_same(o.cpu().numpy(), got["obs"][k], k) and assert_same(r.cpu().numpy(), got["rew"][k], k)
        assert_same(i["Sensor angle"].cpu().numpy(), got["ang"][k], k)
    assert_states_equal(state_of(twin), st, "twin")
    halves = make_env(N, plant)                                          # two calls of K / 2
    a, b = halves.rollout(d[:K // 2], u[:K // 2]), halves.rollout(d[K // 2:], u[K // 2:])
    assert_same(np.concatenate([a[0].cpu().numpy(), b[0].cpu().numpy()]), got["obs"], "halves")
    assert_same(np.concatenate([a[3]["Sensor angle"].cpu().numpy(), b[3]["Sensor angle"].cpu().numpy()]), got["ang"], "halves")
    assert_states_equal(state_of(halves), st, "halves")
    for env in (one, twin, halves):
        env.close()


@pytest.mark.gpu
def test_rollout_flags_and_skips_an_action_outside_the_action_space_as_step_does():
    N, K = 200, 12
    so = stream_of(N)
    dev, dur, _ = model_streams(None, 40, 20, START, PERIOD)
    d, u = dev[:K, so].copy(), dur[:K, so].copy()
    d[5, ::3] = 2                                                        # the actuator is not assignable
    u[7, 1::5] = 20                                                      # one past the longest duration
    one, twin = make_env(N), make_env(N)
    obs, rew, _, info = one.rollout(T(d), T(u))
    for k in range(K):
        o, r, _, i = twin.step({"device": T(d[k]), "duration": T(u[k])})
        assert_same(obs[k].cpu().numpy(), o.cpu().numpy(), k) and assert_same(rew[k].cpu().numpy(), r.cpu().numpy(), k)
        assert_same(info["Sensor angle"][k].cpu().numpy(), i["Sensor angle"].cpu().numpy(), k)
    st = state_of(one)
    assert_states_equal(st, state_of(twin), "twin")
    bad = np.zeros(N, bool)
    bad[::3] = True
    bad[1::5] = True
    assert ((st["flags"] & 8) != 0).tolist() == bad.tolist()
    one.close(), twin.close()


# ---- 3. episodes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rollout_with_episodes_matches_the_wrapper_and_its_per_step_composition():
    N, K = 136, EP_STEPS
    so = stream_of(N)
    dev, dur, w_obs, w_rew, w_ang, w_ended, final = episode_streams()
    assert (w_ended & 1).any() and (w_ended & 2).any()
    d, u = T(dev[:, so]), T(dur[:, so])
    env = make_env(N, own_states=True)
    obs, rew, ended, info = env.rollout(d, u, episodes=(EP_MAX, EP_FAIL))
    got_ended = ended.cpu().numpy()
    assert_same(got_ended, w_ended[:, so], "ended")
    assert_same(obs.cpu().numpy(), w_obs[:, so], "obs") and assert_same(rew.cpu().numpy(), w_rew[:, so], "reward")
    assert_same(info["Sensor angle"].cpu().numpy(), w_ang[:, so], "angle")
    st = state_of(env)
    for f in FIELDS + ("age", "cost"):
        assert_same(st[f], final[f][so], f)
    assert not (st["flags"] & 3).any()
    # the same trajectory composed per step: step, the rule in numpy, reset_envs(mask)
    twin = make_env(N, own_states=True)
    age, cost = np.zeros(N, np.int64), np.zeros(N, np.float64)
    for k in range(K):
        o, r, _, i = twin.step({"device": d[k], "duration": u[k]})
        deg = i["Sensor angle"].cpu().numpy()
        assert_same(o.cpu().numpy(), w_obs[k][so], ("twin obs", k)) and assert_same(deg, w_ang[k][so], ("twin angle", k))
        age += 1
        cost = cost + np.abs(deg)
        cause = (age == EP_MAX).astype(np.uint8) | ((np.abs(deg) > EP_FAIL).astype(np.uint8) << 1)
        assert_same(cause, got_ended[k], ("twin ended", k))
        if cause.any():
            twin.reset_envs(T((cause != 0).astype(np.uint8)))
            age[cause != 0], cost[cause != 0] = 0, 0.0
    assert_states_equal(state_of(twin), st, "twin", tuple(f for f in ALL_FIELDS if f not in ("age", "cost")))
    assert_same(st["age"], age, "age") and assert_same(st["cost"], cost, "cost")
    # two calls of K / 2 equal one of K: age and cost live in the handle
    halves = make_env(N, own_states=True)
    a = halves.rollout(d[:K // 2], u[:K // 2], episodes=(EP_MAX, EP_FAIL))
    b = halves.rollout(d[K // 2:], u[K // 2:], episodes=(EP_MAX, EP_FAIL))
    assert_same(np.concatenate([a[2].cpu().numpy(), b[2].cpu().numpy()]), got_ended, "halves")
    assert_states_equal(state_of(halves), st, "halves")
    for e in (env, twin, halves):
        e.close()


@pytest.mark.gpu
def test_rollout_with_both_limits_off_is_the_plain_rollout_with_a_record():
    N, K = 200, 40
    so = stream_of(N)
    dev, dur, steps = model_streams(None, K, 20, START, PERIOD)
    env = make_env(N)
    obs, rew, ended, info = env.rollout(T(dev[:, so]), T(dur[:, so]), episodes=(0, 0.0))
    assert not ended.any()
    ang = info["Sensor angle"].cpu().numpy()
    cost = np.zeros(N)
    for k in range(K):
        assert_same(obs[k].cpu().numpy(), steps[k]["obs"][so], k) and assert_same(ang[k], steps[k]["ang"][so], k)
        cost = cost + np.abs(ang[k])
    st = state_of(env)
    for f in FIELDS:
        assert_same(st[f], steps[-1][f][so], f)
    assert (st["age"] == K).all()
    assert_same(st["cost"], cost, "cost")
    env.close()


# ---- 4. schedules ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("P,L", [(4, 3), (2, 64), (1, 1), (4, 1)])
def test_rollout_schedules_tally_matches_the_wrapper(P, L):
    N, K = 256, SCHED_STEPS
    M = N // P
    so = stream_of(N)
    p_of = np.arange(N) // M
    sch, w_tally, w_dev, w_dur, final, _ = schedule_streams(P, L)
    env = make_env(N, own_states=True)
    tally, sums = env.rollout_schedules(T(sch), (SCHED_MAX, SCHED_FAIL), K)
    tally, sums = tally.cpu().numpy(), sums.cpu().numpy()
    assert tally.shape == (N, 4) and sums.shape == (P, 4)
    assert_same(tally, w_tally[p_of, so], "tally")
    for p in range(P):
        mine = tally[p * M:(p + 1) * M]
        assert (sums[p, :3] == mine[:, :3].sum(0)).all() and sums[p, 2] == K * M          # counts are exact
        exact = math.fsum(mine[:, 3].tolist())
        assert abs(sums[p, 3] - exact) <= M * 2.0 ** -52 * exact, (p, sums[p, 3], exact)
    st = state_of(env)
    rows = p_of * STREAMS + so                                           # schedule_streams lists its states as [p][s]
    for f in FIELDS + ("age", "cost"):
        assert_same(st[f], final[f][rows], f)
    # the state after the call equals rollout with the same schedules expanded to [K][N] actions
    twin = make_env(N, own_states=True)
    twin.rollout(T(w_dev[:, p_of, so]), T(w_dur[:, p_of, so]), episodes=(SCHED_MAX, SCHED_FAIL))
    assert_states_equal(state_of(twin), st, "expanded")
    env.close(), twin.close()


@pytest.mark.gpu
def test_rollout_schedules_refuses_blocks_that_would_span_two_schedules():
    from gymwipe_amd import _native as nat
    env = make_env(192, own_states=True)
    before = state_of(env)
    with pytest.raises(nat.NativeError) as err:
        env.rollout_schedules(T(schedules_of(2, 3)), (SCHED_MAX, SCHED_FAIL), 10)
    assert err.value.code == nat.EUNSUPPORTED and "multiple of 64" in str(err.value)
    assert_states_equal(state_of(env), before, "refused")
    env.close()


# ---- 5. surface ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_control_loop_env_surface_has_the_new_verbs():
    import torch
    import gymwipe_amd
    N, K = 128, 6
    env = gymwipe_amd.make("VecControlLoop-v0", num_envs=N)
    for name in ("set_initial_state", "reset_envs", "rollout", "rollout_schedules"):
        assert callable(getattr(env, name))
    for f, shape in (("age", (N,)), ("cost", (N,)), ("x_init", (N, 4)), ("u_init", (N,))):
        assert env.get_state(f).shape == shape
    assert (env.get_state("x_init") == np.array([0.0, 0.0, 0.05, 0.0])).all() and (env.get_state("u_init") == 0.1).all()
    z = torch.zeros(N, dtype=torch.int32, device="cuda")
    assert (env.reset() == 2).all()                                      # reset() keeps the reference's meaning: nothing is reset
    obs, rew, done, info = env.step({"device": z, "duration": z + 7})
    assert env.reset() is obs and not done.any()
    now = env.get_state("now")
    assert (env.reset() == obs).all() and (env.get_state("now") == now).all() and (now > 0).all()
    out = (torch.empty((K, N), dtype=torch.int32, device="cuda"), torch.empty((K, N), dtype=torch.float32, device="cuda"),
           torch.empty((K, N), dtype=torch.uint8, device="cuda"), torch.empty((K, N), dtype=torch.float64, device="cuda"))
    ptrs = [t.data_ptr() for t in out]
    acts = torch.zeros((K, N), dtype=torch.int32, device="cuda")
    o, r, e, i = env.rollout(acts, acts + 3, episodes=(4, 0.0), out=out)
    assert [t.data_ptr() for t in (o, r, e, i["Sensor angle"])] == ptrs                  # written in place, not reallocated
    assert (e.cpu().numpy()[3] == 1).all() and e.cpu().numpy().sum() == N
    o2, _, _, _ = env.rollout(acts, acts + 3, out=out)
    assert o2.data_ptr() == ptrs[0]
    assert (env.reset_envs() == 2).all() and (env.get_state("now") == 0).all()
    env.set_initial_state([0.0, 0.0, 0.5, 0.0], u0=0.0, mask=torch.arange(N) < 64)       # a single state is broadcast
    assert (env.reset_envs().cpu().numpy() == np.where(np.arange(N) < 64, 28, 2)).all()
    env.close()
