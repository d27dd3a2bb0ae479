"""
gw_rollout_backlog on the GPU: the scored autoreset rollout with a queue-aware scheduler choosing the actions inside the launch
(ct_rollout_backlog<DT, MODE>), its per-step form, and what the call promises of both: replaying the chosen actions through
gw_rollout_autoreset_scored gives everything else again, calls continue one another, a capture replays.

Every expected value comes from the oracle alone: CtOracle + actions.backlog_sample_numpy + actions.score_numpy +
actions.episodes_numpy (oracle_backlog_steps() in tests/test_rollout_backlog_cpu.py).  All comparisons are exact: the eight
[K][N] rows and obs_next, {age, ret}, the tally, the state (STATE_FIELDS + STAT_FIELDS).  N = 200 is three full waves and a
partial one, K = 70 a launch of 64 steps and one of 6.  Fresh envs are identical and the scheduler is deterministic, so every
case begins with the prologue (six steps of seeded random actions, then a reset of every third env) on GPU and oracle alike;
backlog_reference() raises, instead of letting a test pass, when the prologue leaves the envs alike (at the default load every
queue soon sits at its cap and the envs then choose alike, but their clocks, counters and received values differ), when nothing
is delivered or when fewer than MIN_EPISODES episodes end in a case with a step limit.
tests/test_rollout_backlog_cpu.py checks on the CPU that INSTANTIATIONS is exactly the library's set.
"""
import functools

import numpy as np
import pytest

from test_kernel_variants import MODE_SWITCHES, NEAR_LIMIT, SFX_DTS, launches
from test_rollout_backlog_cpu import (CENTER, MODERATE, NAMES, PROLOGUE, case_policy, new_oracle, oracle_backlog_steps, oracle_prologue,
                                      prologue_actions, prologue_mask)
from util import assert_state_equal, STATE_FIELDS, STAT_FIELDS

N, K = 200, 70
MAX_STEPS, MIN_EPISODES = 5, 50
INSTANTIATIONS = {"ct_rollout_backlog<%d, %d>" % (dt, mode): (dt, mode) for dt in SFX_DTS + (0,) for mode in (2, 1, 0)}
# the cases that differ from their neighbours in more than the load: a sender that never produces, a start near the fast forms'
# validity limit (no mode switch: the host's bound on the clocks selects MODE 1 by itself, and lanes straddle the limit during
# the call), and a call without episodes
SPECIAL = {
    "ct_rollout_backlog<5, 2>": {"mult": (1, 3, 0, 2, 1)},
    "ct_rollout_backlog<4, 1>": {"start_time": NEAR_LIMIT, "switches": {}},
    "ct_rollout_backlog<6, 0>": {"max_steps": 0, "on_done": False},
}


def case_score(D):
    from gymwipe_amd.actions import make_score
    return make_score(D, reward=3, delivered=[(5 + 2 * d) * (-1 if d % 2 else 1) for d in range(D)])


def make_env(D, interval=None, mult=None, start_time=None, n=N, **kw):
    from gymwipe_amd import VecCounterTrafficEnv
    kw.setdefault("per_env_stats", True)
    return VecCounterTrafficEnv(n, num_devices=D, counter_interval=interval, multiplicity=mult, start_time=start_time, **kw)


def gpu_prologue(env):
    import torch
    dev, dur = prologue_actions(env.num_devices, env.num_envs)
    env.reset()
    for k in range(PROLOGUE):
        env.step({"device": torch.from_numpy(dev[k]), "duration": torch.from_numpy(dur[k])})
    env.reset(torch.from_numpy(prologue_mask(env.num_envs)))


@functools.lru_cache(maxsize=None)
def backlog_reference(D, interval=None, mult=None, start_time=None, max_steps=MAX_STEPS, on_done=True, steps=K):
    """The oracle's trajectory under case_policy(D) scored by case_score(D) behind the prologue, computed once and read only."""
    policy, score = case_policy(D), case_score(D)
    orc = new_oracle(D, N, interval, mult, start_time)
    oracle_prologue(orc)
    who = "backlog_reference(%s)" % ((D, interval, mult, start_time, max_steps, on_done, steps),)
    if len(np.unique(orc.get("now"))) < N // 2 or len(np.unique(orc.get("qlen"), axis=0)) < 3:
        raise RuntimeError("%s: the prologue leaves the envs alike" % who)
    state = np.zeros((N, 2), np.int32)
    out, obs_next, tally = oracle_backlog_steps(orc, policy, score, steps, state, max_steps, on_done)
    if int(out[4].sum()) == 0:
        raise RuntimeError("%s: no packet delivered" % who)
    if max_steps and tally[0] < MIN_EPISODES:
        raise RuntimeError("%s: %d episodes ended, fewer than %d" % (who, tally[0], MIN_EPISODES))
    for a in out + (obs_next, state, tally, policy, score):
        a.setflags(write=False)
    return {"policy": policy, "score": score, "out": out, "obs_next": obs_next, "state": state, "tally": tally, "orc": orc}


def assert_outputs(got, want, where, rows=slice(None)):
    assert len(got) == len(want) == 8
    for name, g, w in zip(NAMES, got, want):
        g, w = g.cpu().numpy(), w[rows]
        assert g.dtype == w.dtype and g.shape == w.shape, (name, where)
        assert (g.view(np.uint8) == w.view(np.uint8)).all(), \
            "%s differs %s, first at (step, env) %s" % (name, where, np.argwhere(g != w)[:3].tolist())


def assert_episodes(env, ref, where):
    assert (env._last[0].cpu().numpy() == ref["obs_next"]).all(), "obs_next differs " + where
    assert (env.episode_state.cpu().numpy() == ref["state"]).all(), "{age, ret} differs " + where
    assert env.episode_tally.cpu().numpy().tolist() == ref["tally"].tolist(), "tally differs " + where


def delta(after, before):
    return {k: v - before.get(k, 0) for k, v in after.items() if v != before.get(k, 0)}


def same_tensors(a, b):
    import torch
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


def assert_same_episodes(a, b):
    import torch
    assert torch.equal(a.episode_state, b.episode_state) and torch.equal(a.episode_tally, b.episode_tally)
    assert torch.equal(a._last[0], b._last[0])


# ---- 5. one case per instantiation ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(INSTANTIATIONS))
def test_instantiation_matches_the_oracle(name, monkeypatch):
    dt, mode = INSTANTIATIONS[name]
    D = dt if dt else 11
    case = dict(SPECIAL.get(name, {}))
    switches = case.pop("switches", MODE_SWITCHES[mode])
    for k, v in dict(switches, GW_ROLLOUT_STRICT="1").items():
        monkeypatch.setenv(k, v)
    interval = None if (SFX_DTS + (0,)).index(dt) % 2 else MODERATE     # the loads alternate: short queues, queues at the cap
    mult, start_time = case.get("mult"), case.get("start_time")
    max_steps, on_done = case.get("max_steps", MAX_STEPS), case.get("on_done", True)
    ref = backlog_reference(D, interval, mult, start_time, max_steps, on_done)
    env = make_env(D, interval, mult, start_time)
    gpu_prologue(env)
    before = launches(env)
    got = env.rollout_backlog(K, ref["policy"], max_steps=max_steps, on_done=on_done, score=ref["score"])
    assert_outputs(got, ref["out"], "under %s" % name)
    assert_episodes(env, ref, "after %s" % name)
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after %s" % name)
    assert delta(launches(env), before) == {name: 2}, launches(env)     # 64 + 6 steps of the target, no step or reset kernel
    if not max_steps and not on_done:
        assert int(got[3].sum()) == 0 and not ref["tally"].any()
    env.check()


def test_the_special_cases_cover_what_they_are_meant_to():
    assert set(SPECIAL) <= set(INSTANTIATIONS)
    assert 0 in SPECIAL["ct_rollout_backlog<5, 2>"]["mult"] and len(SPECIAL["ct_rollout_backlog<5, 2>"]["mult"]) == 5
    loads = {(SFX_DTS + (0,)).index(dt) % 2 for dt, _ in INSTANTIATIONS.values()}
    assert loads == {0, 1}


# ---- 6. replay --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("interval", [None, MODERATE], ids=["default load", "moderate load"])
def test_the_chosen_actions_replay_through_the_scored_autoreset_call(interval):
    """Two handles' snapshots differ only in the bytes that hold their own device addresses (tests/test_rollout_policy.py):
    after the scheduler on one and the replay of its actions on the other, no other byte may differ."""
    D = 4
    ref = backlog_reference(D, interval)
    env, twin = make_env(D, interval), make_env(D, interval)
    gpu_prologue(env)
    gpu_prologue(twin)
    own = env.snapshot() != twin.snapshot()
    assert own.sum() < 4096, own.sum()
    got = env.rollout_backlog(K, ref["policy"], max_steps=MAX_STEPS, score=ref["score"])
    assert_outputs(got, ref["out"], "by the scheduler")
    rep = twin.rollout_autoreset(got[5], got[6], max_steps=MAX_STEPS, score=ref["score"])
    assert same_tensors(rep, got[:5])
    assert_same_episodes(env, twin)
    assert_episodes(twin, ref, "after the replay")
    differ = env.snapshot() != twin.snapshot()
    assert not (differ & ~own).any(), np.flatnonzero(differ & ~own)[:8]
    assert set(delta(launches(twin), {})) >= {"ct_rollout_sync_eps<4, 2>"} and "ct_rollout_backlog<4, 2>" in launches(env)


@pytest.mark.gpu
def test_no_score_is_the_built_in_reward_and_no_policy_the_longest_queue():
    from gymwipe_amd.actions import backlog_sample_numpy, make_backlog_policy, make_score
    D = 4
    env, twin = make_env(D, MODERATE), make_env(D, MODERATE)
    gpu_prologue(env)
    gpu_prologue(twin)
    qlen = env.get_state("qlen")
    got = env.rollout_backlog(12, max_steps=MAX_STEPS)
    want = twin.rollout_backlog(12, make_backlog_policy(D), max_steps=MAX_STEPS, score=make_score(D))
    assert same_tensors(got, want)
    assert_same_episodes(env, twin)
    for g, w in zip((got[5][0], got[6][0], got[7][0]), backlog_sample_numpy(make_backlog_policy(D), qlen, 20)):
        assert (g.cpu().numpy() == w).all()
    assert (got[7][0].cpu().numpy() == qlen.max(axis=1)).all() and int(got[4].sum()) > 0


# ---- 7. the per-step form ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_per_step_form_equals_the_fused_one(monkeypatch):
    D = 4
    ref = backlog_reference(D, MODERATE)
    fused, unfused = make_env(D, MODERATE), make_env(D, MODERATE)
    gpu_prologue(fused)
    gpu_prologue(unfused)
    own = fused.snapshot() != unfused.snapshot()
    assert own.sum() < 4096, own.sum()
    bytes_f, bytes_u, before = fused.state_bytes(), unfused.state_bytes(), launches(unfused)
    a = fused.rollout_backlog(K, ref["policy"], max_steps=MAX_STEPS, score=ref["score"])
    monkeypatch.setenv("GW_ROLLOUT_POLICY_UNFUSED", "1")                # read per call
    b = unfused.rollout_backlog(K, ref["policy"], max_steps=MAX_STEPS, score=ref["score"])
    monkeypatch.delenv("GW_ROLLOUT_POLICY_UNFUSED")
    assert unfused.state_bytes() == bytes_u + 4 * N and fused.state_bytes() == bytes_f
    assert_outputs(a, ref["out"], "in the fused form")
    assert_outputs(b, ref["out"], "in the per-step form")
    assert_same_episodes(fused, unfused)
    assert_episodes(unfused, ref, "after the per-step form")
    differ = fused.snapshot() != unfused.snapshot()
    assert not (differ & ~own).any(), np.flatnonzero(differ & ~own)[:8]
    assert_state_equal(unfused, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after the per-step form")
    ran = delta(launches(unfused), before)
    assert not [k for k in ran if k.startswith("ct_rollout")] and sum(v for k, v in ran.items() if k.startswith("ct_step")) == K, ran
    # a second pair of calls continues both alike, and the scratch row was allocated once, on the per-step handle only
    a = fused.rollout_backlog(7, ref["policy"], max_steps=MAX_STEPS, score=ref["score"])
    monkeypatch.setenv("GW_ROLLOUT_POLICY_UNFUSED", "1")
    b = unfused.rollout_backlog(7, ref["policy"], max_steps=MAX_STEPS, score=ref["score"])
    monkeypatch.delenv("GW_ROLLOUT_POLICY_UNFUSED")
    assert same_tensors(a, b)
    assert_same_episodes(fused, unfused)
    assert unfused.state_bytes() == bytes_u + 4 * N and fused.state_bytes() == bytes_f
    differ = fused.snapshot() != unfused.snapshot()
    assert not (differ & ~own).any(), np.flatnonzero(differ & ~own)[:8]


@pytest.mark.gpu
def test_a_per_env_geometry_handle_always_takes_the_per_step_form(monkeypatch):
    D, steps = 4, 24
    policy, score = case_policy(D), case_score(D)
    a, b = make_env(D, MODERATE, per_env_geometry=True), make_env(D, MODERATE, per_env_geometry=True)
    for env in (a, b):
        gpu_prologue(env)
        env.set_position(0, 0.5, 1.5)
    own = a.snapshot() != b.snapshot()
    assert own.sum() < 4096, own.sum()
    bytes0 = a.state_bytes()
    ra = a.rollout_backlog(steps, policy, max_steps=MAX_STEPS, score=score)
    monkeypatch.setenv("GW_ROLLOUT_POLICY_UNFUSED", "1")
    rb = b.rollout_backlog(steps, policy, max_steps=MAX_STEPS, score=score)
    monkeypatch.delenv("GW_ROLLOUT_POLICY_UNFUSED")
    assert same_tensors(ra, rb)
    assert_same_episodes(a, b)
    differ = a.snapshot() != b.snapshot()
    assert not (differ & ~own).any(), np.flatnonzero(differ & ~own)[:8]
    assert a.state_bytes() == b.state_bytes() == bytes0 + 4 * N
    assert not [k for k in list(launches(a)) + list(launches(b)) if k.startswith("ct_rollout")]
    assert int(ra[4].sum()) > 0 and int(a.episode_tally[0]) >= MIN_EPISODES and len(np.unique(ra[5].cpu().numpy())) > 1
    # the choice is what the restatement makes of the handle's own queue lengths
    from gymwipe_amd.actions import backlog_sample_numpy
    qlen = a.get_state("qlen")
    nxt = a.rollout_backlog(1, policy, max_steps=MAX_STEPS, score=score)
    for g, w in zip((nxt[5][0], nxt[6][0], nxt[7][0]), backlog_sample_numpy(policy, qlen, 20)):
        assert (g.cpu().numpy() == w).all()


# ---- 8. chunking and capture ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pieces", [(70,), (64, 6), (1,) * K], ids=["70", "64+6", "70x1"])
def test_split_calls_equal_one_call(pieces):
    import torch
    D = 4
    ref = backlog_reference(D, MODERATE)
    env = make_env(D, MODERATE)
    gpu_prologue(env)
    kinds = (torch.int32, torch.float32, torch.uint8, torch.uint8, torch.int32, torch.int32, torch.int32, torch.int32)
    rows = tuple(torch.empty((K, N), dtype=t, device="cuda") for t in kinds)
    s = 0
    for n in pieces:
        out = tuple(r[s:s + n] for r in rows)
        back = env.rollout_backlog(n, ref["policy"], max_steps=MAX_STEPS, score=ref["score"], out=out)
        assert len(back) == 8 and all(x is y for x, y in zip(back, out))
        s += n
    assert_outputs(rows, ref["out"], "over calls of %s steps" % (pieces[:3],))
    assert_episodes(env, ref, "after the split calls")
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after the split calls")


@pytest.mark.gpu
def test_a_captured_call_of_8_steps_replayed_three_times_equals_24_eager_steps():
    """A linear capture on a side stream: nothing of the call but its pointers, limits, policy and weights is baked in, so
    every replay continues from the arrays' current contents."""
    import torch
    D, G = 4, 8
    ref = backlog_reference(D, MODERATE, steps=3 * G)
    kinds = (torch.int32, torch.float32, torch.uint8, torch.uint8, torch.int32, torch.int32, torch.int32, torch.int32)
    g = make_env(D, MODERATE)
    gpu_prologue(g)
    g.episode_state                                                     # (first use allocates the episode tensors)
    out = tuple(torch.empty((G, N), dtype=t, device="cuda") for t in kinds)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        g.rollout_backlog(G, ref["policy"], max_steps=MAX_STEPS, score=ref["score"], out=out)
    assert launches(g).get("ct_rollout_backlog<4, 1>") == 1, launches(g)
    for i in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert_outputs(out, ref["out"], "in replay %d" % i, slice(i * G, (i + 1) * G))
    assert_episodes(g, ref, "after three replays")
    assert_state_equal(g, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after three replays")


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("strict", [False, True])
def test_an_explicit_queue_handle_is_refused(strict, monkeypatch):
    from gymwipe_amd import _native as nat
    D = 3
    env = make_env(D, explicit_queue=True)
    env.reset()
    if strict:
        monkeypatch.setenv("GW_ROLLOUT_STRICT", "1")
    bytes0, before = env.state_bytes(), launches(env)
    with pytest.raises(nat.NativeError) as exc:
        env.rollout_backlog(4, max_steps=MAX_STEPS)
    assert exc.value.code == nat.EUNSUPPORTED
    assert launches(env) == before and env.state_bytes() == bytes0


@pytest.mark.gpu
def test_a_handle_without_the_fused_form_is_refused_under_strict(monkeypatch):
    """(GW_ROLLOUT_CAP is read when the handle is created.)"""
    from gymwipe_amd import _native as nat
    D = 4
    monkeypatch.setenv("GW_ROLLOUT_CAP", "0")
    env = make_env(D, MODERATE)
    monkeypatch.delenv("GW_ROLLOUT_CAP")
    gpu_prologue(env)
    bytes0, before = env.state_bytes(), launches(env)
    monkeypatch.setenv("GW_ROLLOUT_STRICT", "1")
    with pytest.raises(nat.NativeError) as exc:
        env.rollout_backlog(4, max_steps=MAX_STEPS)
    assert exc.value.code == nat.EUNSUPPORTED
    assert launches(env) == before and env.state_bytes() == bytes0      # before anything was launched or allocated
    monkeypatch.delenv("GW_ROLLOUT_STRICT")
    ref = backlog_reference(D, MODERATE)
    got = env.rollout_backlog(K, ref["policy"], max_steps=MAX_STEPS, score=ref["score"])    # without the switch: per step
    assert_outputs(got, ref["out"], "on a handle with rollout capacity 0")
    assert env.state_bytes() == bytes0 + 4 * N and not [k for k in launches(env) if k.startswith("ct_rollout")]
