"""
gw_rollout_backlog_population on the GPU: P policies of the queue-aware scheduler, read from device memory, on N / P envs each
in one launch per 64 steps (ct_rollout_backlog_pop<DT, MODE>), its per-step form, and what the call promises of both: every
env fares as under gw_rollout_backlog with its slice's policy, calls continue one another, a capture replays with whatever
policies the array holds then.

Every expected value comes from the oracle alone: CtOracle + actions.backlog_sample_population_numpy + actions.score_numpy +
actions.episodes_numpy, over all envs and again per slice (oracle_population_steps() in tests/test_backlog_population_cpu.py).
All comparisons are exact: the [P][5] tally, the call-wide tally, {age, ret}, obs_next, the state (STATE_FIELDS + STAT_FIELDS).
N = 256 is four policies of one wave each, K = 70 a launch of 64 steps and one of 6.  Every case begins with the parent's
prologue on GPU and oracle alike; population_reference() raises, instead of letting a test pass, when the prologue leaves the
envs alike, when a policy delivers nothing, when a policy ends fewer episodes than the step limit alone must end in its slice
(M * (steps // max_steps)), or when all policies fare alike.
tests/test_backlog_population_cpu.py checks on the CPU that INSTANTIATIONS is exactly the library's set.
"""
import functools

import numpy as np
import pytest

from test_kernel_variants import MODE_SWITCHES, NEAR_LIMIT, SFX_DTS, launches
from test_rollout_backlog_cpu import MODERATE, new_oracle, oracle_prologue
from test_rollout_backlog import assert_same_episodes, delta, gpu_prologue, make_env
from test_backlog_population_cpu import case_population, oracle_population_steps
from util import assert_state_equal, STATE_FIELDS, STAT_FIELDS

N, K, P = 256, 70, 4
MAX_STEPS = 5
INSTANTIATIONS = {"ct_rollout_backlog_pop<%d, %d>" % (dt, mode): (dt, mode) for dt in SFX_DTS + (0,) for mode in (2, 1, 0)}
# as the parent's: a sender that never produces, a start near the fast forms' validity limit (no mode switch: the host's bound
# on the clocks selects MODE 1 by itself), and a call without episodes
SPECIAL = {
    "ct_rollout_backlog_pop<5, 2>": {"mult": (1, 3, 0, 2, 1)},
    "ct_rollout_backlog_pop<4, 1>": {"start_time": NEAR_LIMIT, "switches": {}},
    "ct_rollout_backlog_pop<6, 0>": {"max_steps": 0, "on_done": False},
}


def case_score(D):
    from gymwipe_amd.actions import make_score
    return make_score(D, reward=3, delivered=[(5 + 2 * d) * (-1 if d % 2 else 1) for d in range(D)])


@functools.lru_cache(maxsize=None)
def population_reference(D, interval=None, mult=None, start_time=None, max_steps=MAX_STEPS, on_done=True, steps=K, n=N, policies=P,
                         live=False):
    """The oracle's trajectory under case_population(D, policies) scored by case_score(D) behind the prologue, computed once and
    read only.  (live: the same oracle; the handle it is compared with evaluates the PHY per env.)"""
    population, score = case_population(D, policies), case_score(D)
    M = n // policies
    assert M * policies == n
    orc = new_oracle(D, n, interval, mult, start_time)
    oracle_prologue(orc)
    who = "population_reference(%s)" % ((D, interval, mult, start_time, max_steps, on_done, steps, n, policies),)
    if len(np.unique(orc.get("now"))) < n // 2 or len(np.unique(orc.get("qlen"), axis=0)) < 3:
        raise RuntimeError("%s: the prologue leaves the envs alike" % who)
    state = np.zeros((n, 2), np.int32)
    out, obs_next, tally, tallies = oracle_population_steps(orc, population, M, score, steps, state, max_steps, on_done)
    packets = out[4].reshape(steps, policies, M).sum(axis=(0, 2))
    if (packets == 0).any():
        raise RuntimeError("%s: a policy delivers nothing: %s" % (who, packets.tolist()))
    if max_steps and (tallies[:, 0] < M * (steps // max_steps)).any():
        raise RuntimeError("%s: a policy ends fewer than %d episodes: %s" % (who, M * (steps // max_steps), tallies[:, 0].tolist()))
    fares = [tuple(tallies[p]) + (int(packets[p]), state[p * M:(p + 1) * M].tobytes()) for p in range(policies)]
    if policies > 1 and len(set(fares)) == 1:
        raise RuntimeError("%s: all policies fare alike" % who)
    for a in (obs_next, state, tally, tallies, population, score):
        a.setflags(write=False)
    return {"population": population, "score": score, "M": M, "obs_next": obs_next, "state": state, "tally": tally, "tallies": tallies,
            "orc": orc, "packets": packets}


def assert_population(env, got, ref, where):
    assert got.dtype.is_floating_point is False and tuple(got.shape) == ref["tallies"].shape, where
    assert got.cpu().numpy().tolist() == ref["tallies"].tolist(), "the [P][5] tally differs " + where
    assert env.episode_tally.cpu().numpy().tolist() == ref["tally"].tolist(), "the call-wide tally differs " + where
    assert (env.episode_state.cpu().numpy() == ref["state"]).all(), "{age, ret} differs " + where
    assert (env._last[0].cpu().numpy() == ref["obs_next"]).all(), "obs_next differs " + where
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where=where)


def snapshots_differ_only_in(a, b, own):
    differ = a.snapshot() != b.snapshot()
    assert not (differ & ~own).any(), np.flatnonzero(differ & ~own)[:8]


# ---- 1. one case per instantiation ------------------------------------------------------------------------------------------------
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
    ref = population_reference(D, interval, mult, start_time, max_steps, on_done)
    env = make_env(D, interval, mult, start_time, n=N)
    gpu_prologue(env)
    before = launches(env)
    got = env.rollout_backlog_population(ref["population"], K, max_steps=max_steps, on_done=on_done, score=ref["score"])
    assert_population(env, got, ref, "after %s" % name)
    assert delta(launches(env), before) == {name: 2}, launches(env)     # 64 + 6 steps of the target, no step or reset kernel
    if not max_steps and not on_done:
        assert not got.any() and not ref["tally"].any()
    env.check()


def test_the_special_cases_cover_what_they_are_meant_to():
    assert set(SPECIAL) <= set(INSTANTIATIONS)
    assert 0 in SPECIAL["ct_rollout_backlog_pop<5, 2>"]["mult"] and len(SPECIAL["ct_rollout_backlog_pop<5, 2>"]["mult"]) == 5
    assert {(SFX_DTS + (0,)).index(dt) % 2 for dt, _ in INSTANTIATIONS.values()} == {0, 1}


# ---- 2. slices and blocks -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_policy_that_spans_two_blocks(monkeypatch):
    monkeypatch.setenv("GW_ROLLOUT_STRICT", "1")
    D = 4
    ref = population_reference(D, MODERATE, policies=2)
    assert ref["M"] == 128
    env = make_env(D, MODERATE, n=N)
    gpu_prologue(env)
    got = env.rollout_backlog_population(ref["population"], K, max_steps=MAX_STEPS, score=ref["score"])
    assert_population(env, got, ref, "with two policies of 128 envs")


@pytest.mark.gpu
@pytest.mark.parametrize("interval", [None, MODERATE], ids=["default load", "moderate load"])
def test_one_policy_is_rollout_backlog_bit_for_bit(interval, monkeypatch):
    import torch
    monkeypatch.setenv("GW_ROLLOUT_STRICT", "1")
    D = 4
    ref = population_reference(D, interval, policies=1)
    env, twin = make_env(D, interval, n=N), make_env(D, interval, n=N)
    gpu_prologue(env)
    gpu_prologue(twin)
    own = env.snapshot() != twin.snapshot()
    assert own.sum() < 4096, own.sum()
    got = env.rollout_backlog_population(ref["population"], K, max_steps=MAX_STEPS, score=ref["score"])
    out = twin.rollout_backlog(K, ref["population"][0, :-3], max_steps=MAX_STEPS, score=ref["score"])
    assert_population(env, got, ref, "with one policy")
    assert_same_episodes(env, twin)
    assert torch.equal(got[0], twin.episode_tally) and int(out[4].sum()) == int(ref["packets"][0])
    snapshots_differ_only_in(env, twin, own)


# ---- 3. the per-step form -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_per_step_form_with_slices_of_50_envs_matches_the_oracle(monkeypatch):
    """M = 50 on N = 200: the selection's and the bookkeeping's blocks of 256 span policies, the last wave is partial."""
    from gymwipe_amd import _native as nat
    D, n = 4, 200
    ref = population_reference(D, MODERATE, n=n)
    assert ref["M"] == 50
    env = make_env(D, MODERATE, n=n)
    gpu_prologue(env)
    bytes0, before = env.state_bytes(), launches(env)
    monkeypatch.setenv("GW_ROLLOUT_STRICT", "1")
    with pytest.raises(nat.NativeError) as exc:
        env.rollout_backlog_population(ref["population"], K, max_steps=MAX_STEPS, score=ref["score"])
    assert exc.value.code == nat.EUNSUPPORTED
    assert launches(env) == before and env.state_bytes() == bytes0      # before anything was launched or allocated
    monkeypatch.delenv("GW_ROLLOUT_STRICT")
    got = env.rollout_backlog_population(ref["population"], K, max_steps=MAX_STEPS, score=ref["score"])
    assert_population(env, got, ref, "in the per-step form with M = 50")
    ran = delta(launches(env), before)
    assert not [k for k in ran if k.startswith("ct_rollout")] and sum(v for k, v in ran.items() if k.startswith("ct_step")) == K, ran
    assert env.state_bytes() == bytes0 + 4 * (4 * n + (n + 1) // 2) + 4 * n         # the six scratch rows and the counters' copy


@pytest.mark.gpu
def test_the_per_step_form_equals_the_fused_one(monkeypatch):
    import torch
    D = 4
    ref = population_reference(D, MODERATE)
    fused, unfused = make_env(D, MODERATE, n=N), make_env(D, MODERATE, n=N)
    gpu_prologue(fused)
    gpu_prologue(unfused)
    own = fused.snapshot() != unfused.snapshot()
    assert own.sum() < 4096, own.sum()
    bytes_f, before = fused.state_bytes(), launches(unfused)
    a = fused.rollout_backlog_population(ref["population"], K, max_steps=MAX_STEPS, score=ref["score"])
    monkeypatch.setenv("GW_ROLLOUT_POLICY_UNFUSED", "1")                # read per call
    b = unfused.rollout_backlog_population(ref["population"], K, max_steps=MAX_STEPS, score=ref["score"])
    monkeypatch.delenv("GW_ROLLOUT_POLICY_UNFUSED")
    assert fused.state_bytes() == bytes_f
    assert_population(fused, a, ref, "in the fused form")
    assert_population(unfused, b, ref, "in the per-step form")
    assert torch.equal(a, b)
    assert_same_episodes(fused, unfused)
    snapshots_differ_only_in(fused, unfused, own)                       # the header's clock bound included
    ran = delta(launches(unfused), before)
    assert not [k for k in ran if k.startswith("ct_rollout")] and sum(v for k, v in ran.items() if k.startswith("ct_step")) == K, ran
    # a second pair of calls continues both alike, adding into the callers' tallies
    a = fused.rollout_backlog_population(ref["population"], 7, max_steps=MAX_STEPS, score=ref["score"], tally=a)
    monkeypatch.setenv("GW_ROLLOUT_POLICY_UNFUSED", "1")
    b = unfused.rollout_backlog_population(ref["population"], 7, max_steps=MAX_STEPS, score=ref["score"], tally=b)
    monkeypatch.delenv("GW_ROLLOUT_POLICY_UNFUSED")
    assert torch.equal(a, b) and (a[:, 0].cpu().numpy() > ref["tallies"][:, 0]).all()
    assert_same_episodes(fused, unfused)
    snapshots_differ_only_in(fused, unfused, own)


@pytest.mark.gpu
def test_a_live_phy_handle_takes_the_per_step_form_and_matches_the_oracle():
    D, n = 3, 100
    ref = population_reference(D, MODERATE, n=n, live=True)
    assert ref["M"] == 25
    env = make_env(D, MODERATE, n=n, per_env_geometry=True)
    gpu_prologue(env)
    got = env.rollout_backlog_population(ref["population"], K, max_steps=MAX_STEPS, score=ref["score"])
    assert_population(env, got, ref, "on a live-PHY handle")
    assert not [k for k in launches(env) if k.startswith("ct_rollout")]


@pytest.mark.gpu
@pytest.mark.parametrize("strict", [False, True])
def test_an_explicit_queue_handle_is_refused(strict, monkeypatch):
    from gymwipe_amd import _native as nat
    from gymwipe_amd.actions import make_backlog_policy, make_backlog_population
    D = 3
    env = make_env(D, explicit_queue=True, n=N)
    env.reset()
    if strict:
        monkeypatch.setenv("GW_ROLLOUT_STRICT", "1")
    bytes0, before = env.state_bytes(), launches(env)
    with pytest.raises(nat.NativeError) as exc:
        env.rollout_backlog_population(make_backlog_population([make_backlog_policy(D)] * 4), 4, max_steps=MAX_STEPS)
    assert exc.value.code == nat.EUNSUPPORTED
    assert launches(env) == before and env.state_bytes() == bytes0


# ---- 4. continuation, unvalidated weights, capture ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_calls_of_30_and_40_steps_equal_one_of_70(monkeypatch):
    monkeypatch.setenv("GW_ROLLOUT_STRICT", "1")
    D = 4
    ref = population_reference(D, MODERATE)
    env = make_env(D, MODERATE, n=N)
    gpu_prologue(env)
    tally = env.rollout_backlog_population(ref["population"], 30, max_steps=MAX_STEPS, score=ref["score"])
    back = env.rollout_backlog_population(ref["population"], 40, max_steps=MAX_STEPS, score=ref["score"], tally=tally)
    assert back is tally
    assert_population(env, tally, ref, "after calls of 30 and 40 steps")


@pytest.mark.gpu
@pytest.mark.parametrize("unfused", [False, True], ids=["fused", "per step"])
def test_weights_outside_their_bounds_are_clamped_where_they_are_read(unfused, monkeypatch):
    """-5 counts as 0 and 5000 as 1024, in both forms: the device array is never validated."""
    import torch
    from gymwipe_amd import actions
    from test_rollout_backlog_cpu import oracle_chosen_steps
    D, steps = 4, 24
    raw = case_population(D, P).copy()
    w = raw[:, :4 * actions.MAX_DEVICES].view("<i4")
    w[0, :D] = [-5, 2, 1, 5000]             # as [0, 2, 1, 1024]
    w[1, :D] = [400, 5000, -5, 300]         # as [400, 1024, 0, 300]: 400 x 3 > 1024 x 1, where 5000 x 1 would still win
    w[2, :D] = [-(2 ** 31), 1, 2 ** 31 - 1, 1]
    valid = raw.copy()
    valid[:, :4 * actions.MAX_DEVICES].view("<i4")[:] = np.clip(w, 0, actions.SCORE_W_MAX)
    score = case_score(D)
    orc = new_oracle(D, N, MODERATE)
    oracle_prologue(orc)
    state = np.zeros((N, 2), np.int32)
    out, obs_next, tally, tallies = oracle_population_steps(orc, raw, N // P, score, steps, state, MAX_STEPS, True)
    chosen = actions.backlog_sample_population_numpy(raw, N // P, np.full((N, D), 3), 20)[0]
    assert chosen.reshape(P, -1)[:3, 0].tolist() == [3, 1, 2] and int(out[4].sum()) > 0 and (tallies[:, 0] > 0).all()
    scaled = valid.copy()                   # policy 1 with the ratios 5000 would have given: the trajectory must tell them apart
    scaled[:, :4 * actions.MAX_DEVICES].view("<i4")[1, :D] = [80, 1000, 0, 60]
    other = new_oracle(D, N, MODERATE)
    oracle_prologue(other)
    assert (oracle_population_steps(other, scaled, N // P, score, steps, np.zeros((N, 2), np.int32), MAX_STEPS, True)[3][1] != tallies[1]).any()
    env = make_env(D, MODERATE, n=N)
    gpu_prologue(env)
    monkeypatch.setenv("GW_ROLLOUT_POLICY_UNFUSED" if unfused else "GW_ROLLOUT_STRICT", "1")
    got = env.rollout_backlog_population(torch.from_numpy(raw).cuda(), steps, max_steps=MAX_STEPS, score=score)
    ref = {"tallies": tallies, "tally": tally, "state": state, "obs_next": obs_next, "orc": orc}
    assert_population(env, got, ref, "with weights outside their bounds")
    # ... and the clamped array is the same policy
    twin = make_env(D, MODERATE, n=N)
    gpu_prologue(twin)
    assert torch.equal(twin.rollout_backlog_population(valid, steps, max_steps=MAX_STEPS, score=score), got)
    assert_same_episodes(env, twin)


@pytest.mark.gpu
def test_a_captured_call_reads_the_policies_the_array_holds_at_each_replay():
    """A linear capture of one call of 8 steps on a side stream; between replays the device array is overwritten.  Each replay
    equals the eager call with those policies on a twin handle: the policies are not baked into the recording."""
    import torch
    D, G = 4, 8
    pops = [case_population(D, 2 * P)[P:], case_population(D, P), case_population(D, P)[::-1].copy()]
    score = case_score(D)
    g, twin = make_env(D, MODERATE, n=N), make_env(D, MODERATE, n=N)
    gpu_prologue(g)
    gpu_prologue(twin)
    g.episode_state                                                     # (first use allocates the episode tensors)
    policies = torch.from_numpy(pops[0]).cuda()
    tally = torch.zeros((P, 5), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        g.rollout_backlog_population(policies, G, max_steps=MAX_STEPS, score=score, tally=tally)
    assert launches(g).get("ct_rollout_backlog_pop<4, 1>") == 1, launches(g)
    seen = []
    for i, pop in enumerate(pops):
        policies.copy_(torch.from_numpy(pop))
        tally.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want = twin.rollout_backlog_population(pop, G, max_steps=MAX_STEPS, score=score)
        assert torch.equal(tally, want), "replay %d" % i
        assert_same_episodes(g, twin)
        for f in STATE_FIELDS + STAT_FIELDS:                            # (a snapshot's header tells a handle that was captured)
            assert (g.get_state(f).view(np.uint8) == twin.get_state(f).view(np.uint8)).all(), (f, i)
        seen.append(tuple(want.cpu().numpy().ravel().tolist()))
    assert len(set(seen)) == 3 and all(any(s) for s in seen)            # the three populations fare differently


# ---- 5. the agent ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_search_agent_runs_generations_from_the_same_snapshot():
    from gymwipe_amd.actions import make_score
    from gymwipe_amd.agents import BacklogSearchAgent
    D, policies = 4, 8

    def run(seed):
        env = make_env(D, 0.03, n=512)
        agent = BacklogSearchAgent(env, policies, 32, 8, seed=seed, score=make_score(D, reward=0, delivered=1))
        start = env.snapshot()
        assert (start == agent._start).all()
        first = agent.step()
        after = env.snapshot()
        assert (after != start).any()
        again = agent.evaluate(agent_population(agent, policies), 1)     # restores the snapshot first: the default policy's figure again
        assert tuple(again.shape) == (policies, 5) and again.dtype.is_floating_point is False
        assert float(again[0, 3]) / float(again[0, 0]) == first["of_mu"] and (again[0] == again[1:]).all()
        agent.step()
        return agent

    def agent_population(agent, n):
        from gymwipe_amd.actions import make_backlog_policy, make_backlog_population
        return make_backlog_population([make_backlog_policy(D)] * n)

    a, b = run(3), run(3)
    assert len(a.history) == 2 and a.history[0]["fitness"].shape == (policies,) and a.history[0]["best"] > 0
    assert a.policy().tobytes() == b.policy().tobytes() and (a.mu == b.mu).all()
    assert all((x["fitness"] == y["fitness"]).all() for x, y in zip(a.history, b.history))
    assert len(set(a.history[0]["fitness"].tolist())) > 1
