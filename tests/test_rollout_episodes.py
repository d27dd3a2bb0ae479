"""
gw_rollout_episodes / gw_rollout_episodes_stats / gw_transition_stats_ep on the GPU: the closed loop of
tests/test_rollout_policy.py with episodes -- an env whose step returned done, or whose episode reached its step limit, is reset
inside the launch (ct_rollout_policy_ep<DT, MODE>, ct_rollout_pstats_ep<DT, MODE>) -- and the per-step form of every other handle.

Every expected value comes from the oracle alone: CtOracle.step with actions.policy_sample_numpy, then actions.episodes_numpy,
then CtOracle.reset(mask) for the envs whose episode ended (episode_reference()).  All comparisons are exact, the state
included (STATE_FIELDS + STAT_FIELDS: queue contents and flags too).  An expected trajectory must exercise what it is for:
episode_reference() raises, instead of letting a test pass, when it ends fewer than MIN_EPISODES episodes by a cause the case is
meant to exercise, and expected_table() when an observation class has fewer than MIN_BINS non-empty bins.
tests/test_rollout_episodes_cpu.py checks on the CPU that the two INSTANTIATIONS sets are exactly the library's.
"""
import functools

import numpy as np
import pytest

from test_kernel_variants import MODE_SWITCHES, SFX_DTS, launches
from test_rollout_policy import (CENTER, K_INST, K_LONG, MAX_DURATION, N, PARITY_DS, SEED, delta, gpu_prep, make_env, oracle_prep,
                                 policy_table)
from test_rollout_stats import MIN_BINS, assert_table, gate
from util import assert_state_equal, STATE_FIELDS, STAT_FIELDS

INSTANTIATIONS = {"ct_rollout_policy_ep<%d, %d>" % (dt, mode): (dt, mode) for dt in SFX_DTS + (0,) for mode in (2, 1, 0)}
STATS_INSTANTIATIONS = {"ct_rollout_pstats_ep<%d, %d>" % (dt, mode): (dt, mode) for dt in SFX_DTS + (0,) for mode in (2, 1, 0)}
MIN_EPISODES = 50
MAX_STEPS = 5                           # does not divide 64: episodes straddle the launch chunks
NAMES = ("device", "duration", "obs", "reward", "done", "ended")
DTYPES = (np.int32, np.int32, np.int32, np.float32, np.uint8, np.uint8)


def oracle_episode_steps(orc, cdf, steps, seed, step0, env_id0, obs_prev, state, max_steps, on_done, center=CENTER):
    """The oracle under the policy with episodes: the six [steps][n] outputs, the observation each env acts on next and the
    episode tally; ``state`` ({age, ret}, int32[n][2]) is updated in place."""
    from gymwipe_amd.actions import EP_COLS, episodes_numpy, policy_sample_numpy
    n = orc.n
    out = [np.empty((steps, n), t) for t in DTYPES]
    tally = np.zeros(EP_COLS, np.int64)
    acts_on = np.asarray(obs_prev, np.int32).copy()
    for k in range(steps):
        d, u = policy_sample_numpy(seed, env_id0, env_id0 + n, step0 + k, cdf, acts_on, center, MAX_DURATION)
        obs, r, dn = orc.step(d, u)
        ended, t = episodes_numpy(state, r, dn, max_steps, on_done)
        tally += t
        if ended.any():
            orc.reset((ended != 0).astype(np.uint8))
        for a, v in zip(out, (d, u, obs, r, dn, ended)):
            a[k] = v
        acts_on = np.where(ended != 0, center, obs).astype(np.int32)
    return tuple(out), acts_on, tally


def new_oracle(D, n=N, bound=None, mult=None):
    from oracle.ct_oracle import CtOracle, default_config
    cfg = default_config(D, mult=mult)
    if bound is not None:
        cfg.counter_bound = bound
    return CtOracle(n, D, config=cfg, nthreads=8)


@functools.lru_cache(maxsize=None)
def episode_reference(D, steps=K_LONG, max_steps=MAX_STEPS, on_done=True, bound=None, mult1=False, causes=(2,)):
    """The oracle's trajectory of `steps` episodic policy steps after the PREP ordinary ones, computed once and read only.
    `causes`: the ways an episode ends that the case is meant to exercise (1 done, 2 step limit)."""
    _, cdf = policy_table(D)
    orc = new_oracle(D, bound=bound, mult=(1,) * D if mult1 else None)
    center = CENTER if bound is None else bound
    obs_prev = oracle_prep(orc, D)
    state = np.zeros((N, 2), np.int32)
    out, obs_next, tally = oracle_episode_steps(orc, cdf, steps, SEED, 0, 0, obs_prev, state, max_steps, on_done, center)
    by = {1: int(tally[1]), 2: int(tally[0] - tally[1])}
    for cause in causes:
        if by[cause] < MIN_EPISODES:
            raise RuntimeError("episode_reference(%d, %d): %d episodes ended by cause %d, fewer than %d"
                               % (D, steps, by[cause], cause, MIN_EPISODES))
    assert tally[0] == (out[5] != 0).sum() and tally[1] == (out[5] == 1).sum()
    for a in out + (obs_next, state, tally):
        a.setflags(write=False)
    return {"cdf": cdf, "obs_prev": obs_prev, "out": out, "obs_next": obs_next, "state": state, "tally": tally, "orc": orc,
            "center": center}


@functools.lru_cache(maxsize=None)
def expected_table(D, steps=K_LONG):
    from gymwipe_amd.actions import transition_stats_numpy
    ref = episode_reference(D, steps)
    t = gate(transition_stats_numpy(ref["obs_prev"], *ref["out"][:5], CENTER, MAX_DURATION, D, ended=ref["out"][5]),
             "episode_reference(%d, %d)" % (D, steps))
    assert t[..., 0].sum() == steps * N
    t.setflags(write=False)
    return t


def assert_outputs(got, want, where, cols=slice(None)):
    assert len(got) == len(want) == 6
    for name, g, w in zip(NAMES, got, want):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w[:, cols].shape, (name, where)
        same = g.view(np.uint8) == np.ascontiguousarray(w[:, cols]).view(np.uint8)
        assert same.all(), "%s differs %s, first at (step, env) %s" % (name, where, np.argwhere(g != w[:, cols])[:3].tolist())


def assert_episodes(env, ref, where, cols=slice(None), tally=True):
    """obs_next, {age, ret} and (for a whole handle) the tally against the oracle's."""
    assert (env._last[0].cpu().numpy() == ref["obs_next"][cols]).all(), "obs_next differs " + where
    assert (env.episode_state.cpu().numpy() == ref["state"][cols]).all(), "{age, ret} differs " + where
    if tally:
        assert env.episode_tally.cpu().numpy().tolist() == ref["tally"].tolist(), "tally differs " + where


def ep_launches(env):
    return {k: v for k, v in launches(env).items() if k.startswith("ct_rollout_p")}


# ---- 1. one call ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("D", PARITY_DS)
def test_one_call_matches_the_oracle(D):
    ref = episode_reference(D)
    env = make_env(D)
    gpu_prep(env, D)
    got = env.rollout_episodes(ref["cdf"], K_LONG, SEED, max_steps=MAX_STEPS)
    assert_outputs(got, ref["out"], "in one call of %d steps" % K_LONG)
    assert_episodes(env, ref, "after the call")
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after the call")
    dt = D if D in SFX_DTS else 0
    assert ep_launches(env) == {"ct_rollout_policy_ep<%d, 2>" % dt: 3}, launches(env)
    stats = env.episode_stats()
    n, by_done, length, ret, sq = (int(x) for x in ref["tally"])
    assert stats["episodes"] == n and stats["by_done"] == by_done and stats["mean_length"] == length / n
    assert stats["mean_return"] == ret / n
    assert abs(stats["return_stderr"] - (max(sq / n - (ret / n) ** 2, 0.0) / n) ** 0.5) <= 1e-12
    env.check()


# ---- 2. both causes -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_done_and_the_step_limit_both_end_episodes():
    """counter_bound = 2 at D = 2: a delivered payload (value 2) reaches the bound, so done fires with the first delivery."""
    ref = episode_reference(2, bound=2, causes=(1, 2))
    env = make_env(2, counter_bound=2)
    gpu_prep(env, 2)
    got = env.rollout_episodes(ref["cdf"], K_LONG, SEED, max_steps=MAX_STEPS, on_done=True)
    assert_outputs(got, ref["out"], "with both causes")
    assert_episodes(env, ref, "with both causes")
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="with both causes")


# ---- 3. a reset after every step ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_reset_after_every_step():
    """max_steps = 1 with one packet per tick: a queue's 100 entries span many breakpoints, so the head's counter value comes
    from the ring's older entries (gw_tick_value's deep path), and both branches of the breakpoint rule are taken (a step
    without a tick in it overwrites the newest breakpoint).  A state and queue parity check: the other classes are hardly seen."""
    D = 4
    ref = episode_reference(D, max_steps=1, mult1=True)
    assert ref["tally"][0] == K_LONG * N
    env = make_env(D, multiplicity=[1] * D)
    gpu_prep(env, D)
    got = env.rollout_episodes(ref["cdf"], K_LONG, SEED, max_steps=1)
    assert_outputs(got, ref["out"], "with a reset after every step")
    assert_episodes(env, ref, "with a reset after every step")
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="with a reset after every step")


# ---- 4. split calls -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pieces", [(64, 64, 22), (1,) * K_LONG], ids=["64+64+22", "150x1"])
def test_split_calls_equal_one_call(pieces):
    """{age, ret} and obs_next are carried in place from call to call; the tally and the table start from a pattern."""
    import torch
    D = 4
    ref, want = episode_reference(D), expected_table(D)
    env, twin = make_env(D), make_env(D)
    gpu_prep(env, D)
    gpu_prep(twin, D)
    tally0 = np.array([3, 1, 1 << 40, -(1 << 33), 7], np.int64)
    pattern = (np.arange(want.size, dtype=np.int64).reshape(want.shape) * 1000003 - 77) * (1 << 20)
    table = torch.from_numpy(pattern.copy()).to(twin.device)
    for e in (env, twin):
        e.episode_tally.copy_(torch.from_numpy(tally0))
    rows, s = [], 0
    for n in pieces:
        before = (env.episode_state.data_ptr(), env._last[0].data_ptr() if s else None)
        rows.append(env.rollout_episodes(ref["cdf"], n, SEED, max_steps=MAX_STEPS, step0=s))
        assert twin.rollout_episodes_stats(ref["cdf"], n, SEED, max_steps=MAX_STEPS, step0=s, table=table) is table
        assert env.episode_state.data_ptr() == before[0] and (before[1] is None or env._last[0].data_ptr() == before[1])
        s += n
    got = tuple(torch.cat([r[i] for r in rows]) for i in range(6))
    assert_outputs(got, ref["out"], "over calls of %s steps" % (pieces[:3],))
    assert_table(table, pattern + want, "over calls of %s steps" % (pieces[:3],))
    for e in (env, twin):
        assert_episodes(e, ref, "after the split calls", tally=False)
        assert (e.episode_tally.cpu().numpy() == tally0 + ref["tally"]).all()
        assert_state_equal(e, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after the split calls")


# ---- 5. limits off --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_without_limits_it_is_rollout_policy():
    """max_steps = 0, on_done = 0 on one handle, rollout_policy on its twin: output for output, and no byte of the two
    snapshots differs that did not differ before the calls (the header's own device addresses)."""
    D = 4
    _, cdf = policy_table(D)
    env, twin = make_env(D), make_env(D)
    gpu_prep(env, D)
    gpu_prep(twin, D)
    own = env.snapshot() != twin.snapshot()
    assert own.sum() < 4096, own.sum()
    got = env.rollout_episodes(cdf, K_LONG, SEED, max_steps=0, on_done=False)
    want = twin.rollout_policy(cdf, K_LONG, SEED)
    for name, g, w in zip(NAMES, got, want):
        assert (g == w).all(), name
    assert int(got[5].sum()) == 0 and float(got[3].abs().sum()) > 0
    differ = env.snapshot() != twin.snapshot()
    assert not (differ & ~own).any(), np.flatnonzero(differ & ~own)[:8]
    state = env.episode_state.cpu().numpy()
    assert (state[:, 0] == K_LONG).all() and (state[:, 1] == got[3].cpu().numpy().astype(np.int64).sum(axis=0)).all()
    assert (env._last[0] == got[2][-1]).all() and int(env.episode_tally.abs().sum()) == 0


# ---- 6. stats -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("D", PARITY_DS)
def test_stats_match_the_oracle_and_the_recorded_rows(D):
    ref, want = episode_reference(D), expected_table(D)
    env, twin = make_env(D), make_env(D)
    first = gpu_prep(env, D).clone()
    gpu_prep(twin, D)
    fused = env.rollout_episodes_stats(ref["cdf"], K_LONG, SEED, max_steps=MAX_STEPS)
    assert_table(fused, want, "from the fused form")
    assert_episodes(env, ref, "after the fused stats call")
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after the fused stats call")
    dt = D if D in SFX_DTS else 0
    assert ep_launches(env) == {"ct_rollout_pstats_ep<%d, 2>" % dt: 3}, launches(env)
    out = twin.rollout_episodes(ref["cdf"], K_LONG, SEED, max_steps=MAX_STEPS)
    recorded = twin.transition_stats(first, *out[:5], ended=out[5])
    assert_table(recorded, want, "from recorded rows")
    plain = twin.transition_stats(first, *out[:5])                      # (the rows without `ended`: another table)
    assert not (plain == recorded).all()


# ---- 7. one case per instantiation ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(INSTANTIATIONS))
def test_instantiation_matches_the_oracle(name, monkeypatch):
    dt, mode = INSTANTIATIONS[name]
    D = dt if dt else 11
    for k, v in dict(MODE_SWITCHES[mode], GW_ROLLOUT_STRICT="1").items():
        monkeypatch.setenv(k, v)
    ref = episode_reference(D, K_INST)                                  # (shared by the three modes of a sender count)
    env = make_env(D)
    gpu_prep(env, D)
    before = launches(env)
    got = env.rollout_episodes(ref["cdf"], K_INST, SEED, max_steps=MAX_STEPS)
    assert_outputs(got, ref["out"], "under %s" % name)
    assert_episodes(env, ref, "after %s" % name)
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after %s" % name)
    assert delta(launches(env), before) == {name: 1}, launches(env)     # the target, and no step or reset kernel


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(STATS_INSTANTIATIONS))
def test_stats_instantiation_matches_the_oracle(name, monkeypatch):
    dt, mode = STATS_INSTANTIATIONS[name]
    D = dt if dt else 11
    for k, v in dict(MODE_SWITCHES[mode], GW_ROLLOUT_STRICT="1").items():
        monkeypatch.setenv(k, v)
    ref, want = episode_reference(D, K_INST), expected_table(D, K_INST)
    env = make_env(D)
    gpu_prep(env, D)
    before = launches(env)
    table = env.rollout_episodes_stats(ref["cdf"], K_INST, SEED, max_steps=MAX_STEPS)
    assert_table(table, want, "under %s" % name)
    assert_episodes(env, ref, "after %s" % name)
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after %s" % name)
    assert delta(launches(env), before) == {name: 1}, launches(env)


# ---- 8. other handles -------------------------------------------------------------------------------------------------------------
K_OTHER = 24


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["explicit_queue", "per_env_geometry", "unfused_switch"])
def test_handles_without_a_fused_form_reset_per_step(kind, monkeypatch):
    from gymwipe_amd import _native as nat
    from gymwipe_amd.actions import transition_stats_numpy
    D = {"explicit_queue": 3, "per_env_geometry": 4, "unfused_switch": 4}[kind]
    kw = {"explicit_queue": {"explicit_queue": True}, "per_env_geometry": {"per_env_geometry": True}, "unfused_switch": {}}[kind]
    if kind == "unfused_switch":
        monkeypatch.setenv("GW_ROLLOUT_POLICY_UNFUSED", "1")
    _, cdf = policy_table(D)
    env, twin, orc = make_env(D, **kw), make_env(D, **kw), new_oracle(D)
    gpu_prep(env, D)
    first = gpu_prep(twin, D).clone()
    acts_on = oracle_prep(orc, D)
    state, tally, rows = np.zeros((N, 2), np.int32), 0, []
    obs_prev = acts_on
    before = launches(env)
    for call in range(2):
        got = env.rollout_episodes(cdf, K_OTHER, SEED, max_steps=MAX_STEPS, step0=call * K_OTHER)
        want, acts_on, t = oracle_episode_steps(orc, cdf, K_OTHER, SEED, call * K_OTHER, 0, acts_on, state, MAX_STEPS, True)
        tally = tally + t
        rows.append(want)
        assert_outputs(got, want, "in call %d (%s)" % (call, kind))
    if tally[0] < MIN_EPISODES:
        raise RuntimeError("%d episodes ended, fewer than %d" % (tally[0], MIN_EPISODES))
    assert_episodes(env, {"obs_next": acts_on, "state": state, "tally": tally}, "after two calls (%s)" % kind)
    if kind == "per_env_geometry":                                      # (received power as tests/test_rollout_policy.py bounds it)
        fields = tuple(f for f in STATE_FIELDS + STAT_FIELDS if f != "rx_power")
        a, b = env.get_state("rx_power"), orc.get("rx_power")
        assert np.max(np.abs(a - b) / b) < 1e-5
    else:
        fields = STATE_FIELDS + STAT_FIELDS
    assert_state_equal(env, orc, fields, where="after two calls (%s)" % kind)
    ran = delta(launches(env), before)
    assert not [k for k in launches(env) if "_ep<" in k], ran
    assert sum(v for k, v in ran.items() if k.startswith("ct_step")) == 2 * K_OTHER and len(ran) == 1, ran
    # the stats call composes the same table from rollout_episodes and transition_stats(ended=...)
    both = tuple(np.concatenate([r[i] for r in rows]) for i in range(6))
    table = gate(transition_stats_numpy(obs_prev, *both[:5], CENTER, MAX_DURATION, D, ended=both[5]), kind)
    got = twin.rollout_episodes_stats(cdf, 2 * K_OTHER, SEED, max_steps=MAX_STEPS, obs_prev=first)
    assert_table(got, table, "through the fallback (%s)" % kind)
    assert not [k for k in launches(twin) if "_ep<" in k]
    if kind != "unfused_switch":
        monkeypatch.setenv("GW_ROLLOUT_STRICT", "1")
        for call in (lambda: env.rollout_episodes(cdf, 4, SEED, max_steps=MAX_STEPS, step0=2 * K_OTHER),
                     lambda: env.rollout_episodes_stats(cdf, 4, SEED, max_steps=MAX_STEPS, step0=2 * K_OTHER)):
            with pytest.raises(nat.NativeError) as exc:
                call()
            assert exc.value.code == nat.EUNSUPPORTED
        assert delta(launches(env), before) == ran                      # refused before anything was launched


# ---- 9. shards --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_shards_equal_one_handle():
    import torch
    D = 4
    ref = episode_reference(D)
    total = torch.zeros(5, dtype=torch.int64, device="cuda")
    for lo in (0, 100):
        cols = slice(lo, lo + 100)
        env = make_env(D, n=100)
        gpu_prep(env, D, cols)
        got = env.rollout_episodes(ref["cdf"], K_LONG, SEED, max_steps=MAX_STEPS, env_id0=lo)
        assert_outputs(got, ref["out"], "in the shard at %d" % lo, cols)
        assert_episodes(env, ref, "in the shard at %d" % lo, cols, tally=False)
        for f in STATE_FIELDS + STAT_FIELDS:
            assert (env.get_state(f).view(np.uint8) == ref["orc"].get(f)[cols].view(np.uint8)).all(), (f, lo)
        total += env.episode_tally
    assert total.cpu().numpy().tolist() == ref["tally"].tolist()


# ---- 10. agents -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_tabular_agent_with_episodes_needs_no_reset_between_calls():
    from gymwipe_amd.actions import transition_stats_numpy
    from gymwipe_amd.agents import TabularCounterTrafficAgent
    D, steps = 4, 64
    env, orc = make_env(D), new_oracle(D)
    agent = TabularCounterTrafficAgent(env, gamma=0.9, tau=0.5, seed=5, episode_steps=MAX_STEPS)
    env.reset()
    acts_on = orc.reset()
    state = np.zeros((N, 2), np.int32)
    cdf = agent.policy_cdf().cpu().numpy().astype(np.uint32)           # the table the launch reads, taken to the oracle
    assert agent.collect(steps) is agent.table and agent.stream_pos == steps
    out, acts_on, tally = oracle_episode_steps(orc, cdf, steps, 5, 0, 0, acts_on, state, MAX_STEPS, True)
    want = gate(transition_stats_numpy(np.full(N, CENTER), *out[:5], CENTER, MAX_DURATION, D, ended=out[5]), "the agent's collect")
    assert_table(agent.table, want, "after collect")
    assert (np.abs(agent.learn(3).cpu().numpy()) > 0.1).any()
    cdf = agent.policy_cdf().cpu().numpy().astype(np.uint32)
    mean, err = agent.evaluate(steps)                                   # continues the episodes: no reset in between
    out2, acts_on, tally2 = oracle_episode_steps(orc, cdf, steps, 5, steps, 0, acts_on, state, MAX_STEPS, True)
    rew = out2[3].astype(np.float64)
    assert abs(mean - rew.mean()) <= 1e-12 and abs(err - rew.std() / rew.size ** 0.5) <= 1e-12
    assert np.abs(rew).mean() > 0.05                                    # (not the absorbing state's zeros)
    assert_table(agent.table, want, "after evaluate: untouched")
    assert env.episode_stats()["episodes"] == int(tally[0] + tally2[0]) >= 2 * MIN_EPISODES
    assert_state_equal(env, orc, STATE_FIELDS + STAT_FIELDS, where="after collect, learn and evaluate")


@pytest.mark.gpu
def test_dqn_agent_stores_the_observation_acted_on_and_the_terminal_one():
    import torch
    from gymwipe_amd.agents import DqnCounterTrafficAgent
    n, steps = 256, 32
    env = make_env(4, n=n)
    agent = DqnCounterTrafficAgent(env, seed=5)
    first = env.reset().clone()
    dev, dur, obs, rew, done, ended = agent.collect(steps, episode_steps=MAX_STEPS)
    assert agent.m_len == steps * n and agent.stream_pos == steps
    m_obs, m_next = agent.m_obs[:steps * n].view(steps, n), agent.m_next[:steps * n].view(steps, n)
    # the default configuration never returns done, so every env's episodes end at steps 4, 9, 14, ... by the step limit
    want_ended = torch.zeros_like(ended)
    want_ended[MAX_STEPS - 1::MAX_STEPS] = 2
    assert torch.equal(ended, want_ended) and int(done.sum()) == 0
    assert torch.equal(m_next, obs.float()) and torch.equal(m_obs[0], first.float())   # the terminal observation stays
    over = ended[:-1] != 0
    assert torch.equal(m_obs[1:][over], torch.full_like(m_obs[1:][over], agent.center))   # acted on the reset's observation
    assert torch.equal(m_obs[1:][~over], obs[:-1][~over].float())
    assert bool((obs[:-1][over] != int(agent.center)).any())            # (some terminal observations were off the centre)
    assert torch.equal(agent.m_act[:steps * n].view(steps, n), dev.long() * MAX_DURATION + dur.long())
    assert torch.equal(agent.m_rew[:steps * n].view(steps, n), rew)
    assert len(agent.collect(4)) == 5                                   # without episode_steps: as before
