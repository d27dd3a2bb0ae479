"""
The tally with the packets a step delivered, on the GPU: gw_rollout_episodes_stats_delivered (ct_rollout_pstats_epd<DT, MODE>),
gw_rollout_policy_stats_delivered (ct_rollout_pstats_d<DT, MODE>) and gw_transition_stats_delivered
(transition_stats_rows_d<LDS, EP>), the composed fallback of env.rollout_episodes_stats(packets=True), and
TabularCounterTrafficAgent(score=).

The fused calls' expected table is always actions.transition_stats_numpy(delivered=) applied to the ORACLE's trajectory -- for
the episodic call tests/test_rollout_scored_cpu.py's oracle_scored_steps with the neutral score, for the other one CtOracle
stepped with the CPU restatement of the draw and its delivered counter differenced across each step -- never anything the
library computed; the rows kernel is checked against the same restatement of the rows it was given.
Integer adds commute, so every comparison is exact.  Columns 0-6 and everything else a call leaves behind are compared with the
parent call on a twin handle.  N = 200 is three full blocks and one of 8 lanes, K = 70 a launch of 64 steps and one of 6.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_kernel_variants import SFX_DTS, launches
from test_rollout_episodes import MAX_STEPS, MIN_EPISODES
from test_rollout_policy import CENTER, MAX_DURATION, N, SEED, delta, gpu_prep, make_env, oracle_prep, policy_table
from test_rollout_scored_cpu import delivered_now, new_oracle, oracle_scored_steps
from test_rollout_stats import assert_table, gate

K = 70
DS = (2, 4, 7, 11)                      # a packed record, the default, an odd templated count, no kernel of its own (DT == 0)


def fused_name(family, D):
    return "%s<%d, 2>" % (family, D if D in SFX_DTS else 0)


def stats_launches(env):
    return {k: v for k, v in launches(env).items() if k.startswith("ct_rollout_pstats")}


def gate_packets(table, what):
    gate(table, what)
    if not ((table[..., 7] > 0).sum(axis=1) >= 2).all() or (table[..., 7] < 0).any() or (table[..., 7] > 65535 * table[..., 0]).any():
        raise RuntimeError("%s: the packets column is hardly exercised, or impossible" % what)
    return table


@functools.lru_cache(maxsize=None)
def episodic_reference(D, n=N):
    """The oracle composition: K episodic steps under the neutral score after the PREP ordinary ones, and their table."""
    from gymwipe_amd.actions import make_score, transition_stats_numpy
    _, cdf = policy_table(D)
    orc = new_oracle(D, n)
    obs_prev = oracle_prep(orc, D, slice(0, n))
    before = delivered_now(orc)
    state = np.zeros((n, 2), np.int32)
    out, plain, obs_next, tally = oracle_scored_steps(orc, cdf, make_score(D), K, SEED, 0, 0, obs_prev, state, MAX_STEPS, True)
    assert (out[3] == plain).all()
    if tally[0] < MIN_EPISODES:
        raise RuntimeError("episodic_reference(%d): %d episodes ended, fewer than %d" % (D, tally[0], MIN_EPISODES))
    table = gate_packets(transition_stats_numpy(obs_prev, *out[:5], CENTER, MAX_DURATION, D, ended=out[5], delivered=out[6]),
                         "episodic_reference(%d)" % D)
    assert table[..., 0].sum() == K * n and table[..., 7].sum() == (delivered_now(orc) - before).sum() == out[6].sum()
    for a in out + (obs_prev, obs_next, state, tally, table):
        a.setflags(write=False)
    return {"cdf": cdf, "obs_prev": obs_prev, "out": out, "obs_next": obs_next, "state": state, "tally": tally, "table": table}


@functools.lru_cache(maxsize=None)
def plain_reference(D):
    """The same for the call without episodes: the oracle under the policy, its delivered counter differenced per step."""
    from gymwipe_amd.actions import policy_sample_numpy, transition_stats_numpy
    _, cdf = policy_table(D)
    orc = new_oracle(D, N)
    obs_prev = oracle_prep(orc, D)
    out = [np.empty((K, N), t) for t in (np.int32, np.int32, np.int32, np.float32, np.uint8, np.int32)]
    obs = obs_prev
    for k in range(K):
        d, u = policy_sample_numpy(SEED, 0, N, k, cdf, obs, CENTER, MAX_DURATION)
        before = delivered_now(orc)
        obs, r, dn = orc.step(d, u)
        for a, v in zip(out, (d, u, obs, r, dn, delivered_now(orc) - before)):
            a[k] = v
    table = gate_packets(transition_stats_numpy(obs_prev, *out[:5], CENTER, MAX_DURATION, D, delivered=out[5]), "plain_reference(%d)" % D)
    table.setflags(write=False)
    return {"cdf": cdf, "obs_last": out[2][-1].copy(), "returns": out[3].astype(np.int64).sum(axis=0), "table": table}


def twins(D, n=N, **kw):
    """Two handles in the same state, the observation both act on, and the bytes of their snapshots that differ anyway (the
    header's own device addresses)."""
    env, twin = make_env(D, n=n, **kw), make_env(D, n=n, **kw)
    first = gpu_prep(env, D, slice(0, n)).clone()
    gpu_prep(twin, D, slice(0, n))
    own = env.snapshot() != twin.snapshot()
    assert own.sum() < 4096, own.sum()
    return env, twin, first, own


def assert_same_state(env, twin, own, where):
    differ = env.snapshot() != twin.snapshot()
    assert not (differ & ~own).any(), "%s: snapshots differ at %s" % (where, np.flatnonzero(differ & ~own)[:8].tolist())
    assert (env._last[0] == twin._last[0]).all(), where


def delivered_total(env):
    return int(env.get_state("n_delivered").astype(np.int64).sum())


# ---- 1. the fused forms -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("D", DS)
def test_fused_episodic_table_equals_the_oracle_composition(D):
    import torch
    ref = episodic_reference(D)
    env, twin, _, own = twins(D)
    had = delivered_total(env)
    got = env.rollout_episodes_stats(ref["cdf"], K, SEED, max_steps=MAX_STEPS, packets=True)
    assert tuple(got.shape) == (3, D * MAX_DURATION, 8)
    assert_table(got, ref["table"], "from the fused form")
    assert stats_launches(env) == {fused_name("ct_rollout_pstats_epd", D): 2}, launches(env)      # 64 + 6 steps
    assert int(got[..., 7].sum()) == delivered_total(env) - had > 0
    parent = twin.rollout_episodes_stats(ref["cdf"], K, SEED, max_steps=MAX_STEPS)
    assert stats_launches(twin) == {fused_name("ct_rollout_pstats_ep", D): 2}, launches(twin)
    assert torch.equal(got[..., :7], parent)
    assert (env.episode_state.cpu().numpy() == ref["state"]).all() and torch.equal(env.episode_state, twin.episode_state)
    assert env.episode_tally.cpu().numpy().tolist() == ref["tally"].tolist() and torch.equal(env.episode_tally, twin.episode_tally)
    assert (env._last[0].cpu().numpy() == ref["obs_next"]).all()
    assert_same_state(env, twin, own, "after the episodic calls")
    assert env.rollout_episodes_stats(ref["cdf"], 0, SEED, max_steps=MAX_STEPS, table=got, packets=True) is got       # steps == 0
    with pytest.raises(ValueError):
        env.rollout_episodes_stats(ref["cdf"], 1, SEED, max_steps=MAX_STEPS, table=parent, packets=True)              # seven columns
    env.check()


@pytest.mark.gpu
@pytest.mark.parametrize("D", DS)
def test_fused_table_without_episodes_equals_the_oracle_composition(D):
    import torch
    ref = plain_reference(D)
    env, twin, _, own = twins(D)
    had = delivered_total(env)
    ret, ret_twin = (torch.zeros(N, dtype=torch.int32, device=env.device) for _ in range(2))
    got = env.rollout_policy_stats(ref["cdf"], K, SEED, returns=ret, packets=True)
    assert_table(got, ref["table"], "from the fused form")
    assert stats_launches(env) == {fused_name("ct_rollout_pstats_d", D): 2}, launches(env)
    assert int(got[..., 7].sum()) == delivered_total(env) - had > 0
    parent = twin.rollout_policy_stats(ref["cdf"], K, SEED, returns=ret_twin)
    assert stats_launches(twin) == {fused_name("ct_rollout_pstats", D): 2}, launches(twin)
    assert torch.equal(got[..., :7], parent) and torch.equal(ret, ret_twin)
    assert (ret.cpu().numpy() == ref["returns"]).all() and (env._last[0].cpu().numpy() == ref["obs_last"]).all()
    assert_same_state(env, twin, own, "after the calls without episodes")
    env.check()


@pytest.mark.gpu
def test_split_calls_accumulate_into_one_table():
    """1 + 63 + 6 steps: the launch's delivered counter restarts at 0 in every launch, and the baseline with it."""
    D = 4
    for episodic in (True, False):
        ref = episodic_reference(D) if episodic else plain_reference(D)
        env = make_env(D)
        gpu_prep(env, D)
        table, s = None, 0
        for n in (1, 63, 6):
            if episodic:
                table = env.rollout_episodes_stats(ref["cdf"], n, SEED, max_steps=MAX_STEPS, step0=s, table=table, packets=True)
            else:
                table = env.rollout_policy_stats(ref["cdf"], n, SEED, step0=s, table=table, packets=True)
            s += n
        assert_table(table, ref["table"], "over calls of 1 + 63 + 6 steps (episodic: %s)" % episodic)


# ---- 2. recorded rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_recorded_rows_give_the_fused_table_in_both_forms_of_the_rows_kernel():
    """The records of rollout_episodes(score=make_score(D)) on a twin handle.  LDS form: the handle's own action space (240
    bins).  Direct form: the same rows read by a handle of 32 senders x 40 durations, whose 3 840 bins do not fit the LDS
    histogram -- no fused form exists at that size, so its table is compared bin by bin through a = device * 40 + duration."""
    import torch
    from gymwipe_amd import _native as nat
    from gymwipe_amd.actions import make_score
    D = 4
    ref = episodic_reference(D)
    env, twin, first, _ = twins(D)
    fused = env.rollout_episodes_stats(ref["cdf"], K, SEED, max_steps=MAX_STEPS, packets=True)
    out = twin.rollout_episodes(ref["cdf"], K, SEED, max_steps=MAX_STEPS, score=make_score(D))
    recorded = twin.transition_stats(first, *out[:5], ended=out[5], delivered=out[6])
    assert torch.equal(recorded, fused)
    assert_table(recorded, ref["table"], "from recorded rows, LDS form")
    assert twin.transition_stats(first, *out[:5], ended=out[5], delivered=out[6], table=recorded) is recorded      # ... and adds
    assert_table(recorded, 2 * ref["table"], "after the second call into the same table")
    plain = twin.transition_stats(first, *out[:5], delivered=out[6])                   # (without `ended`: another table)
    assert int(plain[..., 7].sum()) == int(fused[..., 7].sum()) and not torch.equal(plain, fused)
    # the direct form
    L = nat.lib()
    D2, md2 = 32, 40
    cfg = nat.default_config(N, D2)
    cfg.max_duration = md2
    h = C.c_void_p()
    nat.check(L.gw_create(C.byref(cfg), C.byref(h)))
    try:
        wide = torch.zeros((3, D2 * md2, 8), dtype=torch.int64, device="cuda")
        nat.check(L.gw_transition_stats_delivered(h, K, first.data_ptr(), *[out[i].data_ptr() for i in (0, 1, 2, 3, 4, 5, 6)],
                                                  wide.data_ptr(), None))
        torch.cuda.synchronize()
        a = np.arange(D * MAX_DURATION)
        to = torch.from_numpy((a // MAX_DURATION) * md2 + a % MAX_DURATION).cuda()
        assert torch.equal(wide[:, to], fused), "direct form"
        assert int(wide[..., 0].sum()) == K * N and int(wide.abs().sum()) == int(fused.abs().sum())     # nothing anywhere else
    finally:
        L.gw_destroy(h)


@pytest.mark.gpu
def test_recorded_rows_of_the_scored_autoreset_call():
    """rollout_autoreset(score=) returns delivered and ended too: its records tally as transition_stats_numpy tallies them."""
    import torch
    from gymwipe_amd.actions import make_score, transition_stats_numpy
    D, n, steps = 4, 70, 40
    rng = np.random.default_rng(9)
    dev = rng.integers(-1, D + 1, (steps, n)).astype(np.int32)           # some actions outside the action space: skipped rows
    dur = rng.integers(0, MAX_DURATION, (steps, n)).astype(np.int32)
    env = make_env(D, n=n)
    first = env.reset().clone()
    obs, rew, done, ended, dl = env.rollout_autoreset(torch.from_numpy(dev), torch.from_numpy(dur), max_steps=MAX_STEPS, score=make_score(D))
    got = env.transition_stats(first, dev, dur, obs, rew, done, ended=ended, delivered=dl)
    want = transition_stats_numpy(first.cpu().numpy(), dev, dur, *[t.cpu().numpy() for t in (obs, rew, done)], CENTER, MAX_DURATION, D,
                                  ended=ended.cpu().numpy(), delivered=dl.cpu().numpy())
    assert_table(got, want, "from the scored autoreset call's records")
    assert 0 < want[..., 0].sum() < steps * n and int(want[..., 7].sum()) == int(dl.sum()) > 0


@pytest.mark.gpu
def test_field_top():
    """One full tile: 4 096 transitions of one bin, each with the largest reward, done set and 65 535 packets -- every field of
    the bin's two words at its top at once.  Then counts beyond the clamp and below 0, in both forms of the kernel's input."""
    import torch
    D, n, steps = 4, 64, 64
    env = make_env(D, n=n)
    full = lambda v, t: torch.full((steps, n), v, dtype=t, device=env.device)
    first = torch.full((n,), CENTER + 2, dtype=torch.int32, device=env.device)
    rows = (full(3, torch.int32), full(19, torch.int32), full(CENTER + 2, torch.int32), full(10.0, torch.float32), full(1, torch.uint8))
    parent = env.transition_stats(first, *rows)
    got = env.transition_stats(first, *rows, delivered=full(65535, torch.int32))
    assert int(parent[2, 79, 0]) == 4096 and int(parent[..., 0].sum()) == 4096
    assert torch.equal(got[..., :7], parent)
    assert int(got[2, 79, 7]) == 65535 * 4096 and int(got[..., 7].sum()) == 65535 * 4096
    over = env.transition_stats(first, *rows, delivered=full(70000, torch.int32))
    assert torch.equal(over, got)
    mixed = full(-3, torch.int32)
    mixed[0, :5] = torch.tensor([0, 1, 65535, 65536, 2 ** 31 - 1], dtype=torch.int32)
    under = env.transition_stats(first, *rows, delivered=mixed, ended=full(0, torch.uint8))
    assert torch.equal(under[..., :7], parent) and int(under[2, 79, 7]) == 1 + 3 * 65535


# ---- 3. handles without the fused form ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["rollout_cap_0", "per_env_geometry"])
def test_the_composed_fallback_gives_the_fused_table(kind, monkeypatch):
    """(GW_ROLLOUT_CAP is read when the handle is created, so the first handle is a default one without a fused rollout.)"""
    import torch
    from gymwipe_amd import _native as nat
    D = 4
    ref = episodic_reference(D)
    if kind == "rollout_cap_0":
        monkeypatch.setenv("GW_ROLLOUT_CAP", "0")
    env = make_env(D, **({"per_env_geometry": True} if kind == "per_env_geometry" else {}))
    monkeypatch.delenv("GW_ROLLOUT_CAP", raising=False)
    first = gpu_prep(env, D).clone()
    before, snap = launches(env), env.snapshot()
    # the C entry points answer GW_EUNSUPPORTED before they launch anything
    words = env._policy_table(ref["cdf"])
    table = torch.zeros((3, D * MAX_DURATION, 8), dtype=torch.int64, device=env.device)
    nxt = torch.empty(N, dtype=torch.int32, device=env.device)
    ep = nat.Episodes(MAX_STEPS, 1, env.episode_state.data_ptr(), env.episode_tally.data_ptr())
    L = nat.lib()
    assert L.gw_rollout_episodes_stats_delivered(env._h, K, words.data_ptr(), SEED, 0, 0, C.byref(ep), first.data_ptr(), nxt.data_ptr(),
                                                 table.data_ptr(), None) == nat.EUNSUPPORTED
    assert b"gw_rollout_episodes_stats_delivered" in L.gw_last_error()
    assert L.gw_rollout_policy_stats_delivered(env._h, K, words.data_ptr(), SEED, 0, 0, first.data_ptr(), nxt.data_ptr(), None,
                                               table.data_ptr(), None) == nat.EUNSUPPORTED
    assert b"gw_rollout_policy_stats_delivered" in L.gw_last_error()
    torch.cuda.synchronize()
    assert launches(env) == before and int(table.abs().sum()) == 0 and (env.snapshot() == snap).all()
    # ... rollout_policy_stats(packets=True) has nothing to compose from, GW_ROLLOUT_STRICT refuses the episodic call's composition
    with pytest.raises(nat.NativeError) as exc:
        env.rollout_policy_stats(ref["cdf"], K, SEED, packets=True)
    assert exc.value.code == nat.EUNSUPPORTED
    monkeypatch.setenv("GW_ROLLOUT_STRICT", "1")
    with pytest.raises(nat.NativeError) as exc:
        env.rollout_episodes_stats(ref["cdf"], K, SEED, max_steps=MAX_STEPS, packets=True)
    monkeypatch.delenv("GW_ROLLOUT_STRICT")
    assert exc.value.code == nat.EUNSUPPORTED and launches(env) == before and (env.snapshot() == snap).all()
    # ... and without it the call composes the fused form's table, per step
    got = env.rollout_episodes_stats(ref["cdf"], K, SEED, max_steps=MAX_STEPS, table=table, packets=True)
    assert got is table
    assert_table(got, ref["table"], "through the fallback (%s)" % kind)
    assert (env.episode_state.cpu().numpy() == ref["state"]).all() and env.episode_tally.cpu().numpy().tolist() == ref["tally"].tolist()
    assert (env._last[0].cpu().numpy() == ref["obs_next"]).all()
    ran = delta(launches(env), before)
    assert not stats_launches(env) and not [k for k in launches(env) if "_ep" in k], ran
    assert sum(v for k, v in ran.items() if k.startswith("ct_step")) == K and len(ran) == 1, ran


@pytest.mark.gpu
def test_an_explicit_queue_handle_is_refused():
    from gymwipe_amd import _native as nat
    D = 3
    _, cdf = policy_table(D)
    env = make_env(D, explicit_queue=True)
    gpu_prep(env, D)
    before = launches(env)
    for call in (lambda: env.rollout_episodes_stats(cdf, 4, SEED, max_steps=MAX_STEPS, packets=True),
                 lambda: env.rollout_policy_stats(cdf, 4, SEED, packets=True)):
        with pytest.raises(nat.NativeError) as exc:
            call()
        assert exc.value.code == nat.EUNSUPPORTED
    assert launches(env) == before


# ---- 4. the agent -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("episode_steps", [8, None])
def test_tabular_agent_learns_from_the_score(episode_steps):
    import torch
    from gymwipe_amd.actions import make_score, table_score
    from gymwipe_amd.agents import TabularCounterTrafficAgent
    D, n, steps, gamma = 4, 256, 64, 0.9
    score = make_score(D, reward=2, delivered=[1, 3, 0, 5])
    env = make_env(D, n=n)
    agent = TabularCounterTrafficAgent(env, gamma=gamma, tau=0.5, seed=5, episode_steps=episode_steps, score=score)
    assert tuple(agent.table.shape) == (3, D * MAX_DURATION, 8)
    env.reset()
    q = torch.zeros_like(agent.q)
    for rnd in range(2):
        assert agent.collect(steps) is agent.table and agent.stream_pos == (rnd + 1) * steps
        assert int(agent.table[..., 0].sum()) == (rnd + 1) * steps * n and int(agent.table[..., 7].sum()) > 0
        sums = table_score(agent.table, score, MAX_DURATION)
        q = TabularCounterTrafficAgent.q_iteration(q, agent.table, gamma, 3, r_sum=sums)
        assert torch.equal(agent.learn(3), q)
        # ... which is the formula in numpy on the downloaded table, with the score sums where the reward sums were
        t = agent.table.cpu().numpy()
        w = score.astype(np.int64)
        s_np = (w[0] * t[..., 1] + w[1 + np.arange(D * MAX_DURATION) // MAX_DURATION] * t[..., 7]).astype(np.float64)
        assert (sums.cpu().numpy() == s_np).all() and not (s_np == w[0] * t[..., 1]).all()
    assert float(q.abs().max()) > 0.1
    name = "ct_rollout_pstats_epd" if episode_steps else "ct_rollout_pstats_d"
    assert stats_launches(env) == {fused_name(name, D): 2}, launches(env)
    kept = agent.table.clone()
    env.reset()                                  # (a packet carries its counter's value: without a reset it soon outgrows every window)
    mean, err = agent.evaluate(steps)
    assert err is None and mean > 0.0 and torch.equal(agent.table, kept) and agent.stream_pos == 3 * steps
    assert TabularCounterTrafficAgent(make_env(D, n=64), seed=5).table.shape[-1] == 7       # score=None: the seven-column agent
