"""
gw_rollout_policy on the GPU: the closed loop observation -> policy -> step inside one launch (ct_rollout_policy<DT, MODE>),
and its unfused form on every other handle.

The checker is oracle.ct_oracle.CtOracle stepped with actions.policy_sample_numpy, the CPU restatement of the draw: device,
duration, obs, reward and done are compared bit for bit at every step, then the state (STATE_FIELDS and STAT_FIELDS).  The
oracle's trajectories are computed once per configuration and shared (reference() / episodic_reference()); each must visit
every observation class often enough, else the test errors instead of passing on a policy row that was never used.
tests/test_rollout_policy_cpu.py checks on the CPU that INSTANTIATIONS is exactly the library's set.
"""
import functools

import numpy as np
import pytest

from test_kernel_variants import MODE_SWITCHES, SFX_DTS, launches
from util import action_stream, assert_state_equal, STATE_FIELDS, STAT_FIELDS

N, K_LONG = 200, 150                    # three full waves and a partial one; chunks of 64 + 64 + 22
PREP = 2                                # ordinary steps before the call, so that obs_prev is not all centre
CENTER, MAX_DURATION = 65536, 20        # counter_traffic.py:35, envs/core.py:25 (the default configuration)
# Seed and PREP picked on the oracle alone (no GPU involved), so that every observation class is visited often enough (at
# D = 2 an env leaves the centre class only while exactly one of its two senders has delivered since the last reset).
# Rarest class among the 30 000 (env, step) pairs of reference(D): 133 at D = 2, 1 047 at D = 4, 2 230 / 4 938 / 6 169 at
# D = 5 / 9 / 32; of episodic_reference(D): 10.8 % at D = 2, 7.5 % at D = 4, 13.0 / 15.5 / 7.9 % at D = 5 / 9 / 32.
# Of the 8 000 pairs of reference(D, K_INST): 133 at D = 2 (the same visits as over 150 steps: none of that class after
# step 40), 334 at D = 3, 419 to 2 004 at the other sender counts.
SEED = 7
PARITY_DS = (2, 4, 5, 9, 32)

INSTANTIATIONS = {"ct_rollout_policy<%d, %d>" % (dt, mode): (dt, mode) for dt in SFX_DTS + (0,) for mode in (2, 1, 0)}


def policy_table(D):
    """Three Dirichlet(0.3) rows over the D * 20 flat actions, a quarter of each row's actions set to p = 0."""
    from gymwipe_amd.actions import policy_cdf
    A = D * MAX_DURATION
    rng = np.random.default_rng(1000 * SEED + D)
    p = rng.dirichlet(np.full(A, 0.3), size=3)
    for row in p:
        row[rng.permutation(A)[:A // 4]] = 0.0
    p /= p.sum(axis=1, keepdims=True)
    return p, policy_cdf(p)


def class_counts(seen):
    return np.bincount((np.sign(np.asarray(seen, np.int64) - CENTER) + 1).ravel(), minlength=3)


def new_oracle(D, n=N, **cfg):
    from oracle.ct_oracle import CtOracle, default_config
    return CtOracle(n, D, config=default_config(D, **cfg), nthreads=8)


def prep_actions(D):
    return action_stream(11 + D, PREP, N, D)


def oracle_prep(orc, D, cols=slice(None)):
    dev, dur = prep_actions(D)
    obs = orc.reset()
    for k in range(PREP):
        obs, _, _ = orc.step(dev[k][cols], dur[k][cols])
    return obs


def oracle_policy_steps(orc, cdf, steps, seed, step0, env_id0, obs_prev, hook=None):
    """The oracle under the policy: (device, duration, obs, reward, done)[steps][n] and the observations acted on."""
    from gymwipe_amd.actions import policy_sample_numpy
    n = orc.n
    out = [np.empty((steps, n), t) for t in (np.int32, np.int32, np.int32, np.float32, np.uint8)]
    seen = np.empty((steps, n), np.int32)
    obs = np.asarray(obs_prev, np.int32)
    for k in range(steps):
        seen[k] = obs
        d, u = policy_sample_numpy(seed, env_id0, env_id0 + n, step0 + k, cdf, obs, CENTER, MAX_DURATION)
        obs, r, dn = orc.step(d, u)
        for a, v in zip(out, (d, u, obs, r, dn)):
            a[k] = v
    return tuple(out), seen


@functools.lru_cache(maxsize=None)
def reference(D, steps=K_LONG):
    """The oracle's trajectory of `steps` policy steps after the PREP ordinary ones, computed once: outputs, the observation
    before the call, and the oracle itself in its final state (read only from here on)."""
    _, cdf = policy_table(D)
    orc = new_oracle(D)
    obs_prev = oracle_prep(orc, D)
    out, seen = oracle_policy_steps(orc, cdf, steps, SEED, 0, 0, obs_prev)
    return {"cdf": cdf, "obs_prev": obs_prev, "out": out, "classes": class_counts(seen), "orc": orc}


def reset_mask(call):
    """The episodic form's masked reset before call `call`: about half of the envs, drawn from the draw's own hash."""
    from gymwipe_amd.actions import policy_u_numpy
    return (policy_u_numpy(SEED ^ 0x5eed, 0, N, 1 << 40 | call) & 1).astype(np.uint8)


EPISODES, K_EPISODE = 10, 15


@functools.lru_cache(maxsize=None)
def episodic_reference(D):
    _, cdf = policy_table(D)
    orc = new_oracle(D)
    obs = oracle_prep(orc, D)
    outs, seen = [], []
    for call in range(EPISODES):
        if call:
            obs = orc.reset(reset_mask(call))
        out, s = oracle_policy_steps(orc, cdf, K_EPISODE, SEED, call * K_EPISODE, 0, obs)
        obs = out[2][-1]
        outs.append(out)
        seen.append(s)
    return {"cdf": cdf, "outs": outs, "classes": class_counts(np.concatenate(seen)), "orc": orc}


def make_env(D, n=N, **kw):
    from gymwipe_amd import VecCounterTrafficEnv
    kw.setdefault("per_env_stats", True)
    return VecCounterTrafficEnv(n, num_devices=D, **kw)


def gpu_prep(env, D, cols=slice(None)):
    import torch
    dev, dur = prep_actions(D)
    env.reset()
    for k in range(PREP):
        o, _, _, _ = env.step({"device": torch.from_numpy(np.ascontiguousarray(dev[k][cols])),
                               "duration": torch.from_numpy(np.ascontiguousarray(dur[k][cols]))})
    return o


NAMES = ("device", "duration", "obs", "reward", "done")


def assert_outputs(got, want, where, cols=slice(None)):
    for name, g, w in zip(NAMES, got, want):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w[:, cols].shape, (name, where)
        same = g.view(np.uint8) == np.ascontiguousarray(w[:, cols]).view(np.uint8)
        assert same.all(), "%s differs %s, first at (step, env) %s" % (name, where, np.argwhere(g != w[:, cols])[:3].tolist())


def policy_launches(env):
    return {k: v for k, v in launches(env).items() if k.startswith("ct_rollout_policy")}


def delta(after, before):
    return {k: v - before.get(k, 0) for k, v in after.items() if v != before.get(k, 0)}


# ---- 1. parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("D", PARITY_DS)
def test_one_call_matches_the_oracle(D):
    ref = reference(D)
    if ref["classes"].min() < 100:
        raise RuntimeError("observation classes visited %s times: a policy row is hardly used" % ref["classes"].tolist())
    env = make_env(D)
    gpu_prep(env, D)
    got = env.rollout_policy(ref["cdf"], K_LONG, SEED)                  # obs_prev: the observation the env returned last
    assert_outputs(got, ref["out"], "in one call of %d steps" % K_LONG)
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after the call")
    dt = D if D in SFX_DTS else 0
    assert policy_launches(env) == {"ct_rollout_policy<%d, 2>" % dt: 3}, launches(env)
    env.check()                                                        # (no GW_FLAG_BADACT: every draw is inside the space)


# ---- 2. episodic form -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("D", PARITY_DS)
def test_calls_with_masked_resets_in_between_match_the_oracle(D):
    import torch
    ref = episodic_reference(D)
    total = EPISODES * K_EPISODE * N
    if ref["classes"].min() < total // 100:
        raise RuntimeError("observation classes visited %s times of %d" % (ref["classes"].tolist(), total))
    env = make_env(D)
    gpu_prep(env, D)
    for call in range(EPISODES):
        if call:
            env.reset(torch.from_numpy(reset_mask(call)))              # its observations are what the next call acts on
        got = env.rollout_policy(ref["cdf"], K_EPISODE, SEED, step0=call * K_EPISODE)
        assert_outputs(got, ref["outs"][call], "in call %d" % call)
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after the last call")


# ---- 3. replay ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_recorded_actions_replay_through_gw_rollout_on_a_twin_handle():
    """Two handles' snapshots differ in the bytes that hold their own device addresses (the header in front of the state
    records) and nowhere else: the positions that differ after the same PREP steps.  After the closed loop on one and the
    replay of its recorded actions on the other, no other byte may differ."""
    D = 4
    ref = reference(D)
    env, twin = make_env(D), make_env(D)
    gpu_prep(env, D)
    gpu_prep(twin, D)
    own = env.snapshot() != twin.snapshot()
    assert own.sum() < 4096, own.sum()
    dev, dur, obs, rew, done = env.rollout_policy(ref["cdf"], K_LONG, SEED)
    o2, r2, d2 = twin.rollout(dev, dur)
    assert_outputs((o2, r2, d2), ref["out"][2:], "in the replay")
    assert (o2 == obs).all() and (r2 == rew).all() and (d2 == done).all()
    differ = env.snapshot() != twin.snapshot()
    assert not (differ & ~own).any(), np.flatnonzero(differ & ~own)[:8]
    assert_state_equal(twin, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after the replay")


# ---- 4. stream continuity ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pieces", [(64, 64, 22), (1,) * K_LONG], ids=["64+64+22", "150x1"])
def test_split_calls_continue_the_stream(pieces):
    import torch
    D = 4
    ref = reference(D)
    env = make_env(D)
    gpu_prep(env, D)
    rows, s = [], 0
    for n in pieces:
        rows.append(env.rollout_policy(ref["cdf"], n, SEED, step0=s))
        s += n
    got = tuple(torch.cat([r[i] for r in rows]) for i in range(5))
    assert_outputs(got, ref["out"], "over calls of %s steps" % (pieces[:3],))
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after the split calls")


@pytest.mark.gpu
def test_reused_out_buffers_continue_from_their_own_last_row():
    """The same `out` call after call: the default obs_prev is then the last row of the obs buffer the call is about to
    write.  The native call wants the two apart, so rollout_policy copies the row; the results are the one call's."""
    import torch
    D, k = 4, K_LONG // 3
    ref = reference(D)
    env = make_env(D)
    gpu_prep(env, D)
    out = tuple(torch.empty((k, N), dtype=t, device=env.device)
                for t in (torch.int32, torch.int32, torch.int32, torch.float32, torch.uint8))
    for call in range(3):
        got = env.rollout_policy(ref["cdf"], k, SEED, step0=call * k, out=out)
        assert all(g is o for g, o in zip(got, out))
        assert_outputs(got, tuple(w[call * k:(call + 1) * k] for w in ref["out"]), "in call %d into the same buffers" % call)
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after three calls into the same buffers")


# ---- 5. shards ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_shards_equal_one_handle():
    D = 4
    ref = reference(D)
    for lo in (0, 100):
        cols = slice(lo, lo + 100)
        env = make_env(D, n=100)
        gpu_prep(env, D, cols)
        got = env.rollout_policy(ref["cdf"], K_LONG, SEED, env_id0=lo)
        assert_outputs(got, ref["out"], "in the shard at %d" % lo, cols)
        for f in STATE_FIELDS + STAT_FIELDS:
            assert (env.get_state(f).view(np.uint8) == ref["orc"].get(f)[cols].view(np.uint8)).all(), (f, lo)


# ---- 6. other handles -------------------------------------------------------------------------------------------------------
K_OTHER = 24


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["explicit_queue", "per_env_geometry", "unfused_switch"])
def test_handles_without_a_fused_form_draw_and_step_per_step(kind, monkeypatch):
    from gymwipe_amd import _native as nat
    D = {"explicit_queue": 3, "per_env_geometry": 4, "unfused_switch": 4}[kind]
    kw = {"explicit_queue": {"explicit_queue": True}, "per_env_geometry": {"per_env_geometry": True}, "unfused_switch": {}}[kind]
    if kind == "unfused_switch":
        monkeypatch.setenv("GW_ROLLOUT_POLICY_UNFUSED", "1")
    _, cdf = policy_table(D)
    env, orc = make_env(D, **kw), new_oracle(D)
    gpu_prep(env, D)
    obs = oracle_prep(orc, D)
    before = launches(env)
    for call in range(2):
        if call and kind == "per_env_geometry":                         # a radio moves between the two calls
            env.set_position(1, 0.5, -2.5)
            orc.set_position(1, 0.5, -2.5)
        got = env.rollout_policy(cdf, K_OTHER, SEED, step0=call * K_OTHER)
        want, _ = oracle_policy_steps(orc, cdf, K_OTHER, SEED, call * K_OTHER, 0, obs)
        obs = want[2][-1]
        assert_outputs(got, want, "in call %d (%s)" % (call, kind))
    if kind == "per_env_geometry":
        # the live PHY recomputes moved links with the device libm: received power as tests/test_live_phy.py bounds it
        # (1e-5 relative), everything else bit for bit
        fields = tuple(f for f in STATE_FIELDS + STAT_FIELDS if f != "rx_power")
        a, b = env.get_state("rx_power"), orc.get("rx_power")
        assert np.max(np.abs(a - b) / b) < 1e-5
    else:
        fields = STATE_FIELDS + STAT_FIELDS
    assert_state_equal(env, orc, fields, where="after two calls (%s)" % kind)
    ran = delta(launches(env), before)
    assert not policy_launches(env), ran
    assert sum(v for k, v in ran.items() if k.startswith("ct_step")) == 2 * K_OTHER and len(ran) == 1, ran
    if kind != "unfused_switch":
        monkeypatch.setenv("GW_ROLLOUT_STRICT", "1")
        with pytest.raises(nat.NativeError) as exc:
            env.rollout_policy(cdf, 4, SEED, step0=2 * K_OTHER)
        assert exc.value.code == nat.EUNSUPPORTED
        assert delta(launches(env), before) == ran                      # refused before anything was launched


# ---- 7. one case per instantiation --------------------------------------------------------------------------------------------
K_INST = 40


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(INSTANTIATIONS))
def test_instantiation_matches_the_oracle(name, monkeypatch):
    dt, mode = INSTANTIATIONS[name]
    D = dt if dt else 11
    for k, v in dict(MODE_SWITCHES[mode], GW_ROLLOUT_STRICT="1").items():
        monkeypatch.setenv(k, v)
    ref = reference(D, K_INST)                                          # (shared by the three modes of a sender count)
    if ref["classes"].min() < 100:                                      # as in 1, unscaled although K is shorter
        raise RuntimeError("observation classes visited %s times: a policy row is hardly used" % ref["classes"].tolist())
    want, cdf, orc = ref["out"], ref["cdf"], ref["orc"]
    env = make_env(D)
    gpu_prep(env, D)
    before = launches(env)
    got = env.rollout_policy(cdf, K_INST, SEED)
    assert_outputs(got, want, "under %s" % name)
    assert_state_equal(env, orc, STATE_FIELDS + STAT_FIELDS, where="after %s" % name)
    assert delta(launches(env), before) == {name: 1}, launches(env)     # the target, and no step kernel


# ---- 8. agent ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_agent_collects_transitions_and_builds_its_table_on_the_gpu():
    import torch
    from gymwipe_amd import actions
    from gymwipe_amd.agents import DqnCounterTrafficAgent
    n, steps = 256, 32
    env = make_env(4, n=n)
    agent = DqnCounterTrafficAgent(env, seed=5)
    first = env.reset().clone()
    dev, dur, obs, rew, done = agent.collect(steps)
    assert agent.m_len == steps * n and agent.m_pos == steps * n and agent.stream_pos == steps
    m_obs, m_next = agent.m_obs[:steps * n].view(steps, n), agent.m_next[:steps * n].view(steps, n)
    assert torch.equal(m_next[:-1], m_obs[1:])                         # step k's successor is what step k + 1 acted on
    assert torch.equal(m_obs[0], first.float()) and torch.equal(m_next, obs.float())
    assert torch.equal(agent.m_act[:steps * n].view(steps, n), dev.long() * MAX_DURATION + dur.long())
    assert torch.equal(agent.m_rew[:steps * n].view(steps, n), rew) and torch.equal(agent.m_done[:steps * n].view(steps, n), done.float())
    assert int(dev.min()) >= 0 and int(dev.max()) < 4 and int(dur.min()) >= 0 and int(dur.max()) < MAX_DURATION
    # the table: actions.policy_cdf of the same softmax, taken to the host.  The f32 probabilities are the same numbers on
    # both sides; the f64 cumulative sums are added in another order on the GPU (a parallel scan) than by numpy's running
    # sum.  Every partial sum of either order is below 2, so each of its at most A - 1 additions rounds by at most 2^-53, and
    # the two sums of a prefix differ by less than 2 * (A - 1) * 2^-53 < 2^-45 for A = 80: an ulp or two of a number near 1.
    # Times 2^32 that is below 2^-13, so the floors are equal unless an integer lies between the two products -- the entries
    # differ by at most 1.
    with torch.no_grad():
        x = torch.tensor([agent.center - 2.0, agent.center, agent.center + 2.0], device=agent.dev)
        p = torch.softmax(torch.clamp(agent.q(agent._features(x)) / agent.tau, -500.0, 500.0), dim=-1)
    host = actions.policy_cdf(p.cpu().numpy()).astype(np.int64)
    table = agent.policy_cdf().cpu().numpy().astype(np.int64)
    assert table.shape == host.shape == (3, 80)
    assert np.abs(table - host).max() <= 1, np.abs(table - host).max()
    assert (table[:, -1] == 0xffffffff).all() and (np.diff(table, axis=1) >= 0).all()


@pytest.mark.gpu
def test_policy_cdf_on_the_gpu_keeps_the_table_rules():
    """torch.cumsum on the GPU is a parallel scan, so policy_cdf enforces there what numpy's running sum gives by itself: rows
    non-decreasing, a p == 0 action's entry equal to its predecessor's (0 in front).  Against the numpy table an entry may
    differ by 1 (the bound derived above, A = 640 here: 2 * 639 * 2^-53 * 2^32 < 2^-10, so at most one integer in between)."""
    import torch
    from gymwipe_amd import actions
    p, host = policy_table(32)
    table = actions.policy_cdf(torch.from_numpy(p).cuda()).cpu().numpy()
    assert table.dtype == np.int64 and table.shape == host.shape
    assert (np.diff(table, axis=1) >= 0).all() and table.min() >= 0 and table.max() == 0xffffffff
    before = np.concatenate([np.zeros((3, 1), np.int64), table[:, :-1]], axis=1)
    last = np.where(p > 0, np.arange(p.shape[1]), -1).max(axis=1, keepdims=True)
    inner = (p == 0) & (np.arange(p.shape[1]) < last)                   # (from `last` on: the all-ones tail)
    assert (table[inner] == before[inner]).all()
    assert (table[np.arange(p.shape[1]) >= last.ravel()[:, None]] == 0xffffffff).all()
    assert np.abs(table - host.astype(np.int64)).max() <= 1
