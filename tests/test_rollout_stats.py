"""
gw_rollout_policy_stats and gw_transition_stats on the GPU: the closed loop of tests/test_rollout_policy.py with the transitions
tallied into int64 table[3][A][7] inside the launch (ct_rollout_pstats<DT, MODE>), and the same table from recorded transitions.

The expected table is always actions.transition_stats_numpy applied to the ORACLE's trajectory (test_rollout_policy.reference:
CtOracle stepped with the CPU restatement of the draw), never anything the library computed.  Integer adds commute, so every
comparison is exact.  An expected table must exercise the bins: expected_table() raises, instead of letting a test pass, when
a class row has fewer than 10 non-empty bins.  tests/test_rollout_stats_cpu.py checks on the CPU that INSTANTIATIONS is exactly
the library's set.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_kernel_variants import MODE_SWITCHES, SFX_DTS, launches
from test_rollout_policy import (CENTER, K_INST, K_LONG, MAX_DURATION, N, PARITY_DS, SEED, delta, gpu_prep, make_env, new_oracle,
                                 oracle_policy_steps, oracle_prep, policy_table, prep_actions, reference)
from util import assert_state_equal, STATE_FIELDS, STAT_FIELDS

INSTANTIATIONS = {"ct_rollout_pstats<%d, %d>" % (dt, mode): (dt, mode) for dt in SFX_DTS + (0,) for mode in (2, 1, 0)}
MIN_BINS = 10


def gate(table, what):
    bins = (np.asarray(table)[..., 0] > 0).sum(axis=1)
    if bins.min() < MIN_BINS:
        raise RuntimeError("%s: non-empty bins per observation class %s, fewer than %d: the table is hardly exercised"
                           % (what, bins.tolist(), MIN_BINS))
    return table


def numpy_table(obs_prev, out, D, center=CENTER):
    from gymwipe_amd.actions import transition_stats_numpy
    return transition_stats_numpy(obs_prev, *out, center, MAX_DURATION, D)


@functools.lru_cache(maxsize=None)
def expected_table(D, steps=K_LONG):
    """The oracle's trajectory of reference(D, steps) as a table, computed once and read only."""
    ref = reference(D, steps)
    t = gate(numpy_table(ref["obs_prev"], ref["out"], D), "reference(%d, %d)" % (D, steps))
    assert t[..., 0].sum() == steps * N and (t[..., 3:6].sum(axis=-1) == t[..., 0]).all()
    t.setflags(write=False)
    return t


def stats_launches(env):
    return {k: v for k, v in launches(env).items() if k.startswith("ct_rollout_pstats")}


def assert_table(got, want, where):
    got = got.cpu().numpy()
    assert got.dtype == np.int64 and got.shape == want.shape, where
    assert (got == want).all(), "table differs %s, first at (class, action, column) %s" % (where, np.argwhere(got != want)[:4].tolist())


# ---- 1. parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("D", PARITY_DS)
def test_one_call_matches_the_oracle(D):
    import torch
    ref, want = reference(D), expected_table(D)
    env = make_env(D)
    gpu_prep(env, D)
    returns = torch.zeros(N, dtype=torch.int32, device=env.device)
    table = env.rollout_policy_stats(ref["cdf"], K_LONG, SEED, returns=returns)
    assert_table(table, want, "in one call of %d steps" % K_LONG)
    assert (env._last[0].cpu().numpy() == ref["out"][2][-1]).all()
    assert (returns.cpu().numpy() == ref["out"][3].astype(np.int64).sum(axis=0)).all()
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after the call")
    dt = D if D in SFX_DTS else 0
    assert stats_launches(env) == {"ct_rollout_pstats<%d, 2>" % dt: 3}, launches(env)
    assert not [k for k in launches(env) if k.startswith("ct_rollout_policy")]
    env.check()


# ---- 2. accumulation and stream continuity ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pieces", [(64, 64, 22), (1,) * K_LONG], ids=["64+64+22", "150x1"])
def test_split_calls_accumulate_into_one_table(pieces):
    """Each call acts on the observations the one before left (obs_last in place as the next obs_prev) and adds into the same
    table, which starts from a pattern: pattern + the one-call table comes back."""
    import torch
    D = 4
    ref, want = reference(D), expected_table(D)
    env = make_env(D)
    gpu_prep(env, D)
    pattern = (np.arange(want.size, dtype=np.int64).reshape(want.shape) * 1000003 - 77) * (1 << 20)
    table = torch.from_numpy(pattern.copy()).to(env.device)
    returns = torch.full((N,), 5, dtype=torch.int32, device=env.device)
    s = 0
    for n in pieces:
        before = env._stats_last.data_ptr() if s else None
        assert env.rollout_policy_stats(ref["cdf"], n, SEED, step0=s, table=table, returns=returns) is table
        assert before is None or env._last[0].data_ptr() == before      # the same array, read and then written
        s += n
    assert_table(table, pattern + want, "over calls of %s steps" % (pieces[:3],))
    assert (returns.cpu().numpy() == 5 + ref["out"][3].astype(np.int64).sum(axis=0)).all()
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after the split calls")


# ---- 3. the two entry points agree ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_recorded_transitions_give_the_same_table_on_a_twin_handle():
    D = 4
    ref, want = reference(D), expected_table(D)
    env, twin = make_env(D), make_env(D)
    first = gpu_prep(env, D).clone()
    gpu_prep(twin, D)
    out = env.rollout_policy(ref["cdf"], K_LONG, SEED)
    recorded = env.transition_stats(first, *out)
    fused = twin.rollout_policy_stats(ref["cdf"], K_LONG, SEED)
    assert_table(recorded, want, "from recorded transitions")
    assert_table(fused, want, "from the fused form")
    assert (recorded == fused).all()
    assert (twin._last[0] == out[2][-1]).all()


# ---- 4. one case per instantiation --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(INSTANTIATIONS))
def test_instantiation_matches_the_oracle(name, monkeypatch):
    dt, mode = INSTANTIATIONS[name]
    D = dt if dt else 11
    for k, v in dict(MODE_SWITCHES[mode], GW_ROLLOUT_STRICT="1").items():
        monkeypatch.setenv(k, v)
    ref, want = reference(D, K_INST), expected_table(D, K_INST)         # (shared by the three modes of a sender count)
    env = make_env(D)
    gpu_prep(env, D)
    before = launches(env)
    table = env.rollout_policy_stats(ref["cdf"], K_INST, SEED)
    assert_table(table, want, "under %s" % name)
    assert (env._last[0].cpu().numpy() == ref["out"][2][-1]).all()
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after %s" % name)
    assert delta(launches(env), before) == {name: 1}, launches(env)     # the target, and nothing else


# ---- 5. the done column -----------------------------------------------------------------------------------------------------
K_DONE = 40


@functools.lru_cache(maxsize=None)
def done_reference():
    """counter_bound = 2 at D = 2: a delivered payload (value 2) reaches the bound, so done fires from the first delivery on."""
    from oracle.ct_oracle import CtOracle, default_config
    from gymwipe_amd.actions import policy_sample_numpy
    D, bound = 2, 2
    _, cdf = policy_table(D)
    cfg = default_config(D)
    cfg.counter_bound = bound
    orc = CtOracle(N, D, config=cfg, nthreads=8)
    obs_prev = oracle_prep(orc, D)
    out = [np.empty((K_DONE, N), t) for t in (np.int32, np.int32, np.int32, np.float32, np.uint8)]
    obs = obs_prev
    for k in range(K_DONE):                                           # oracle_policy_steps with this configuration's centre
        d, u = policy_sample_numpy(SEED, 0, N, k, cdf, obs, bound, MAX_DURATION)
        obs, r, dn = orc.step(d, u)
        for a, v in zip(out, (d, u, obs, r, dn)):
            a[k] = v
    want = gate(numpy_table(obs_prev, out, D, center=bound), "done_reference")
    return {"cdf": cdf, "out": tuple(out), "orc": orc, "table": want}


@pytest.mark.gpu
def test_done_column():
    ref = done_reference()
    want = ref["table"]
    assert 0 < want[..., 6].sum() < want[..., 0].sum(), (want[..., 6].sum(), want[..., 0].sum())
    env = make_env(2, counter_bound=2)
    gpu_prep(env, 2)
    table = env.rollout_policy_stats(ref["cdf"], K_DONE, SEED)
    assert_table(table, want, "with done firing")
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after the done case")


# ---- 6. handles without a fused form ------------------------------------------------------------------------------------------
K_OTHER = 48


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["explicit_queue", "per_env_geometry", "unfused_switch"])
def test_handles_without_a_fused_form(kind, monkeypatch):
    """GW_ROLLOUT_POLICY_UNFUSED leaves no handle a fused form (read per call), as it does for gw_rollout_policy: the C entry
    point answers GW_EUNSUPPORTED before it launches anything, and rollout_policy_stats composes the table from rollout_policy
    and transition_stats."""
    import torch
    from gymwipe_amd import _native as nat
    D = {"explicit_queue": 3, "per_env_geometry": 4, "unfused_switch": 4}[kind]
    kw = {"explicit_queue": {"explicit_queue": True}, "per_env_geometry": {"per_env_geometry": True}, "unfused_switch": {}}[kind]
    if kind == "unfused_switch":
        monkeypatch.setenv("GW_ROLLOUT_POLICY_UNFUSED", "1")
    _, cdf = policy_table(D)
    env, orc = make_env(D, **kw), new_oracle(D)
    first = gpu_prep(env, D).clone()
    obs_prev = oracle_prep(orc, D)
    out, _ = oracle_policy_steps(orc, cdf, K_OTHER, SEED, 0, 0, obs_prev)
    want = gate(numpy_table(obs_prev, out, D), kind)
    before = launches(env)
    words = env._policy_table(cdf)
    table = torch.zeros(want.shape, dtype=torch.int64, device=env.device)
    last = torch.empty(N, dtype=torch.int32, device=env.device)
    rc = nat.lib().gw_rollout_policy_stats(env._h, K_OTHER, words.data_ptr(), SEED, 0, 0, first.data_ptr(), last.data_ptr(), None,
                                           table.data_ptr(), None)
    assert rc == nat.EUNSUPPORTED
    assert launches(env) == before and int(table.abs().sum()) == 0      # refused before anything was launched
    returns = torch.zeros(N, dtype=torch.int32, device=env.device)
    got = env.rollout_policy_stats(cdf, K_OTHER, SEED, table=table, returns=returns)
    assert_table(got, want, "through the fallback (%s)" % kind)
    assert (env._last[0].cpu().numpy() == out[2][-1]).all()
    assert (returns.cpu().numpy() == out[3].astype(np.int64).sum(axis=0)).all()
    fields = tuple(f for f in STATE_FIELDS + STAT_FIELDS if f != "rx_power" or kind != "per_env_geometry")
    assert_state_equal(env, orc, fields, where="after the fallback (%s)" % kind)
    assert not stats_launches(env), launches(env)


# ---- 7. shards ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_shards_sum_to_one_handle():
    import torch
    D = 4
    ref, want = reference(D), expected_table(D)
    total = torch.zeros(want.shape, dtype=torch.int64, device="cuda")
    for lo, hi in ((0, 120), (120, N)):
        cols = slice(lo, hi)
        env = make_env(D, n=hi - lo)
        gpu_prep(env, D, cols)
        part = env.rollout_policy_stats(ref["cdf"], K_LONG, SEED, env_id0=lo)
        assert_table(part, numpy_table(ref["obs_prev"][cols], tuple(a[:, cols] for a in ref["out"]), D), "in the shard at %d" % lo)
        total += part
    assert_table(total, want, "summed over the shards")


# ---- 8. gw_transition_stats on arbitrary content ------------------------------------------------------------------------------
def hand_made_rows(D, md, n, steps, seed):
    """Rows with actions around the edges of the action space, observations on and off the three values, rewards that need
    the rounding and the clamp, done bytes above 1."""
    rng = np.random.default_rng(seed)
    dev = rng.integers(-2, D + 2, (steps, n)).astype(np.int32)
    dur = rng.integers(-2, md + 2, (steps, n)).astype(np.int32)
    dev[0, :3], dur[0, :3] = (D - 1, 0, -2 ** 31), (md - 1, 0, 5)
    values = np.array([CENTER - 2, CENTER, CENTER + 2, 0, 2 ** 31 - 1, -2 ** 31, CENTER + 1], np.int32)
    obs = values[rng.integers(0, len(values), (steps, n))]
    obs_prev = values[rng.integers(0, len(values), n)]
    rewards = np.array([3.6, -50.0, 2.0, -2.0, 0.0, 0.5, 1.5, 2.5, -0.5, 9.51, 10.49, 1e30, -1e30, np.inf], np.float32)
    rew = rewards[rng.integers(0, len(rewards), (steps, n))]
    done = rng.integers(0, 256, (steps, n)).astype(np.uint8) * (rng.random((steps, n)) < 0.5).astype(np.uint8)
    return obs_prev, (dev, dur, obs, rew, done)


@pytest.mark.gpu
def test_transition_stats_on_hand_made_rows():
    D, n, steps = 4, 70, 96                                             # a partial wave; 6 720 rows: two tiles, the second partial
    obs_prev, rows = hand_made_rows(D, MAX_DURATION, n, steps, 5)
    want = gate(numpy_table(obs_prev, rows, D), "hand-made rows")
    assert want[..., 0].sum() < n * steps and want[..., 6].sum() > 0     # rows were skipped, done bytes counted
    env = make_env(D, n=n)
    got = env.transition_stats(obs_prev, *rows)
    assert_table(got, want, "on hand-made rows")
    assert env.transition_stats(obs_prev, *rows, table=got) is got      # ... and adds
    assert_table(got, 2 * want, "after the second call into the same table")


@pytest.mark.gpu
def test_transition_stats_with_an_action_space_beyond_the_lds_histogram():
    """max_duration = 40 at 32 senders: 3 * 1 280 bins do not fit the LDS histogram, the rows go straight into the table."""
    import torch
    from gymwipe_amd import _native as nat
    L = nat.lib()
    D, md, n, steps = 32, 40, 70, 64
    cfg = nat.default_config(n, D)
    cfg.max_duration = md
    h = C.c_void_p()
    nat.check(L.gw_create(C.byref(cfg), C.byref(h)))
    try:
        obs_prev, rows = hand_made_rows(D, md, n, steps, 6)
        from gymwipe_amd.actions import transition_stats_numpy
        want = gate(transition_stats_numpy(obs_prev, *rows, CENTER, md, D), "hand-made rows, 1 280 actions")
        dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (obs_prev,) + rows]
        table = torch.zeros(want.shape, dtype=torch.int64, device="cuda")
        nat.check(L.gw_transition_stats(h, steps, *[t.data_ptr() for t in dev], table.data_ptr(), None))
        torch.cuda.synchronize()
        assert_table(table, want, "without the LDS histogram")
    finally:
        L.gw_destroy(h)


# ---- 9. agent ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_tabular_agent_collects_learns_and_evaluates():
    import torch
    from gymwipe_amd.agents import TabularCounterTrafficAgent
    D, n, steps = 4, 256, 64
    env, twin = make_env(D, n=n), make_env(D, n=n)
    agent = TabularCounterTrafficAgent(env, gamma=0.9, tau=0.5, seed=5)
    env.reset()
    twin.reset()
    assert agent.collect(steps) is agent.table and agent.stream_pos == steps
    assert int(agent.table[..., 0].sum()) == steps * n
    # learn: the same formula in numpy on the downloaded table
    t = agent.table.cpu().numpy().astype(np.float64)
    q = agent.q.cpu().numpy().copy()
    visited, nn = t[..., 0] > 0, np.maximum(t[..., 0], 1.0)
    for _ in range(3):
        v = q.max(axis=1)
        q = np.where(visited, t[..., 1] / nn + 0.9 * (1.0 - t[..., 6] / nn) * (t[..., 3:6] / nn[..., None] * v).sum(axis=-1), q)
    got = agent.learn(3).cpu().numpy()
    assert visited.sum() >= 3 * MIN_BINS and np.abs(q).max() > 0.1
    assert np.abs(got - q).max() <= 1e-12, np.abs(got - q).max()
    # evaluate: the mean reward of the same steps on a twin handle, transitions and all
    twin.rollout_policy_stats(TabularCounterTrafficAgent(twin, tau=0.5, seed=5).policy_cdf(), steps, 5)   # (the collect above)
    env.reset()                                                         # (rewards come with the first deliveries after a reset)
    twin.reset()
    cdf, pos = agent.policy_cdf(), agent.stream_pos
    mean, err = agent.evaluate(steps)
    rew = twin.rollout_policy(cdf, steps, 5, step0=pos)[3].double()
    assert agent.stream_pos == pos + steps and int(agent.table[..., 0].sum()) == steps * n
    assert abs(mean - float(rew.mean())) <= 1e-12, (mean, float(rew.mean()))
    assert abs(err - float(rew.std(unbiased=False)) / (steps * n) ** 0.5) <= 1e-12
    assert float(rew.abs().mean()) > 0.01                               # (the comparison is not one of zeros)
