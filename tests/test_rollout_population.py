"""
gw_rollout_population on the GPU: P policy tables on one handle, M envs each, in one launch per 64 steps
(ct_rollout_pop_ep<DT, MODE>) where M is a multiple of 64, and the per-step form of every other call.

Every expected value comes from the oracle alone: CtOracle.step with actions.policy_sample_population_numpy, then
actions.episodes_numpy per policy slice, then CtOracle.reset(mask) (oracle_population_steps() in
tests/test_rollout_population_cpu.py).  All comparisons are exact, the state included (STATE_FIELDS + STAT_FIELDS).  An expected
trajectory must exercise what it is for: population_reference() raises, instead of letting a test pass, when a policy ended
fewer than MIN_EPISODES episodes by a cause the case is for, and when two policies' tally rows are equal -- a kernel that staged
table 0 for every block must fail.  tests/test_rollout_population_cpu.py checks on the CPU that INSTANTIATIONS is exactly the
library's set.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_kernel_variants import MODE_SWITCHES, SFX_DTS, launches
from test_rollout_episodes import MAX_STEPS, MIN_EPISODES, new_oracle
from test_rollout_policy import CENTER, K_INST, K_LONG, MAX_DURATION, N as PREP_N, PARITY_DS, SEED, delta, gpu_prep, make_env, oracle_prep
from test_rollout_population_cpu import AGENT, assert_same_history, oracle_agent, oracle_population_steps
from util import assert_state_equal, STATE_FIELDS, STAT_FIELDS

INSTANTIATIONS = {"ct_rollout_pop_ep<%d, %d>" % (dt, mode): (dt, mode) for dt in SFX_DTS + (0,) for mode in (2, 1, 0)}
P_LONG, M_LONG = 3, 128                 # N = 384: a policy spans two blocks, so two blocks add into one tally row
P_INST, M_INST = 4, 64                  # N = 256: one block per policy
M_BOTH, BOTH_PICKS = 512, (0, 15, 23)   # test_done_and_the_step_limit_both_end_episodes


def population_tables(D, P, picks=None):
    """policy_table()'s recipe once per policy, each with an rng seed of its own (policy 0's is policy_table()'s, unless
    `picks` names others): P x three Dirichlet(0.3) rows over the D * 20 flat actions, a quarter of each row's actions set
    to p = 0."""
    from gymwipe_amd.actions import policy_cdf
    A = D * MAX_DURATION
    tables = np.empty((P, 3, A))
    for pol, pick in enumerate(picks or range(P)):
        rng = np.random.default_rng(1000 * (SEED + pick) + D)
        p = rng.dirichlet(np.full(A, 0.3), size=3)
        for row in p:
            row[rng.permutation(A)[:A // 4]] = 0.0
        tables[pol] = p / p.sum(axis=1, keepdims=True)
    return policy_cdf(tables)


def prep_cols(lo, hi):
    """Columns of the PREP action stream (PREP_N wide) for envs [lo, hi) of a handle wider than the stream."""
    return np.arange(lo, hi) % PREP_N


def gate(tally, causes, who):
    """The tally of an expected trajectory, or an error where it does not exercise what the case is for."""
    by = {1: tally[:, 1], 2: tally[:, 0] - tally[:, 1]}
    for cause in causes:
        if (by[cause] < MIN_EPISODES).any():
            raise RuntimeError("%s: %s episodes per policy ended by cause %d, fewer than %d somewhere"
                               % (who, by[cause].tolist(), cause, MIN_EPISODES))
    if len({tuple(row) for row in tally.tolist()}) != len(tally):
        raise RuntimeError("%s: two policies have the same tally row %s" % (who, tally.tolist()))
    return tally


@functools.lru_cache(maxsize=None)
def population_reference(D, P=P_LONG, M=M_LONG, steps=K_LONG, max_steps=MAX_STEPS, on_done=True, bound=None, causes=(2,), picks=None):
    """The oracle's trajectory of `steps` population steps after the PREP ordinary ones, computed once and read only."""
    n = P * M
    cdfs = population_tables(D, P, picks)
    orc = new_oracle(D, n=n, bound=bound)
    center = CENTER if bound is None else bound
    obs_prev = oracle_prep(orc, D, prep_cols(0, n))
    state = np.zeros((n, 2), np.int32)
    obs_next, tally = oracle_population_steps(orc, cdfs, M, steps, SEED, 0, 0, obs_prev, state, max_steps, on_done, center)
    gate(tally, causes, "population_reference(%d, %d, %d, %d)" % (D, P, M, steps))
    for a in (obs_next, state, tally):
        a.setflags(write=False)
    return {"cdfs": cdfs, "obs_prev": obs_prev, "obs_next": obs_next, "state": state, "tally": tally, "orc": orc, "center": center,
            "P": P, "M": M, "n": n}


def prepared_env(D, ref=None, n=None, lo=0, **kw):
    n = ref["n"] if n is None else n
    env = make_env(D, n=n, **kw)
    gpu_prep(env, D, prep_cols(lo, lo + n))
    return env


def assert_population(env, tally, ref, where, cols=slice(None), rows=slice(None), call_wide=True):
    """The [P][5] tally, the call-wide tally (its column sums), obs_next and {age, ret} against the oracle's."""
    assert tally.cpu().numpy().tolist() == ref["tally"][rows].tolist(), "the per-policy tally differs " + where
    if call_wide:
        assert env.episode_tally.cpu().numpy().tolist() == ref["tally"][rows].sum(axis=0).tolist(), "the call-wide tally differs " + where
    assert (env._last[0].cpu().numpy() == ref["obs_next"][cols]).all(), "obs_next differs " + where
    assert (env.episode_state.cpu().numpy() == ref["state"][cols]).all(), "{age, ret} differs " + where


def pop_launches(env):
    return {k: v for k, v in launches(env).items() if k.startswith("ct_rollout_p")}


# ---- 1. one call ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("D", PARITY_DS)
def test_one_call_matches_the_oracle(D):
    ref = population_reference(D)
    env = prepared_env(D, ref)
    tally = env.rollout_population(ref["cdfs"], K_LONG, SEED, max_steps=MAX_STEPS)
    assert tally.shape == (P_LONG, 5) and str(tally.dtype) == "torch.int64"
    assert_population(env, tally, ref, "after one call of %d steps" % K_LONG)
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after the call")
    dt = D if D in SFX_DTS else 0
    assert pop_launches(env) == {"ct_rollout_pop_ep<%d, 2>" % dt: 3}, launches(env)      # chunks of 64 + 64 + 22
    env.check()
    stats = env.population_stats(tally)
    for pol, (n, by_done, length, ret, sq) in enumerate(ref["tally"].tolist()):
        assert int(stats["episodes"][pol]) == n and int(stats["by_done"][pol]) == by_done
        assert float(stats["mean_length"][pol]) == length / n and float(stats["mean_return"][pol]) == ret / n
        assert abs(float(stats["return_stderr"][pol]) - (max(sq / n - (ret / n) ** 2, 0.0) / n) ** 0.5) <= 1e-12
    import torch
    none = env.population_stats(torch.zeros((2, 5), dtype=torch.int64))
    assert none["episodes"].tolist() == [0, 0] and all(bool(torch.isnan(none[k]).all()) for k in ("mean_length", "mean_return", "return_stderr"))


# ---- 2. both causes -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_done_and_the_step_limit_both_end_episodes():
    """counter_bound = 2 at D = 2: a delivered payload (value 2) reaches the bound, so done fires with the first delivery, and
    an episode reaches the step limit only where five steps in a row deliver nothing.  Tables picked on the oracle alone, among
    the recipe's first 24 seeds, for how often that happens (37, 28 and 16 such episodes per 128 envs; most seeds have none),
    and 512 envs per policy, so that every policy ends MIN_EPISODES episodes that way."""
    ref = population_reference(2, M=M_BOTH, bound=2, causes=(1, 2), picks=BOTH_PICKS)
    env = prepared_env(2, ref, counter_bound=2)
    tally = env.rollout_population(ref["cdfs"], K_LONG, SEED, max_steps=MAX_STEPS, on_done=True)
    assert_population(env, tally, ref, "with both causes")
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="with both causes")


# ---- 3. split calls -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pieces", [(1, 63, 64, 22), (K_LONG,)], ids=["1+63+64+22", "150"])
def test_split_calls_accumulate(pieces):
    """{age, ret} and obs_next are carried in place from call to call; both tallies start from a pattern and are added into."""
    import torch
    D = 4
    ref = population_reference(D)
    env = prepared_env(D, ref)
    wide0 = np.array([3, 1, 1 << 40, -(1 << 33), 7], np.int64)
    rows0 = (np.arange(P_LONG * 5, dtype=np.int64).reshape(P_LONG, 5) * 1000003 - 77) * (1 << 20)
    env.episode_tally.copy_(torch.from_numpy(wide0))
    tally = torch.from_numpy(rows0.copy()).to(env.device)
    s = 0
    for n in pieces:
        assert env.rollout_population(ref["cdfs"], n, SEED, max_steps=MAX_STEPS, step0=s, tally=tally) is tally
        s += n
    where = "over calls of %s steps" % (pieces,)
    assert (tally.cpu().numpy() == rows0 + ref["tally"]).all(), "the per-policy tally differs " + where
    assert (env.episode_tally.cpu().numpy() == wide0 + ref["tally"].sum(axis=0)).all(), "the call-wide tally differs " + where
    assert_population(env, tally - torch.from_numpy(rows0).to(env.device), ref, where, call_wide=False)
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where=where)


# ---- 4. a policy's slice is rollout_episodes under its table ----------------------------------------------------------------------
@pytest.mark.gpu
def test_slices_equal_rollout_episodes():
    """P twin handles of all N envs, each run with ONE of the tables: slice p of the population's handle is slice p of twin p,
    in state, {age, ret} and obs_next -- and the next slice is not, so the comparison tells the tables apart."""
    D = 4
    ref = population_reference(D)
    env = prepared_env(D, ref)
    env.rollout_population(ref["cdfs"], K_LONG, SEED, max_steps=MAX_STEPS)
    state, nxt = env.episode_state.cpu().numpy(), env._last[0].cpu().numpy()
    for pol in range(P_LONG):
        s = slice(pol * M_LONG, (pol + 1) * M_LONG)
        twin = prepared_env(D, ref)
        twin.rollout_episodes(ref["cdfs"][pol], K_LONG, SEED, max_steps=MAX_STEPS)
        assert (twin.episode_state.cpu().numpy()[s] == state[s]).all() and (twin._last[0].cpu().numpy()[s] == nxt[s]).all(), pol
        for f in STATE_FIELDS + STAT_FIELDS:
            assert (env.get_state(f)[s].view(np.uint8) == twin.get_state(f)[s].view(np.uint8)).all(), (f, pol)
        other = slice(((pol + 1) % P_LONG) * M_LONG, ((pol + 1) % P_LONG + 1) * M_LONG)
        assert any((env.get_state(f)[other].view(np.uint8) != twin.get_state(f)[other].view(np.uint8)).any()
                   for f in STATE_FIELDS + STAT_FIELDS), pol            # (another table: another trajectory)


# ---- 5. shards --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_shards_equal_one_handle():
    """Handles of P / 2 policies each, the second with env_id0 = N / 2: the stream is shifted, the policy index is the handle's
    own.  The two tallies stacked are the one handle's."""
    import torch
    D = 4
    ref = population_reference(D, P_INST, M_INST, K_INST)
    half, rows = ref["n"] // 2, []
    for lo in (0, half):
        cols, pols = slice(lo, lo + half), slice(lo // M_INST, (lo + half) // M_INST)
        env = prepared_env(D, n=half, lo=lo)
        tally = env.rollout_population(ref["cdfs"][pols], K_INST, SEED, max_steps=MAX_STEPS, env_id0=lo)
        assert_population(env, tally, ref, "in the shard at %d" % lo, cols, pols)
        for f in STATE_FIELDS + STAT_FIELDS:
            assert (env.get_state(f).view(np.uint8) == ref["orc"].get(f)[cols].view(np.uint8)).all(), (f, lo)
        rows.append(tally)
    assert torch.cat(rows).cpu().numpy().tolist() == ref["tally"].tolist()


# ---- 6. the per-step form ---------------------------------------------------------------------------------------------------------
K_OTHER = 24
OTHER = {                               # kind: (D, P, M, handle)
    "odd_m": (4, 4, 50, {}),                                            # N = 200: one bookkeeping block over four policies
    "explicit_queue": (3, 3, 128, {"explicit_queue": True}),            # N = 384: a block over two policies, a block in one
    "per_env_geometry": (4, 3, 128, {"per_env_geometry": True}),
    "unfused_switch": (4, 3, 128, {}),
}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(OTHER))
def test_calls_without_a_fused_form_run_per_step(kind, monkeypatch):
    import torch
    from gymwipe_amd import _native as nat
    D, P, M, kw = OTHER[kind]
    n = P * M
    cdfs = population_tables(D, P)
    env, orc = make_env(D, n=n, **kw), new_oracle(D, n=n)
    bytes0 = env.state_bytes()
    if kind == "unfused_switch":
        monkeypatch.setenv("GW_ROLLOUT_POLICY_UNFUSED", "1")
    monkeypatch.setenv("GW_ROLLOUT_STRICT", "1")                         # refused on a fresh handle: nothing allocated
    env.reset()
    with pytest.raises(nat.NativeError) as exc:
        env.rollout_population(cdfs, 4, SEED, max_steps=MAX_STEPS)
    assert exc.value.code == nat.EUNSUPPORTED and env.state_bytes() == bytes0
    monkeypatch.delenv("GW_ROLLOUT_STRICT")
    gpu_prep(env, D, prep_cols(0, n))
    acts_on = oracle_prep(orc, D, prep_cols(0, n))
    state, want = np.zeros((n, 2), np.int32), np.zeros((P, 5), np.int64)
    before = launches(env)
    tally = None
    for call in range(2):
        tally = env.rollout_population(cdfs, K_OTHER, SEED, max_steps=MAX_STEPS, step0=call * K_OTHER, tally=tally)
        acts_on, t = oracle_population_steps(orc, cdfs, M, K_OTHER, SEED, call * K_OTHER, 0, acts_on, state, MAX_STEPS, True)
        want += t
    ref = {"tally": gate(want, (2,), kind), "obs_next": acts_on, "state": state}
    assert_population(env, tally, ref, "after two calls (%s)" % kind)
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
    assert env.state_bytes() >= bytes0 + 18 * n                         # the six rows, counted once they exist
    bytes1 = env.state_bytes()
    # refused under GW_ROLLOUT_STRICT before anything is launched: state and tallies unchanged
    monkeypatch.setenv("GW_ROLLOUT_STRICT", "1")
    snap, kept = env.snapshot(), (tally.clone(), env.episode_tally.clone(), env.episode_state.clone(), env._last[0].clone())
    with pytest.raises(nat.NativeError) as exc:
        env.rollout_population(cdfs, 4, SEED, max_steps=MAX_STEPS, step0=2 * K_OTHER, tally=tally)
    assert exc.value.code == nat.EUNSUPPORTED
    assert delta(launches(env), before) == ran and env.state_bytes() == bytes1
    assert (env.snapshot() == snap).all()
    for a, b in zip(kept, (tally, env.episode_tally, env.episode_state, env._last[0])):
        assert torch.equal(a, b)


# ---- 7. one case per instantiation ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(INSTANTIATIONS))
def test_instantiation_matches_the_oracle(name, monkeypatch):
    dt, mode = INSTANTIATIONS[name]
    D = dt if dt else 11
    for k, v in dict(MODE_SWITCHES[mode], GW_ROLLOUT_STRICT="1").items():
        monkeypatch.setenv(k, v)
    ref = population_reference(D, P_INST, M_INST, K_INST)               # (shared by the three modes of a sender count)
    env = prepared_env(D, ref)
    before = launches(env)
    tally = env.rollout_population(ref["cdfs"], K_INST, SEED, max_steps=MAX_STEPS)
    assert_population(env, tally, ref, "after %s" % name)
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after %s" % name)
    assert delta(launches(env), before) == {name: 1}, launches(env)     # the target, and no step or reset kernel


# ---- 8. errors ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_errors():
    import torch
    from gymwipe_amd import _native as nat
    from test_interpreter_plugin import _reference_interpreter
    D = 4
    n = P_INST * M_INST
    cdfs = population_tables(D, P_INST)
    env = prepared_env(D, n=n)
    before = launches(env)
    table = env._policy_table(cdfs, population=True)
    tally = torch.zeros((P_INST, 5), dtype=torch.int64, device=env.device)
    ep = nat.Episodes(MAX_STEPS, 1, env.episode_state.data_ptr(), env.episode_tally.data_ptr())
    nxt = torch.empty(n, dtype=torch.int32, device=env.device)
    for P, M in ((P_INST, M_INST - 1), (P_INST - 1, M_INST), (P_INST, 2 * M_INST), (1 << 16, 1 << 16)):
        pop = nat.Population(P, M, table.data_ptr(), tally.data_ptr())
        rc = nat.lib().gw_rollout_population(env._h, 4, C.byref(pop), SEED, 0, 0, C.byref(ep), env._last[0].data_ptr(), nxt.data_ptr(), None)
        assert rc == nat.EINVAL and b"envs" in nat.lib().gw_last_error(), (P, M)
    torch.cuda.synchronize()
    assert launches(env) == before and int(tally.abs().sum()) == 0 and int(env.episode_tally.abs().sum()) == 0
    for bad in (cdfs[0], cdfs[:, :2], cdfs[:, :, :-1], cdfs[:3]):       # (three policies do not divide 256 envs)
        with pytest.raises(ValueError):
            env.rollout_population(bad, 4, SEED, max_steps=MAX_STEPS)
    with pytest.raises(ValueError):
        env.rollout_population(cdfs, 4, SEED, max_steps=MAX_STEPS, tally=torch.zeros((P_INST, 4), dtype=torch.int64, device=env.device))
    assert launches(env) == before
    plug = make_env(2, n=n, interpreter=_reference_interpreter(torch, n, 2, CENTER, torch.device("cuda:0")))
    plug.reset()
    with pytest.raises(ValueError):
        plug.rollout_population(population_tables(2, P_INST), 4, SEED, max_steps=MAX_STEPS)


@pytest.mark.gpu
def test_without_limits_nothing_is_tallied_and_each_slice_is_rollout_policy():
    """max_steps = 0, on_done = 0: every tally untouched, and slice p walks gw_rollout_policy's trajectory under table p."""
    D = 4
    n = P_INST * M_INST
    cdfs = population_tables(D, P_INST)
    env = prepared_env(D, n=n)
    tally = env.rollout_population(cdfs, K_INST, SEED, max_steps=0, on_done=False)
    assert int(tally.abs().sum()) == 0 and int(env.episode_tally.abs().sum()) == 0
    assert (env.episode_state[:, 0] == K_INST).all()
    for pol in range(P_INST):
        s = slice(pol * M_INST, (pol + 1) * M_INST)
        twin = prepared_env(D, n=n)
        out = twin.rollout_policy(cdfs[pol], K_INST, SEED)
        assert (out[2][-1][s] == env._last[0][s]).all() and (out[3].sum(dim=0).int()[s] == env.episode_state[s, 1]).all(), pol
        for f in STATE_FIELDS + STAT_FIELDS:
            assert (env.get_state(f)[s].view(np.uint8) == twin.get_state(f)[s].view(np.uint8)).all(), (f, pol)


# ---- 9. the agent -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_population_search_agent_equals_the_oracle_backed_run():
    from gymwipe_amd.agents import PopulationSearchAgent
    want = oracle_agent()
    want.fit(AGENT["generations"])
    env = make_env(AGENT["D"], n=AGENT["P"] * AGENT["M"])
    agent = PopulationSearchAgent(env, AGENT["P"], AGENT["steps"], AGENT["episode_steps"], seed=AGENT["seed"])
    assert agent.nb_actions == AGENT["D"] * MAX_DURATION
    agent.fit(AGENT["generations"])
    assert_same_history(agent.history, want.history)
    assert (agent.mu == want.mu).all() and (agent.sigma == want.sigma).all()
    assert not [k for k in launches(env) if "_ep<" in k]                # (M = 16: the per-step form)
    env.check()
