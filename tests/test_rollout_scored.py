"""
gw_rollout_episodes_scored / gw_rollout_population_scored on the GPU: the fused closed loops with the step's score --
w_reward * reward + w_delivered[sender] * packets the RRM decoded -- where their parents carry the reward
(ct_rollout_policy_eps<DT, MODE>, ct_rollout_pop_eps<DT, MODE>), and the per-step form of the handles without a fused one.

Every expected value comes from the oracle alone (oracle_scored_steps() / oracle_scored_population_steps() in
tests/test_rollout_scored_cpu.py).  All comparisons are exact, the state included (STATE_FIELDS + STAT_FIELDS).  An expected
trajectory must exercise what it is for: the reference builders raise, instead of letting a test pass, unless enough episodes
ended, at least two different senders delivered packets and the score differs from w_reward * reward (records form); unless
two policies' tally rows differ and the rows differ from the unscored tally (population) -- so a kernel that ignores the
sender, that keeps the delivered baseline across launches (STEPS crosses the 64-step launch boundary) or that scores the
reward only must fail.  Shapes are the smallest that can go wrong: N = 160 is three blocks, the last one half full.
tests/test_rollout_scored_cpu.py checks on the CPU that the two INSTANTIATIONS sets are exactly the library's.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_kernel_variants import SFX_DTS, launches
from test_rollout_episodes import MAX_STEPS, MIN_EPISODES
from test_rollout_policy import SEED, delta, gpu_prep, make_env, oracle_prep, policy_table
from test_rollout_population import population_tables
from test_rollout_scored_cpu import NAMES, new_oracle, oracle_scored_population_steps, oracle_scored_steps
from util import assert_state_equal, STATE_FIELDS, STAT_FIELDS

INSTANTIATIONS = {"ct_rollout_policy_eps<%d, %d>" % (dt, mode): (dt, mode) for dt in SFX_DTS + (0,) for mode in (2, 1, 0)}
POP_INSTANTIATIONS = {"ct_rollout_pop_eps<%d, %d>" % (dt, mode): (dt, mode) for dt in SFX_DTS + (0,) for mode in (2, 1, 0)}
N, STEPS = 160, 70                      # three blocks, the last half full; launches of 64 + 6 steps
DS = (2, 4, 16, 9)                      # 9: no kernel of its own (DT == 0)
POPS = ((3, 128), (4, 64))              # a policy spans two blocks; one block per policy


def case_score(D):
    """w_reward = 3 and a weight per sender, all distinct, every third one negative."""
    from gymwipe_amd.actions import make_score
    return make_score(D, reward=3, delivered=[(5 + 2 * d) * (-1 if d % 3 == 2 else 1) for d in range(D)])


def scored_launches(env):
    return {k: v for k, v in launches(env).items() if "_eps<" in k}


def fused_name(family, D):
    return "%s<%d, 2>" % (family, D if D in SFX_DTS else 0)


def gated(out, plain, tally, score, who):
    if tally[0] < MIN_EPISODES:
        raise RuntimeError("%s: %d episodes ended, fewer than %d" % (who, tally[0], MIN_EPISODES))
    senders = np.unique(out[0][out[6] > 0])
    if len(senders) < 2:
        raise RuntimeError("%s: only senders %s delivered packets" % (who, senders.tolist()))
    if not (out[3] != int(score[0]) * plain).any():
        raise RuntimeError("%s: the score is w_reward * reward in every step" % who)


@functools.lru_cache(maxsize=None)
def scored_reference(D, n=N, steps=STEPS):
    """The oracle's trajectory of `steps` scored episodic steps after the PREP ordinary ones, computed once and read only."""
    _, cdf = policy_table(D)
    score = case_score(D)
    orc = new_oracle(D, n)
    obs_prev = oracle_prep(orc, D, slice(0, n))
    state = np.zeros((n, 2), np.int32)
    out, plain, obs_next, tally = oracle_scored_steps(orc, cdf, score, steps, SEED, 0, 0, obs_prev, state, MAX_STEPS, True)
    gated(out, plain, tally, score, "scored_reference(%d, %d, %d)" % (D, n, steps))
    for a in out + (obs_next, state, tally, score):
        a.setflags(write=False)
    return {"cdf": cdf, "score": score, "out": out, "obs_next": obs_next, "state": state, "tally": tally, "orc": orc, "n": n}


@functools.lru_cache(maxsize=None)
def population_reference(D, P, M, steps=STEPS):
    from gymwipe_amd.actions import make_score
    n = P * M
    cdfs, score = population_tables(D, P), case_score(D)
    runs = []
    for sc in (score, make_score(D)):                                   # the second: what the unscored call would tally
        orc = new_oracle(D, n)
        obs_prev = oracle_prep(orc, D, np.arange(n) % 200)
        state = np.zeros((n, 2), np.int32)
        runs.append(oracle_scored_population_steps(orc, cdfs, M, sc, steps, SEED, 0, 0, obs_prev, state, MAX_STEPS, True) + (state, orc))
    (obs_next, tally, packets, state, orc), plain = runs[0], runs[1]
    who = "population_reference(%d, %d, %d)" % (D, P, M)
    if (tally[:, 0] < MIN_EPISODES).any():
        raise RuntimeError("%s: %s episodes per policy, fewer than %d somewhere" % (who, tally[:, 0].tolist(), MIN_EPISODES))
    if len({tuple(row) for row in tally.tolist()}) != P:
        raise RuntimeError("%s: two policies have the same tally row" % who)
    if (tally[:, 3:] == plain[1][:, 3:]).all(axis=1).any() or not (tally[:, :3] == plain[1][:, :3]).all():
        raise RuntimeError("%s: a policy's scored row is its unscored row, or the score changed the episodes" % who)
    if (packets == 0).any():
        raise RuntimeError("%s: a policy delivered nothing" % who)
    for a in (obs_next, tally, state):
        a.setflags(write=False)
    return {"cdfs": cdfs, "score": score, "obs_next": obs_next, "tally": tally, "state": state, "orc": orc, "n": n, "P": P, "M": M}


def prepared_env(D, n, lo=0, **kw):
    env = make_env(D, n=n, **kw)
    gpu_prep(env, D, np.arange(lo, lo + n) % 200)
    return env


def assert_outputs(got, want, where):
    assert len(got) == len(want) == 7
    for name, g, w in zip(NAMES, got, want):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (name, where)
        assert (g.view(np.uint8) == w.view(np.uint8)).all(), \
            "%s differs %s, first at (step, env) %s" % (name, where, np.argwhere(g != w)[:3].tolist())


def assert_episodes(env, ref, where, cols=slice(None), tally=None):
    assert (env._last[0].cpu().numpy() == ref["obs_next"][cols]).all(), "obs_next differs " + where
    assert (env.episode_state.cpu().numpy() == ref["state"][cols]).all(), "{age, ret} differs " + where
    if tally is not None:
        assert env.episode_tally.cpu().numpy().tolist() == np.asarray(tally).tolist(), "the call-wide tally differs " + where


def fields_without_rx_power(env, orc):
    """The state fields to compare exactly on a live-PHY handle (received power as tests/test_rollout_policy.py bounds it)."""
    a, b = env.get_state("rx_power"), orc.get("rx_power")
    assert np.max(np.abs(a - b) / b) < 1e-5
    return tuple(f for f in STATE_FIELDS + STAT_FIELDS if f != "rx_power")


# ---- 1. the records form ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("D", DS)
def test_records_form_matches_the_oracle(D):
    ref = scored_reference(D)
    env = prepared_env(D, N)
    got = env.rollout_episodes(ref["cdf"], STEPS, SEED, max_steps=MAX_STEPS, score=ref["score"])
    assert_outputs(got, ref["out"], "in one call of %d steps" % STEPS)
    assert_episodes(env, ref, "after the call", tally=ref["tally"])
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after the call")
    assert scored_launches(env) == {fused_name("ct_rollout_policy_eps", D): 2}, launches(env)      # 64 + 6 steps
    assert not [k for k in launches(env) if "_ep<" in k]
    env.check()


@pytest.mark.gpu
def test_records_form_in_split_calls_and_into_the_callers_rows():
    import torch
    D = 4
    ref = scored_reference(D)
    env = prepared_env(D, N)
    kinds = (torch.int32, torch.int32, torch.int32, torch.float32, torch.uint8, torch.uint8, torch.int32)
    rows = tuple(torch.empty((STEPS, N), dtype=t, device=env.device) for t in kinds)
    s = 0
    for n in (1, 63, 6):
        out = tuple(r[s:s + n] for r in rows)
        back = env.rollout_episodes(ref["cdf"], n, SEED, max_steps=MAX_STEPS, step0=s, out=out, score=ref["score"])
        assert len(back) == 7 and all(a is b for a, b in zip(back, out))
        s += n
    assert_outputs(rows, ref["out"], "over calls of 1 + 63 + 6 steps")
    assert_episodes(env, ref, "after the split calls", tally=ref["tally"])
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after the split calls")


# ---- 2. the neutral score is the parent --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_neutral_score_gives_the_parents_results():
    from gymwipe_amd.actions import make_score
    D = 4
    _, cdf = policy_table(D)
    env, twin = prepared_env(D, N), prepared_env(D, N)
    got = env.rollout_episodes(cdf, STEPS, SEED, max_steps=MAX_STEPS, score=make_score(D, reward=1, delivered=0))
    want = twin.rollout_episodes(cdf, STEPS, SEED, max_steps=MAX_STEPS)
    assert len(got) == 7 and len(want) == 6
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and (g.cpu().numpy().view(np.uint8) == w.cpu().numpy().view(np.uint8)).all(), name
    assert (got[6].cpu().numpy() == scored_reference(D)["out"][6]).all()           # (the score changes no trajectory)
    P, M = POPS[1]
    cdfs = population_tables(D, P)
    penv, ptwin = prepared_env(D, P * M), prepared_env(D, P * M)
    t1 = penv.rollout_population(cdfs, STEPS, SEED, max_steps=MAX_STEPS, score=make_score(D))
    t2 = ptwin.rollout_population(cdfs, STEPS, SEED, max_steps=MAX_STEPS)
    assert t1.cpu().numpy().tolist() == t2.cpu().numpy().tolist() and int(t1[:, 0].min()) >= MIN_EPISODES
    for a, b in ((env, twin), (penv, ptwin)):
        assert (a.episode_state == b.episode_state).all() and (a.episode_tally == b.episode_tally).all()
        assert (a._last[0] == b._last[0]).all()
        for f in STATE_FIELDS + STAT_FIELDS:
            assert (a.get_state(f).view(np.uint8) == b.get_state(f).view(np.uint8)).all(), f
    assert scored_launches(env) and scored_launches(penv) and not scored_launches(twin) and not scored_launches(ptwin)


# ---- 3. the population --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("D,P,M", [(D, 3, 128) for D in DS] + [(4, 4, 64)])
def test_population_matches_the_oracle(D, P, M):
    ref = population_reference(D, P, M)
    env = prepared_env(D, ref["n"])
    tally = env.rollout_population(ref["cdfs"], STEPS, SEED, max_steps=MAX_STEPS, score=ref["score"])
    assert tally.cpu().numpy().tolist() == ref["tally"].tolist(), "the per-policy tally differs"
    assert_episodes(env, ref, "after the call", tally=ref["tally"].sum(axis=0))
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after the call")
    assert scored_launches(env) == {fused_name("ct_rollout_pop_eps", D): 2}, launches(env)
    assert not [k for k in launches(env) if "_ep<" in k]
    env.check()


@pytest.mark.gpu
def test_population_in_two_slices_equals_one_call():
    """Two handles of P / 2 policies each, the second with env_id0 = N / 2; and the calls split at the launch boundary."""
    import torch
    D, (P, M) = 4, POPS[1]
    ref = population_reference(D, P, M)
    half, rows = ref["n"] // 2, []
    for lo in (0, half):
        cols, pols = slice(lo, lo + half), slice(lo // M, (lo + half) // M)
        env = prepared_env(D, half, lo=lo)
        tally = None
        for s, n in ((0, 64), (64, STEPS - 64)):
            tally = env.rollout_population(ref["cdfs"][pols], n, SEED, max_steps=MAX_STEPS, step0=s, env_id0=lo, tally=tally,
                                           score=ref["score"])
        assert tally.cpu().numpy().tolist() == ref["tally"][pols].tolist(), lo
        assert_episodes(env, ref, "in the slice at %d" % lo, cols, tally=ref["tally"][pols].sum(axis=0))
        for f in STATE_FIELDS + STAT_FIELDS:
            assert (env.get_state(f).view(np.uint8) == ref["orc"].get(f)[cols].view(np.uint8)).all(), (f, lo)
        rows.append(tally)
    assert torch.cat(rows).cpu().numpy().tolist() == ref["tally"].tolist()


# ---- 4. the per-step form -------------------------------------------------------------------------------------------------------------
def refused_under_strict(env, call, monkeypatch):
    from gymwipe_amd import _native as nat
    bytes0, before = env.state_bytes(), launches(env)
    monkeypatch.setenv("GW_ROLLOUT_STRICT", "1")
    with pytest.raises(nat.NativeError) as exc:
        call()
    monkeypatch.delenv("GW_ROLLOUT_STRICT")
    assert exc.value.code == nat.EUNSUPPORTED and env.state_bytes() == bytes0 and launches(env) == before


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["unfused_switch", "per_env_geometry"])
def test_records_form_per_step(kind, monkeypatch):
    D = 4
    n = N if kind == "unfused_switch" else 64
    kw = {} if kind == "unfused_switch" else {"per_env_geometry": True}
    if kind == "unfused_switch":
        monkeypatch.setenv("GW_ROLLOUT_POLICY_UNFUSED", "1")
    ref = scored_reference(D, n)
    env = make_env(D, n=n, **kw)
    env.reset()
    refused_under_strict(env, lambda: env.rollout_episodes(ref["cdf"], 4, SEED, max_steps=MAX_STEPS, score=ref["score"]), monkeypatch)
    gpu_prep(env, D, slice(0, n))
    bytes0, before = env.state_bytes(), launches(env)
    got = env.rollout_episodes(ref["cdf"], STEPS, SEED, max_steps=MAX_STEPS, score=ref["score"])
    assert_outputs(got, ref["out"], "per step (%s)" % kind)
    assert_episodes(env, ref, "per step (%s)" % kind, tally=ref["tally"])
    fields = STATE_FIELDS + STAT_FIELDS if kind == "unfused_switch" else fields_without_rx_power(env, ref["orc"])
    assert_state_equal(env, ref["orc"], fields, where="per step (%s)" % kind)
    ran = delta(launches(env), before)
    assert not scored_launches(env) and not [k for k in launches(env) if "_ep<" in k], ran
    assert sum(v for k, v in ran.items() if k.startswith("ct_step")) == STEPS and len(ran) == 1, ran
    assert env.state_bytes() == bytes0 + 4 * n                          # the delivered counters' row, counted once it exists
    refused_under_strict(env, lambda: env.rollout_episodes(ref["cdf"], 4, SEED, max_steps=MAX_STEPS, step0=STEPS, score=ref["score"]),
                         monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["m96", "unfused_switch", "m50"])
def test_population_per_step(kind, monkeypatch):
    """The bookkeeping kernel's blocks are 256 envs.  unfused_switch, 3 x 128: the first block spans two policies (each ended
    episode's words go to its policy's row directly), the second lies in one (summed in LDS, added to the row once).  m50,
    4 x 50: one block, not full, over four policies.  m96, 2 x 96: one block over two."""
    D = 4
    P, M = {"m96": (2, 96), "unfused_switch": POPS[0], "m50": (4, 50)}[kind]
    if kind == "unfused_switch":
        monkeypatch.setenv("GW_ROLLOUT_POLICY_UNFUSED", "1")
    ref = population_reference(D, P, M)
    env = make_env(D, n=ref["n"])
    env.reset()
    refused_under_strict(env, lambda: env.rollout_population(ref["cdfs"], 4, SEED, max_steps=MAX_STEPS, score=ref["score"]), monkeypatch)
    gpu_prep(env, D, np.arange(ref["n"]) % 200)
    bytes0, before = env.state_bytes(), launches(env)
    tally = env.rollout_population(ref["cdfs"], STEPS, SEED, max_steps=MAX_STEPS, score=ref["score"])
    assert tally.cpu().numpy().tolist() == ref["tally"].tolist(), "the per-policy tally differs (%s)" % kind
    assert_episodes(env, ref, "per step (%s)" % kind, tally=ref["tally"].sum(axis=0))
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="per step (%s)" % kind)
    ran = delta(launches(env), before)
    assert not scored_launches(env) and not [k for k in launches(env) if "_ep<" in k], ran
    assert sum(v for k, v in ran.items() if k.startswith("ct_step")) == STEPS and len(ran) == 1, ran
    assert env.state_bytes() >= bytes0 + 22 * ref["n"]                  # the six rows and the delivered counters' row


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals():
    import torch
    from gymwipe_amd import _native as nat
    from gymwipe_amd.actions import make_score
    D = 4
    P, M = POPS[1]
    n = P * M
    L = nat.lib()
    env = prepared_env(D, n)
    before, bytes0 = launches(env), env.state_bytes()
    _, cdf = policy_table(D)
    table = env._policy_table(cdf)
    tables = env._policy_table(population_tables(D, P), population=True)
    rows = [torch.zeros((4, n), dtype=t, device=env.device)
            for t in (torch.int32, torch.int32, torch.int32, torch.float32, torch.uint8, torch.uint8, torch.int32)]
    tally = torch.zeros((P, 5), dtype=torch.int64, device=env.device)
    ep = nat.Episodes(MAX_STEPS, 1, env.episode_state.data_ptr(), env.episode_tally.data_ptr())
    pop = nat.Population(P, M, tables.data_ptr(), tally.data_ptr())
    nxt = torch.empty(n, dtype=torch.int32, device=env.device)
    prev = env._last[0].clone()

    def image(index=None, value=0):
        w = make_score(D, 1, 3)
        if index is not None:
            w[index] = value
        return nat.Score.from_buffer_copy(w.tobytes())

    def episodes(score, steps=4, delivered=rows[6].data_ptr()):
        return L.gw_rollout_episodes_scored(env._h, steps, table.data_ptr(), SEED, 0, 0, C.byref(ep),
                                            C.byref(score) if score is not None else None, prev.data_ptr(), nxt.data_ptr(),
                                            *[r.data_ptr() for r in rows[:6]], delivered, None)

    def population(score, steps=4):
        return L.gw_rollout_population_scored(env._h, steps, C.byref(pop), SEED, 0, 0, C.byref(ep),
                                              C.byref(score) if score is not None else None, prev.data_ptr(), nxt.data_ptr(), None)

    for call in (episodes, population):
        for bad in (image(0, nat.SCORE_W_MAX + 1), image(2, nat.SCORE_W_MAX + 1), image(1, -nat.SCORE_W_MAX - 1)):
            assert call(bad) == nat.EINVAL and b"weight" in L.gw_last_error()
        assert call(None) == nat.EINVAL and b"NULL" in L.gw_last_error()
        assert call(image(), steps=0) == nat.OK
        assert call(image(), steps=-1) == nat.EINVAL
    assert episodes(image(), delivered=None) == nat.EINVAL and b"NULL" in L.gw_last_error()
    torch.cuda.synchronize()
    assert launches(env) == before and env.state_bytes() == bytes0
    assert int(tally.abs().sum()) == 0 and int(env.episode_tally.abs().sum()) == 0 and all(int(r.abs().sum()) == 0 for r in rows)
    for bad in (make_score(D)[:5], make_score(D).astype(np.float64), np.full(33, 2000, np.int32)):
        with pytest.raises(ValueError):
            env.rollout_population(population_tables(D, P), 4, SEED, max_steps=MAX_STEPS, score=bad)
    # an explicit-queue handle keeps no delivered counter per env
    xq = make_env(3, n=128, explicit_queue=True)
    xq.reset()
    was = launches(xq)
    _, cdf3 = policy_table(3)
    for call in (lambda: xq.rollout_episodes(cdf3, 4, SEED, max_steps=MAX_STEPS, score=make_score(3, 0, 1)),
                 lambda: xq.rollout_population(population_tables(3, 2), 4, SEED, max_steps=MAX_STEPS, score=make_score(3, 0, 1))):
        with pytest.raises(nat.NativeError) as exc:
            call()
        assert exc.value.code == nat.EUNSUPPORTED
    assert launches(xq) == was


# ---- 7. the agent -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_population_search_agent_equals_the_oracle_backed_run():
    from gymwipe_amd.agents import PopulationSearchAgent
    from test_rollout_scored_cpu import AGENT, oracle_agent
    want = oracle_agent()
    want.fit(AGENT["generations"])
    env = make_env(AGENT["D"], n=AGENT["P"] * AGENT["M"])
    agent = PopulationSearchAgent(env, AGENT["P"], AGENT["steps"], AGENT["episode_steps"], seed=AGENT["seed"], score=want.score)
    agent.fit(AGENT["generations"])
    for x, y in zip(agent.history, want.history):
        assert x["mean"] == y["mean"] and x["best"] == y["best"] and (x["fitness"] == y["fitness"]).all(), x["generation"]
    assert (agent.mu == want.mu).all() and (agent.sigma == want.sigma).all()
    env.check()
