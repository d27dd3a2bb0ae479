"""
gw_rollout_autoreset_scored on the GPU: gw_rollout_autoreset's staged actions and in-launch resets with the step's score --
w_reward * reward + w_delivered[staged sender] * packets the RRM decoded -- where the parent carries the reward
(ct_rollout_sync_eps<DT, MODE>), its one-step form env.step_autoreset(score=), the per-step form of the handles without a fused
rollout, and DqnCounterTrafficAgent.fit(score=) on top of it.

Every expected value comes from the oracle alone (oracle_scored_autoreset_steps() / rejected_reference() in
tests/test_rollout_autoreset_scored_cpu.py).  All comparisons are exact, the state included (STATE_FIELDS + STAT_FIELDS).
scored_autoreset_reference() raises, instead of letting a test pass, when fewer than MIN_EPISODES episodes end by a cause the
case is meant to exercise, when the case delivers no packet, or when the score differs from the built-in reward in fewer than a
quarter of its env-steps.  Figures of the references, from the CPU oracle: D in (2, 4, 5, 9, 32) at K = 150: 6 000 episodes per
case, all by the step limit, 61 501 ... 62 174 packets, the score differs from the reward in 22 860 ... 23 100 of 30 000
env-steps; D = 4 at K = 40: 1 600 episodes, 17 787 packets, 6 168 of 8 000; the `both` stream at counter_bound = 2, D = 4:
12 732 episodes by done and 864 by the limit, 58 441 packets, 12 732 of 30 000.
tests/test_rollout_autoreset_scored_cpu.py checks on the CPU that INSTANTIATIONS is exactly the library's set.
"""
import functools

import numpy as np
import pytest

from test_kernel_variants import MODE_SWITCHES, SFX_DTS, launches
from test_rollout_autoreset import FLAG_BADACT, ended_by, ep_launches, staged, staged_actions
from test_rollout_autoreset_scored_cpu import (BAD_STEP, NAMES, case_score, oracle_scored_autoreset_steps, rejected_reference)
from test_rollout_episodes import MAX_STEPS, MIN_EPISODES, new_oracle
from test_rollout_policy import CENTER, K_INST, K_LONG, N, PARITY_DS, delta, make_env
from util import assert_state_equal, STATE_FIELDS, STAT_FIELDS

INSTANTIATIONS = {"ct_rollout_sync_eps<%d, %d>" % (dt, mode): (dt, mode) for dt in SFX_DTS + (0,) for mode in (2, 1, 0)}


@functools.lru_cache(maxsize=None)
def scored_autoreset_reference(D, steps=K_LONG, max_steps=MAX_STEPS, on_done=True, both=False, causes=(2,)):
    """The oracle's scored trajectory over the staged rows after a reset, computed once and read only.  `causes`: the ways an
    episode ends that the case is meant to exercise (1 done, 2 step limit)."""
    bound = 2 if both else None
    dev, dur = staged_actions(D, steps, both)
    score = case_score(D)
    orc = new_oracle(D, bound=bound)
    center = CENTER if bound is None else bound
    orc.reset()
    state = np.zeros((N, 2), np.int32)
    out, plain, obs_next, tally = oracle_scored_autoreset_steps(orc, dev, dur, score, state, max_steps, on_done, center)
    who = "scored_autoreset_reference(%d, %d, on_done=%s, both=%s)" % (D, steps, on_done, both)
    by = ended_by(tally)
    for cause in causes:
        if by[cause] < MIN_EPISODES:
            raise RuntimeError("%s: %d episodes ended by cause %d, fewer than %d" % (who, by[cause], cause, MIN_EPISODES))
    if int(out[4].sum()) == 0:
        raise RuntimeError("%s: no packet was delivered" % who)
    if 4 * int((out[1] != plain).sum()) < out[1].size:
        raise RuntimeError("%s: the score differs from the reward in %d of %d env-steps, fewer than a quarter"
                           % (who, int((out[1] != plain).sum()), out[1].size))
    assert tally[0] == (out[3] != 0).sum() and tally[1] == (out[3] == 1).sum()
    for a in out + (obs_next, state, tally, dev, dur, score):
        a.setflags(write=False)
    return {"dev": dev, "dur": dur, "score": score, "out": out, "obs_next": obs_next, "state": state, "tally": tally, "orc": orc,
            "center": center}


def assert_outputs(got, want, where):
    assert len(got) == len(want) == 5
    for name, g, w in zip(NAMES, got, want):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (name, where)
        assert (g.view(np.uint8) == w.view(np.uint8)).all(), \
            "%s differs %s, first at (step, env) %s" % (name, where, np.argwhere(g != w)[:3].tolist())


def assert_episodes(env, ref, where, tally=True):
    assert (env._last[0].cpu().numpy() == ref["obs_next"]).all(), "obs_next differs " + where
    assert (env.episode_state.cpu().numpy() == ref["state"]).all(), "{age, ret} differs " + where
    if tally:
        assert env.episode_tally.cpu().numpy().tolist() == ref["tally"].tolist(), "tally differs " + where


def step_outputs(n=N):
    import torch
    from gymwipe_amd import StepOutputs
    return StepOutputs(torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda"),
                       torch.empty(n, dtype=torch.uint8, device="cuda"), ended=torch.empty(n, dtype=torch.uint8, device="cuda"),
                       delivered=torch.empty(n, dtype=torch.int32, device="cuda"))


# ---- 1. one call ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("D", PARITY_DS)
def test_one_call_matches_the_oracle(D):
    ref = scored_autoreset_reference(D)
    env = make_env(D)
    env.reset()
    got = env.rollout_autoreset(*staged(ref), max_steps=MAX_STEPS, score=ref["score"])
    assert_outputs(got, ref["out"], "in one call of %d steps" % K_LONG)
    assert_episodes(env, ref, "after the call")
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after the call")
    dt = D if D in SFX_DTS else 0
    assert ep_launches(env) == {"ct_rollout_sync_eps<%d, 2>" % dt: 3}, launches(env)
    n, _, _, ret, _ = (int(x) for x in ref["tally"])
    assert env.episode_stats()["mean_return"] == ret / n
    env.check()


# ---- 2. both causes -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("on_done", [True, False])
def test_done_and_the_step_limit_both_end_episodes(on_done):
    """counter_bound = 2: a delivered payload reaches the bound, so done fires with the first delivery; a row of duration 0
    delivers nothing.  on_done=False on the same rows: done never ends an episode."""
    D = 4
    ref = scored_autoreset_reference(D, on_done=on_done, both=True, causes=(1, 2) if on_done else (2,))
    if not on_done:
        assert set(np.unique(ref["out"][3]).tolist()) == {0, 2} and int(ref["out"][2].sum()) >= MIN_EPISODES
    env = make_env(D, counter_bound=2)
    env.reset()
    got = env.rollout_autoreset(*staged(ref), max_steps=MAX_STEPS, on_done=on_done, score=ref["score"])
    assert_outputs(got, ref["out"], "with both causes (on_done=%s)" % on_done)
    assert_episodes(env, ref, "with both causes (on_done=%s)" % on_done)
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="with both causes (on_done=%s)" % on_done)


# ---- 3. the neutral score is the parent ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_neutral_score_gives_the_parents_results():
    import torch
    from gymwipe_amd.actions import make_score
    D = 4
    ref = scored_autoreset_reference(D)
    env, twin = make_env(D), make_env(D)
    env.reset()
    twin.reset()
    got = env.rollout_autoreset(*staged(ref), max_steps=MAX_STEPS, score=make_score(D))
    want = twin.rollout_autoreset(*staged(ref), max_steps=MAX_STEPS)
    assert len(got) == 5 and len(want) == 4
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and (g.cpu().numpy().view(np.uint8) == w.cpu().numpy().view(np.uint8)).all(), name
    assert torch.equal(env.episode_state, twin.episode_state) and torch.equal(env.episode_tally, twin.episode_tally)
    assert torch.equal(env._last[0], twin._last[0]) and int(env.episode_tally[0]) >= MIN_EPISODES
    for f in STATE_FIELDS + STAT_FIELDS:
        assert (env.get_state(f).view(np.uint8) == twin.get_state(f).view(np.uint8)).all(), f
    assert int(got[4].sum()) > 0 and (got[4].cpu().numpy() == ref["out"][4]).all()    # (the score changes no trajectory)
    assert set(ep_launches(env)) == {"ct_rollout_sync_eps<4, 2>"} and set(ep_launches(twin)) == {"ct_rollout_sync_ep<4, 2>"}


# ---- 4. calls continue one another ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pieces", [(37, 64, 49), (1,) * K_LONG], ids=["37+64+49", "150 steps"])
def test_split_calls_equal_one_call(pieces):
    """{age, ret}, the tally and obs_next are carried in place from call to call, and the delivered baseline restarts with
    every launch; a piece of 1 goes through step_autoreset(score=) into a StepOutputs(delivered=), a longer one into the
    caller's rows.  (The one call of 150 is case 1: all three sequences are compared with the same oracle trajectory.)"""
    import torch
    D = 4
    ref = scored_autoreset_reference(D)
    env = make_env(D)
    env.reset()
    tally0 = np.array([3, 1, 1 << 40, -(1 << 33), 7], np.int64)
    env.episode_tally.copy_(torch.from_numpy(tally0))
    dev, dur = staged(ref)
    kinds = (torch.int32, torch.float32, torch.uint8, torch.uint8, torch.int32)
    rows = tuple(torch.empty((K_LONG, N), dtype=t, device="cuda") for t in kinds)
    s = 0
    for n in pieces:
        if n == 1:
            out = step_outputs()
            back = env.step_autoreset({"device": dev[s], "duration": dur[s]}, max_steps=MAX_STEPS, out=out, score=ref["score"])
            assert len(back) == 6 and back[0] is out.obs and back[3] is out.ended and back[4] is env._last[0]
            assert back[5] is out.delivered
            for r, t in zip(rows, back[:4] + (back[5],)):
                r[s].copy_(t)
        else:
            out = tuple(r[s:s + n] for r in rows)
            back = env.rollout_autoreset(dev[s:s + n], dur[s:s + n], max_steps=MAX_STEPS, out=out, score=ref["score"])
            assert len(back) == 5 and all(a is b for a, b in zip(back, out))
        s += n
    assert_outputs(rows, ref["out"], "over calls of %s steps" % (pieces[:3],))
    assert_episodes(env, ref, "after the split calls", tally=False)
    assert (env.episode_tally.cpu().numpy() == tally0 + ref["tally"]).all()
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after the split calls")


@pytest.mark.gpu
def test_step_outputs_without_a_delivered_tensor_are_refused():
    import torch
    from gymwipe_amd import StepOutputs
    D = 4
    env = make_env(D)
    env.reset()
    out = StepOutputs(torch.empty(N, dtype=torch.int32, device="cuda"), torch.empty(N, dtype=torch.float32, device="cuda"),
                      torch.empty(N, dtype=torch.uint8, device="cuda"), ended=torch.empty(N, dtype=torch.uint8, device="cuda"))
    act = {"device": torch.zeros(N, dtype=torch.int32, device="cuda"), "duration": torch.ones(N, dtype=torch.int32, device="cuda")}
    before = launches(env)
    with pytest.raises(ValueError, match="delivered"):
        env.step_autoreset(act, max_steps=MAX_STEPS, out=out, score=case_score(D))
    assert launches(env) == before
    assert len(env.step_autoreset(act, max_steps=MAX_STEPS, out=out)) == 5          # the unscored call is unchanged


# ---- 5. one case per instantiation ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(INSTANTIATIONS))
def test_instantiation_matches_the_oracle(name, monkeypatch):
    dt, mode = INSTANTIATIONS[name]
    D = dt if dt else 11
    for k, v in dict(MODE_SWITCHES[mode], GW_ROLLOUT_STRICT="1").items():
        monkeypatch.setenv(k, v)
    ref = scored_autoreset_reference(D, K_INST)                         # (shared by the three modes of a sender count)
    env = make_env(D)
    env.reset()
    before = launches(env)
    got = env.rollout_autoreset(*staged(ref), max_steps=MAX_STEPS, score=ref["score"])
    assert_outputs(got, ref["out"], "under %s" % name)
    assert_episodes(env, ref, "after %s" % name)
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after %s" % name)
    assert delta(launches(env), before) == {name: 1}, launches(env)     # the target, and no step or reset kernel


# ---- 6. invalid actions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_rejected_action_scores_0_delivers_0_and_is_a_step_of_the_episode():
    """Step 9 of three envs is outside the action space (sender D, duration 99, sender -1): the env is untouched, the row
    repeats what the env acted on, with delivered 0 and reward 0 whatever the weights, and -- being the fifth step of the
    second episode -- it ends that episode by the step limit."""
    import torch
    D = 4
    ref = rejected_reference(D, case_score(D))
    bad, others = ref["bad"], ref["others"]
    g_dev, g_dur = ref["dev"].copy(), ref["dur"].copy()
    g_dev[BAD_STEP, bad[0]] = D
    g_dur[BAD_STEP, bad[1]] = 99
    g_dev[BAD_STEP, bad[2]] = -1
    env = make_env(D)
    env.reset()
    got = [t.cpu().numpy() for t in env.rollout_autoreset(torch.from_numpy(g_dev).cuda(), torch.from_numpy(g_dur).cuda(),
                                                           max_steps=MAX_STEPS, score=case_score(D))]
    assert len(got) == 5
    for name, g, w, w3 in zip(NAMES, got, ref["want"], ref["rows"]):
        assert g.dtype == w.dtype and (g[:, others] == w[:, others]).all(), name
        assert (g[:, bad] == w3).all(), (name, np.argwhere(g[:, bad] != w3)[:3].tolist())
    assert (got[4][BAD_STEP, bad] == 0).all() and (got[1][BAD_STEP, bad] == 0).all() and (got[3][BAD_STEP, bad] == 2).any()
    flags = env.get_state("flags")
    assert np.flatnonzero(flags & FLAG_BADACT).tolist() == bad and env.stats()["bad_actions"] == 3
    nxt = env._last[0].cpu().numpy()
    assert (nxt[others] == ref["acts_big"][others]).all() and (nxt[bad] == ref["acts_on"]).all()
    st = env.episode_state.cpu().numpy()
    assert (st[others] == ref["state_big"][others]).all() and (st[bad] == ref["state"]).all()
    for f in STATE_FIELDS + STAT_FIELDS:
        a = env.get_state(f)
        if f == "flags":
            a = a & ~np.asarray(FLAG_BADACT, a.dtype)
        assert (a[others].view(np.uint8) == ref["big"].get(f)[others].view(np.uint8)).all(), f
        assert (a[bad].view(np.uint8) == ref["small"].get(f).view(np.uint8)).all(), f


# ---- 7. other handles -------------------------------------------------------------------------------------------------------------
K_OTHER = 24


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["per_env_geometry", "rollout_cap_0"])
def test_handles_without_a_fused_form_score_per_step(kind, monkeypatch):
    """(GW_ROLLOUT_CAP is read when the handle is created, so the second handle is a default one without a fused rollout.)"""
    import torch
    from gymwipe_amd import _native as nat
    D = 4
    kw = {"per_env_geometry": {"per_env_geometry": True}, "rollout_cap_0": {}}[kind]
    if kind == "rollout_cap_0":
        monkeypatch.setenv("GW_ROLLOUT_CAP", "0")
    env, orc = make_env(D, **kw), new_oracle(D)
    monkeypatch.delenv("GW_ROLLOUT_CAP", raising=False)
    score = case_score(D)
    dev, dur = staged_actions(D, 2 * K_OTHER)
    t_dev, t_dur = torch.from_numpy(dev).cuda(), torch.from_numpy(dur).cuda()
    env.reset()
    orc.reset()
    calls = (lambda: env.rollout_autoreset(t_dev[:4], t_dur[:4], max_steps=MAX_STEPS, score=score),
             lambda: env.step_autoreset({"device": t_dev[0], "duration": t_dur[0]}, max_steps=MAX_STEPS, score=score))

    def refused_under_strict():
        bytes_was, was = env.state_bytes(), launches(env)
        monkeypatch.setenv("GW_ROLLOUT_STRICT", "1")
        for call in calls:
            with pytest.raises(nat.NativeError) as exc:
                call()
            assert exc.value.code == nat.EUNSUPPORTED
        monkeypatch.delenv("GW_ROLLOUT_STRICT")
        assert env.state_bytes() == bytes_was and launches(env) == was   # before anything was launched or allocated

    refused_under_strict()
    state, tally, packets = np.zeros((N, 2), np.int32), 0, 0
    bytes0, before = env.state_bytes(), launches(env)
    for call in range(2):
        rows = slice(call * K_OTHER, (call + 1) * K_OTHER)
        got = env.rollout_autoreset(t_dev[rows], t_dur[rows], max_steps=MAX_STEPS, score=score)
        want, plain, acts_on, t = oracle_scored_autoreset_steps(orc, dev[rows], dur[rows], score, state, MAX_STEPS, True)
        tally, packets = tally + t, packets + int(want[4].sum())
        assert_outputs(got, want, "in call %d (%s)" % (call, kind))
        assert (want[1] != plain).any()
        assert env.state_bytes() == bytes0 + 4 * N                      # the delivered counters' row: once, with the first call
    if tally[0] < MIN_EPISODES or packets == 0:
        raise RuntimeError("%d episodes ended, %d packets" % (tally[0], packets))
    assert_episodes(env, {"obs_next": acts_on, "state": state, "tally": tally}, "after two calls (%s)" % kind)
    if kind == "per_env_geometry":                                      # (received power as tests/test_rollout_policy.py bounds it)
        fields = tuple(f for f in STATE_FIELDS + STAT_FIELDS if f != "rx_power")
        a, b = env.get_state("rx_power"), orc.get("rx_power")
        assert np.max(np.abs(a - b) / b) < 1e-5
    else:
        fields = STATE_FIELDS + STAT_FIELDS
    assert_state_equal(env, orc, fields, where="after two calls (%s)" % kind)
    ran = delta(launches(env), before)
    assert not [k for k in launches(env) if k.startswith("ct_rollout")], ran
    assert sum(v for k, v in ran.items() if k.startswith("ct_step")) == 2 * K_OTHER and len(ran) == 1, ran
    refused_under_strict()


@pytest.mark.gpu
@pytest.mark.parametrize("strict", [False, True])
def test_an_explicit_queue_handle_is_refused(strict, monkeypatch):
    """The parent accepts such a handle; it keeps no delivered counter per env, so the scored call cannot."""
    import torch
    from gymwipe_amd import _native as nat
    D = 3
    env = make_env(D, explicit_queue=True)
    env.reset()
    dev, dur = (torch.from_numpy(a).cuda() for a in staged_actions(D, 4))
    if strict:
        monkeypatch.setenv("GW_ROLLOUT_STRICT", "1")
    bytes0, before = env.state_bytes(), launches(env)
    for call in (lambda: env.rollout_autoreset(dev, dur, max_steps=MAX_STEPS, score=case_score(D)),
                 lambda: env.step_autoreset({"device": dev[0], "duration": dur[0]}, max_steps=MAX_STEPS, score=case_score(D))):
        with pytest.raises(nat.NativeError) as exc:
            call()
        assert exc.value.code == nat.EUNSUPPORTED
    assert launches(env) == before and env.state_bytes() == bytes0
    if not strict:
        assert len(env.rollout_autoreset(dev, dur, max_steps=MAX_STEPS)) == 4        # the parent still takes it


# ---- 8. hipGraph ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graph_capture_of_reset_and_eight_scored_autoreset_steps():
    """A linear capture on a side stream (as tests/test_rollout_autoreset.py captures the parent): one replay equals eager
    stepping on a twin, the packets per step included, and with max_steps = 3 the eight steps end two episodes per env."""
    import torch
    D, G = 4, 8
    score = case_score(D)
    dev, dur = (torch.from_numpy(a).cuda() for a in staged_actions(D, G))
    acts = [{"device": dev[j].clone(), "duration": dur[j].clone()} for j in range(G)]
    g, e = make_env(D), make_env(D)
    outs_g, outs_e = [step_outputs() for _ in range(G)], [step_outputs() for _ in range(G)]
    for env, outs in ((g, outs_g), (e, outs_e)):                        # eager: fills the identity cache, allocates the tensors
        env.reset()
        for j in range(G):
            env.step_autoreset(acts[j], max_steps=3, out=outs[j], score=score)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        g.reset()
        for j in range(G):
            g.step_autoreset(acts[j], max_steps=3, out=outs_g[j], score=score)
    for o in outs_g:
        o.ended.fill_(9)
        o.delivered.fill_(-1)
    graph.replay()
    e.reset()
    for j in range(G):
        e.step_autoreset(acts[j], max_steps=3, out=outs_e[j], score=score)
    torch.cuda.synchronize()
    packets = 0
    for j in range(G):
        for x, y in zip(outs_g[j]._as_tuple + (outs_g[j].ended, outs_g[j].delivered),
                        outs_e[j]._as_tuple + (outs_e[j].ended, outs_e[j].delivered)):
            assert torch.equal(x, y), j
        assert int(outs_g[j].ended.sum()) == (2 * N if j % 3 == 2 else 0)
        assert int(outs_g[j].delivered.min()) >= 0
        packets += int(outs_g[j].delivered.sum())
    assert packets > 0
    assert torch.equal(g.episode_state, e.episode_state) and torch.equal(g._last[0], e._last[0])
    assert (g.episode_state[:, 0] == G % 3).all()
    for f in STATE_FIELDS + STAT_FIELDS:
        assert (g.get_state(f).view(np.uint8) == e.get_state(f).view(np.uint8)).all(), f
    assert launches(g) == {"ct_rollout_sync_eps<4, 2>": G, "ct_rollout_sync_eps<4, 1>": G}, launches(g)


# ---- 9. the agent ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_dqn_fit_with_a_score_remembers_the_packets_as_the_reward():
    import torch
    from gymwipe_amd.actions import make_score
    from gymwipe_amd.agents import DqnCounterTrafficAgent
    n, steps, E = 256, 48, 8
    env = make_env(4, n=n)
    agent = DqnCounterTrafficAgent(env, seed=5)
    agent.fit(steps, episode_steps=E, score=make_score(4, reward=0, delivered=1))
    assert agent.m_len == steps * n and agent.steps == steps
    rew = agent.m_rew[:steps * n]
    assert bool((rew >= 0).all()) and bool((rew == rew.round()).all())
    total = int(env.get_state("n_delivered").astype(np.int64).sum())    # fit() begins with a reset of fresh envs: the growth
    assert int(rew.to(torch.float64).sum()) == total > 0
    stats = env.episode_stats()
    assert stats["episodes"] == n * (steps // E) > 0 and stats["by_done"] == 0 and stats["mean_length"] == E
    assert stats["mean_return"] == total / stats["episodes"]            # packets per episode (every episode has ended)
    m_obs, m_next = agent.m_obs[:steps * n].view(steps, n), agent.m_next[:steps * n].view(steps, n)
    assert int(agent.m_done.sum()) == 0
    over = torch.zeros(steps - 1, dtype=torch.bool, device=m_obs.device)
    over[E - 1::E] = True
    assert torch.equal(m_obs[0], torch.full_like(m_obs[0], agent.center))
    assert torch.equal(m_obs[1:][over], torch.full_like(m_obs[1:][over], agent.center))   # acted on the reset's observation
    assert torch.equal(m_obs[1:][~over], m_next[:-1][~over])
    assert bool((m_next[:-1][over] != agent.center).any())              # m_next kept the terminal observations
    assert launches(env) == {"ct_rollout_sync_eps<4, 2>": steps}, launches(env)
