"""
gw_rollout_controller / gw_rollout_controller_population on the GPU: the scored closed loops under a finite-state controller
(ct_rollout_fsc<DT, MODE>, ct_rollout_fsc_pop<DT, MODE>) -- the env's node picks the rows the action is drawn from, and moves
behind every step on the new observation class and on whether the step delivered enough.

Every expected value comes from the oracle alone (oracle_controller_steps() in tests/test_rollout_controller_cpu.py).  All
comparisons are exact, the state included (STATE_FIELDS + STAT_FIELDS).  An expected trajectory must exercise what it is for:
controller_reference() raises, instead of letting a test pass, unless every node was visited, both values of the delivered bit
occurred, at least two observation classes drove a transition, at least MIN_EPISODES episodes ended and the rows differ from
the one-node run -- so a kernel that ignores `next`, `need` or the reset to node 0 must fail.  Shapes are the smallest that can
go wrong: N = 160 is three blocks, the last one half full; STEPS = 70 is launches of 64 + 6 steps.
tests/test_rollout_controller_cpu.py checks on the CPU that the two INSTANTIATIONS sets are exactly the library's.
"""
import functools

import numpy as np
import pytest

from test_kernel_variants import MODE_SWITCHES, SFX_DTS, launches
from test_rollout_episodes import MAX_STEPS, MIN_EPISODES
from test_rollout_policy import CENTER, K_INST, MAX_DURATION, SEED, delta, make_env, oracle_prep
from test_rollout_controller_cpu import NAMES, oracle_controller_steps
from test_rollout_scored import case_score, prepared_env
from test_rollout_scored_cpu import new_oracle
from util import assert_state_equal, STATE_FIELDS, STAT_FIELDS

INSTANTIATIONS = {"ct_rollout_fsc<%d, %d>" % (dt, mode): (dt, mode) for dt in SFX_DTS + (0,) for mode in (2, 1, 0)}
POP_INSTANTIATIONS = {"ct_rollout_fsc_pop<%d, %d>" % (dt, mode): (dt, mode) for dt in SFX_DTS + (0,) for mode in (2, 1, 0)}
N, STEPS = 160, 70                      # three blocks, the last half full; launches of 64 + 6 steps
DS = (2, 4, 16, 9)                      # 9: no kernel of its own (DT == 0)
POPS = ((3, 128), (4, 64))              # a controller spans two blocks; one block per controller
S_CASE = 3


def case_controller(D, S=S_CASE, salt=0):
    """S nodes with Dirichlet(0.3) rows of their own per (node, class), `next` drawn uniformly with every node reachable from
    its predecessor through some entry, thresholds of 1 .. 3 packets (a step delivers 0 .. 9)."""
    from gymwipe_amd.actions import make_controller, policy_cdf
    A = D * MAX_DURATION
    rng = np.random.default_rng(100000 * salt + 1000 * SEED + 10 * S + D)
    p = rng.dirichlet(np.full(A, 0.3), size=(S, 3))
    nxt = rng.integers(0, S, size=(S, 3, 2))
    for n in range(S):
        nxt[n, 1, n % 2] = (n + 1) % S                          # the centre class is the common one
    need = 1 + (np.arange(S) + salt) % 3
    return make_controller(D, policy_cdf(p), nxt, need)


def one_node(controller):
    """Node 0 alone: what the run would be without the memory."""
    cdf, nxt, need = controller
    return cdf[:1].copy(), np.zeros((1, 3, 2), np.uint8), need[:1].copy()


def fsc_launches(env):
    return {k: v for k, v in launches(env).items() if k.startswith("ct_rollout_fsc")}


def fused_name(family, D):
    return "%s<%d, 2>" % (family, D if D in SFX_DTS else 0)


def run_reference(D, controller, n, steps, cols):
    score = case_score(D)
    orc = new_oracle(D, n)
    obs_prev = oracle_prep(orc, D, cols)
    state, node = np.zeros((n, 2), np.int32), np.zeros(n, np.uint8)
    out, plain, obs_next, tally = oracle_controller_steps(orc, controller, score, steps, SEED, 0, 0, obs_prev, state, node,
                                                          MAX_STEPS, True)
    return {"controller": controller, "score": score, "out": out, "obs_next": obs_next, "state": state, "node": node,
            "tally": tally, "orc": orc, "n": n}


def gated(ref, plain_run, who):
    """Raises unless the trajectory exercises the controller."""
    cdf, nxt, need = ref["controller"]
    S = cdf.shape[0]
    out = ref["out"]
    moved = out[5] == 0                                          # the steps whose transition read the tables
    at, dl = out[7].astype(np.int64), out[6].astype(np.int64)
    if set(np.unique(at).tolist()) != set(range(S)):
        raise RuntimeError("%s: nodes visited %s, not all of %d" % (who, np.unique(at).tolist(), S))
    bits = dl[moved] >= need.astype(np.int64)[at[moved]]
    if bits.all() or not bits.any():
        raise RuntimeError("%s: the delivered bit took one value only" % who)
    classes = np.unique(np.sign(out[2].astype(np.int64)[moved] - CENTER))
    if len(classes) < 2:
        raise RuntimeError("%s: one observation class drove every transition" % who)
    if ref["tally"][0] < MIN_EPISODES:
        raise RuntimeError("%s: %d episodes ended, fewer than %d" % (who, ref["tally"][0], MIN_EPISODES))
    if not (at[1:][out[5][:-1] != 0] == 0).all() or not (at[1:][out[5][:-1] == 0] != 0).any():
        raise RuntimeError("%s: the reset to node 0 is not visible in the rows" % who)
    if all((a == b).all() for a, b in zip(out[:7], plain_run["out"][:7])):
        raise RuntimeError("%s: the rows are those of the one-node run" % who)


@functools.lru_cache(maxsize=None)
def controller_reference(D, n=N, steps=STEPS, salt=0):
    """The oracle's trajectory of `steps` controller steps after the PREP ordinary ones, computed once and read only."""
    ctl = case_controller(D, salt=salt)
    cols = np.arange(n) % 200
    ref = run_reference(D, ctl, n, steps, cols)
    gated(ref, run_reference(D, one_node(ctl), n, steps, cols), "controller_reference(%d, %d, %d, %d)" % (D, n, steps, salt))
    for a in ref["out"] + (ref["obs_next"], ref["state"], ref["node"], ref["tally"], ref["score"]) + tuple(ctl):
        a.setflags(write=False)
    return ref


def assert_outputs(got, want, where, cols=slice(None)):
    assert len(got) == len(want) == 8
    for name, g, w in zip(NAMES, got, want):
        g = g.cpu().numpy()
        w = np.ascontiguousarray(w[:, cols])
        assert g.dtype == w.dtype and g.shape == w.shape, (name, where)
        assert (g.view(np.uint8) == w.view(np.uint8)).all(), \
            "%s differs %s, first at (step, env) %s" % (name, where, np.argwhere(g != w)[:3].tolist())


def assert_episodes(env, ref, where, cols=slice(None), tally=None):
    assert (env._last[0].cpu().numpy() == ref["obs_next"][cols]).all(), "obs_next differs " + where
    assert (env.episode_state.cpu().numpy() == ref["state"][cols]).all(), "{age, ret} differs " + where
    assert (env.controller_node.cpu().numpy() == ref["node"][cols]).all(), "node_dev differs " + where
    if tally is not None:
        assert env.episode_tally.cpu().numpy().tolist() == np.asarray(tally).tolist(), "the call-wide tally differs " + where


# ---- 1. the records form ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("D", DS)
def test_records_form_matches_the_oracle(D):
    ref = controller_reference(D)
    env = prepared_env(D, N)
    got = env.rollout_controller(ref["controller"], STEPS, SEED, max_steps=MAX_STEPS, score=ref["score"])
    assert_outputs(got, ref["out"], "in one call of %d steps" % STEPS)
    assert_episodes(env, ref, "after the call", tally=ref["tally"])
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after the call")
    assert fsc_launches(env) == {fused_name("ct_rollout_fsc", D): 2}, launches(env)      # 64 + 6 steps
    assert not [k for k in launches(env) if "_eps<" in k or "_ep<" in k]
    env.check()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(INSTANTIATIONS))
def test_instantiation_matches_the_oracle(name, monkeypatch):
    dt, mode = INSTANTIATIONS[name]
    D = dt if dt else 11
    for k, v in dict(MODE_SWITCHES[mode], GW_ROLLOUT_STRICT="1").items():
        monkeypatch.setenv(k, v)
    ref = controller_reference(D, N, K_INST)                            # (shared by the three modes of a sender count)
    env = prepared_env(D, N)
    before = launches(env)
    got = env.rollout_controller(ref["controller"], K_INST, SEED, max_steps=MAX_STEPS, score=ref["score"])
    assert_outputs(got, ref["out"], "under %s" % name)
    assert_episodes(env, ref, "after %s" % name, tally=ref["tally"])
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after %s" % name)
    assert delta(launches(env), before) == {name: 1}, launches(env)     # the target, and no step or reset kernel


@pytest.mark.gpu
def test_records_form_in_split_calls_and_into_the_callers_rows():
    import torch
    D = 4
    ref = controller_reference(D)
    env = prepared_env(D, N)
    kinds = (torch.int32, torch.int32, torch.int32, torch.float32, torch.uint8, torch.uint8, torch.int32, torch.uint8)
    rows = tuple(torch.empty((STEPS, N), dtype=t, device=env.device) for t in kinds)
    s = 0
    for n in (1, 33, 36):
        out = tuple(r[s:s + n] for r in rows)
        back = env.rollout_controller(ref["controller"], n, SEED, max_steps=MAX_STEPS, step0=s, out=out, score=ref["score"])
        assert len(back) == 8 and all(a is b for a, b in zip(back, out))
        s += n
    assert_outputs(rows, ref["out"], "over calls of 1 + 33 + 36 steps")
    assert_episodes(env, ref, "after the split calls", tally=ref["tally"])
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after the split calls")


@pytest.mark.gpu
def test_one_node_is_the_scored_parent_bit_for_bit():
    D = 4
    ref = controller_reference(D)
    ctl = one_node(ref["controller"])
    env, twin = prepared_env(D, N), prepared_env(D, N)
    env.controller_node.fill_(9)                                        # any stored node is node 0 of a one-node controller
    got = env.rollout_controller(ctl, STEPS, SEED, max_steps=MAX_STEPS, score=ref["score"])
    want = twin.rollout_episodes(ctl[0][0], STEPS, SEED, max_steps=MAX_STEPS, score=ref["score"])
    assert len(got) == 8 and len(want) == 7
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and (g.cpu().numpy().view(np.uint8) == w.cpu().numpy().view(np.uint8)).all(), name
    assert int(got[7].max()) == 0 and int(env.controller_node.max()) == 0
    assert (env.episode_state == twin.episode_state).all() and (env.episode_tally == twin.episode_tally).all()
    assert (env._last[0] == twin._last[0]).all() and int(env.episode_tally[0]) >= MIN_EPISODES
    for f in STATE_FIELDS + STAT_FIELDS:
        assert (env.get_state(f).view(np.uint8) == twin.get_state(f).view(np.uint8)).all(), f
    assert fsc_launches(env) and not fsc_launches(twin)


@pytest.mark.gpu
def test_a_slice_handle_with_env_id0_gives_the_big_handles_columns():
    D, lo, n = 4, 64, 96                                                # a block and a half, from the second block on
    ref = controller_reference(D)
    cols = slice(lo, lo + n)
    env = prepared_env(D, n, lo=lo)
    got = env.rollout_controller(ref["controller"], STEPS, SEED, max_steps=MAX_STEPS, env_id0=lo, score=ref["score"])
    assert_outputs(got, ref["out"], "in the slice at %d" % lo, cols)
    assert_episodes(env, ref, "in the slice at %d" % lo, cols)
    for f in STATE_FIELDS + STAT_FIELDS:
        assert (env.get_state(f).view(np.uint8) == ref["orc"].get(f)[cols].view(np.uint8)).all(), f


@pytest.mark.gpu
def test_hostile_bytes_mean_what_the_restatement_says():
    """Nothing of the controller is validated: `next` entries and stored nodes of S and above clamp to S - 1, and need 0 and
    255 are the bit always and never set."""
    D, n, steps = 4, N, 40
    cdf, _, _ = case_controller(D)
    rng = np.random.default_rng(77)
    nxt = rng.integers(S_CASE, 256, size=(S_CASE, 3, 2)).astype(np.uint8)      # every entry clamps to node 2, but:
    nxt[0, :, 1] = 1                                                    # need 0: node 0 always takes the set bit's entry
    nxt[2, :2, 0] = 0                                                   # need 2: node 2 goes back where the step delivered less
    ctl = (cdf, nxt, np.array([0, 255, 2], np.uint8))                   # need 255: node 1 always takes the clear bit's entry
    score = case_score(D)
    orc = new_oracle(D, n)
    obs_prev = oracle_prep(orc, D, np.arange(n) % 200)
    state, node = np.zeros((n, 2), np.int32), (np.arange(n) * 37 % 256).astype(np.uint8)
    env = prepared_env(D, n)
    env.controller_node.copy_(__import__("torch").from_numpy(node.copy()))
    out, _, obs_next, tally = oracle_controller_steps(orc, ctl, score, steps, SEED, 0, 0, obs_prev, state, node, MAX_STEPS, True)
    assert (nxt >= S_CASE).any() and set(np.unique(out[7]).tolist()) == set(range(S_CASE))
    got = env.rollout_controller(ctl, steps, SEED, max_steps=MAX_STEPS, score=score)
    ref = {"obs_next": obs_next, "state": state, "node": node}
    assert_outputs(got, out, "under hostile bytes")
    assert_episodes(env, ref, "under hostile bytes", tally=tally)
    assert_state_equal(env, orc, STATE_FIELDS + STAT_FIELDS, where="under hostile bytes")
    env.check()


# ---- 2. the population ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def population_reference(D, P, M, steps=STEPS):
    """Controller p's envs are columns [p M, (p + 1) M) of the handle: the records-form reference of that controller on those
    columns, with their stream ids."""
    refs = []
    for p in range(P):
        ctl = case_controller(D, salt=p + 1)
        cols = np.arange(p * M, (p + 1) * M) % 200
        score = case_score(D)
        orc = new_oracle(D, M)
        obs_prev = oracle_prep(orc, D, cols)
        state, node = np.zeros((M, 2), np.int32), np.zeros(M, np.uint8)
        out, _, obs_next, tally = oracle_controller_steps(orc, ctl, score, steps, SEED, 0, p * M, obs_prev, state, node, MAX_STEPS,
                                                          True)
        ref = {"controller": ctl, "score": score, "out": out, "obs_next": obs_next, "state": state, "node": node, "tally": tally,
               "orc": orc, "n": M}
        one = run_slice_one_node(D, ctl, cols, p * M, M, steps)
        gated(ref, one, "population_reference(%d, %d, %d)[%d]" % (D, P, M, p))
        refs.append(ref)
    tally = np.stack([r["tally"] for r in refs])
    if len({tuple(row) for row in tally.tolist()}) != P:
        raise RuntimeError("population_reference(%d, %d, %d): two controllers have the same tally row" % (D, P, M))
    return refs, tally


def run_slice_one_node(D, ctl, cols, lo, M, steps):
    orc = new_oracle(D, M)
    obs_prev = oracle_prep(orc, D, cols)
    out, _, _, _ = oracle_controller_steps(orc, one_node(ctl), case_score(D), steps, SEED, 0, lo, obs_prev,
                                           np.zeros((M, 2), np.int32), np.zeros(M, np.uint8), MAX_STEPS, True)
    return {"out": out}


@pytest.mark.gpu
@pytest.mark.parametrize("D,P,M", [(4,) + POPS[0], (4,) + POPS[1], (9,) + POPS[0]])
def test_population_matches_the_records_form_reference_of_each_controller(D, P, M):
    from gymwipe_amd.actions import make_controller_population
    refs, tally_want = population_reference(D, P, M)
    env = prepared_env(D, P * M)
    pop = make_controller_population([r["controller"] for r in refs])
    tally = env.rollout_controller_population(pop, STEPS, SEED, max_steps=MAX_STEPS, score=refs[0]["score"])
    assert tally.cpu().numpy().tolist() == tally_want.tolist(), "the per-controller tally differs"
    assert env.episode_tally.cpu().numpy().tolist() == tally_want.sum(axis=0).tolist(), "the call-wide tally is not the column sums"
    assert len({tuple(row) for row in tally.cpu().numpy().tolist()}) == P
    node, state, nxt = env.controller_node.cpu().numpy(), env.episode_state.cpu().numpy(), env._last[0].cpu().numpy()
    for p, r in enumerate(refs):
        s = slice(p * M, (p + 1) * M)
        assert (node[s] == r["node"]).all(), "node_dev differs for controller %d" % p
        assert (state[s] == r["state"]).all() and (nxt[s] == r["obs_next"]).all(), p
        for f in STATE_FIELDS + STAT_FIELDS:
            assert (env.get_state(f)[s].view(np.uint8) == r["orc"].get(f).view(np.uint8)).all(), (f, p)
    assert fsc_launches(env) == {fused_name("ct_rollout_fsc_pop", D): 2}, launches(env)
    env.check()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(POP_INSTANTIATIONS))
def test_population_instantiation_matches_the_records_form_reference(name, monkeypatch):
    from gymwipe_amd.actions import make_controller_population
    dt, mode = POP_INSTANTIATIONS[name]
    D = dt if dt else 11
    P, M = 2, 64
    for k, v in dict(MODE_SWITCHES[mode], GW_ROLLOUT_STRICT="1").items():
        monkeypatch.setenv(k, v)
    refs, tally_want = population_reference(D, P, M, K_INST)             # (shared by the three modes of a sender count)
    env = prepared_env(D, P * M)
    before = launches(env)
    tally = env.rollout_controller_population(make_controller_population([r["controller"] for r in refs]), K_INST, SEED,
                                              max_steps=MAX_STEPS, score=refs[0]["score"])
    assert tally.cpu().numpy().tolist() == tally_want.tolist(), "the per-controller tally differs under %s" % name
    node = env.controller_node.cpu().numpy()
    for p, r in enumerate(refs):
        s = slice(p * M, (p + 1) * M)
        assert (node[s] == r["node"]).all(), (name, p)
        for f in STATE_FIELDS + STAT_FIELDS:
            assert (env.get_state(f)[s].view(np.uint8) == r["orc"].get(f).view(np.uint8)).all(), (f, p)
    assert delta(launches(env), before) == {name: 1}, launches(env)


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------------
def refused(env, call):
    import torch
    from gymwipe_amd import _native as nat
    node0 = env.controller_node.clone()
    before, bytes0 = launches(env), env.state_bytes()
    with pytest.raises(nat.NativeError) as exc:
        call()
    torch.cuda.synchronize()
    assert exc.value.code == nat.EUNSUPPORTED, exc.value
    assert launches(env) == before and env.state_bytes() == bytes0 and (env.controller_node == node0).all()


@pytest.mark.gpu
def test_refusals(monkeypatch):
    from gymwipe_amd.actions import make_controller, make_controller_population, policy_cdf
    D = 4
    ctl = case_controller(D)
    env = prepared_env(D, 192)
    env.controller_node.fill_(2)
    # M = 96 is no multiple of 64
    refused(env, lambda: env.rollout_controller_population(make_controller_population([ctl, case_controller(D, salt=1)]), 4, SEED,
                                                           max_steps=MAX_STEPS))
    # GW_ROLLOUT_POLICY_UNFUSED: there is no per-step form to fall back to
    monkeypatch.setenv("GW_ROLLOUT_POLICY_UNFUSED", "1")
    refused(env, lambda: env.rollout_controller(ctl, 4, SEED, max_steps=MAX_STEPS))
    refused(env, lambda: env.rollout_controller_population(make_controller_population([ctl] * 3), 4, SEED, max_steps=MAX_STEPS))
    monkeypatch.delenv("GW_ROLLOUT_POLICY_UNFUSED")
    # D = 32 with S = 16: 3 * 16 * 640 words are more than a block's LDS
    big = prepared_env(32, 64)
    A = 32 * MAX_DURATION
    wide = make_controller(32, policy_cdf(np.full((16, 3, A), 1.0 / A)), np.zeros((16, 3, 2), np.uint8), np.zeros(16, np.uint8))
    refused(big, lambda: big.rollout_controller(wide, 4, SEED, max_steps=MAX_STEPS))
    refused(big, lambda: big.rollout_controller_population(make_controller_population([wide]), 4, SEED, max_steps=MAX_STEPS))
    small = tuple(a[:1] for a in wide)                                  # ... and one node of it fits
    assert len(big.rollout_controller(small, 4, SEED, max_steps=MAX_STEPS)) == 8
    # an explicit-queue handle and a live-PHY handle have no fused rollout
    for kw in ({"explicit_queue": True}, {"per_env_geometry": True}):
        other = make_env(D, n=64, **kw)
        other.reset()
        refused(other, lambda: other.rollout_controller(ctl, 4, SEED, max_steps=MAX_STEPS))
        refused(other, lambda: other.rollout_controller_population(make_controller_population([ctl]), 4, SEED, max_steps=MAX_STEPS))
    # and the handle that was refused runs the call afterwards
    out = env.rollout_controller(ctl, 4, SEED, max_steps=MAX_STEPS)
    assert int(out[7][0].min()) == 2 and fsc_launches(env) == {"ct_rollout_fsc<4, 2>": 1}


# ---- 4. the agent -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_controller_search_agent_equals_the_oracle_backed_run():
    from gymwipe_amd.agents import ControllerSearchAgent
    from test_rollout_controller_cpu import AGENT, oracle_agent
    want = oracle_agent()
    want.fit(AGENT["generations"])
    env = make_env(AGENT["D"], n=AGENT["P"] * AGENT["M"])
    agent = ControllerSearchAgent(env, AGENT["P"], AGENT["steps"], AGENT["episode_steps"], seed=AGENT["seed"])
    agent.fit(AGENT["generations"])
    for x, y in zip(agent.history, want.history):
        assert x["mean"] == y["mean"] and x["best"] == y["best"] and (x["fitness"] == y["fitness"]).all(), x["generation"]
    assert (agent.mu == want.mu).all() and (agent.sigma == want.sigma).all()
    assert {k for k in launches(env) if k.startswith("ct_rollout_fsc")} == {"ct_rollout_fsc_pop<4, 2>"}
    env.check()
