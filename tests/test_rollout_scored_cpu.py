"""
gw_rollout_episodes_scored / gw_rollout_population_scored, the part that needs no GPU: the oracle composition the GPU file
compares against (oracle_scored_steps(), oracle_scored_population_steps(): CtOracle.step, the difference of
CtOracle.get("n_delivered") across the step, actions.policy_sample_numpy / _population_numpy, actions.score_numpy,
actions.episodes_numpy fed the score, CtOracle.reset(mask)), the fact that motivates the score (an episode's return under the
built-in reward is 0 or -payload_value whatever the policy does, and the policy that assigns nothing attains 0), the helpers
actions.make_score / score_numpy, argument validation of the two entry points, the catalogue of the two fused families, and
agents.PopulationSearchAgent ranking by delivered packets on the oracle alone.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from gymwipe_amd import actions

CENTER, MAX_DURATION, PAYLOAD_VALUE = 65536, 20, 2      # counter_traffic.py:35, envs/core.py:25, counter_traffic.py:57
NAMES = ("device", "duration", "obs", "reward", "done", "ended", "delivered")
DTYPES = (np.int32, np.int32, np.int32, np.float32, np.uint8, np.uint8, np.int32)


def delivered_now(orc):
    return orc.get("n_delivered").astype(np.int64).copy()


def oracle_scored_steps(orc, cdf, score, steps, seed, step0, env_id0, obs_prev, state, max_steps, on_done, center=CENTER):
    """The oracle under the policy with episodes scored by ``score``: the seven [steps][n] outputs (``reward`` holds the
    score), the built-in reward [steps][n] beside them, the observation each env acts on next and the episode tally; ``state``
    ({age, ret}, int32[n][2]) is updated in place."""
    n = orc.n
    out = [np.empty((steps, n), t) for t in DTYPES]
    plain = np.empty((steps, n), np.float32)
    tally = np.zeros(actions.EP_COLS, np.int64)
    acts_on = np.asarray(obs_prev, np.int32).copy()
    for k in range(steps):
        d, u = actions.policy_sample_numpy(seed, env_id0, env_id0 + n, step0 + k, cdf, acts_on, center, MAX_DURATION)
        before = delivered_now(orc)
        obs, r, dn = orc.step(d, u)
        dl = (delivered_now(orc) - before).astype(np.int32)
        sc = actions.score_numpy(score, r, d, dl)
        ended, t = actions.episodes_numpy(state, sc, dn, max_steps, on_done)
        tally += t
        if ended.any():
            orc.reset((ended != 0).astype(np.uint8))
        for a, v in zip(out, (d, u, obs, sc.astype(np.float32), dn, ended, dl)):
            a[k] = v
        plain[k] = r
        acts_on = np.where(ended != 0, center, obs).astype(np.int32)
    return tuple(out), plain, acts_on, tally


def oracle_scored_population_steps(orc, cdfs, M, score, steps, seed, step0, env_id0, obs_prev, state, max_steps, on_done,
                                   center=CENTER):
    """The oracle under a population of policies with episodes scored by ``score``: env i runs table ``i // M``.  Returns the
    observation each env acts on next, the ``[P][EP_COLS]`` tally, and the packets each policy's envs delivered (int64[P]);
    ``state`` is updated in place."""
    n, P = orc.n, len(cdfs)
    assert n == P * M
    tally = np.zeros((P, actions.EP_COLS), np.int64)
    packets = np.zeros(P, np.int64)
    acts_on = np.asarray(obs_prev, np.int32).copy()
    for k in range(steps):
        d, u = actions.policy_sample_population_numpy(seed, env_id0, env_id0 + n, step0 + k, cdfs, M, acts_on, center, MAX_DURATION)
        before = delivered_now(orc)
        obs, r, dn = orc.step(d, u)
        dl = (delivered_now(orc) - before).astype(np.int32)
        sc = actions.score_numpy(score, r, d, dl)
        ended = np.empty(n, np.uint8)
        for p in range(P):
            s = slice(p * M, (p + 1) * M)
            ended[s], t = actions.episodes_numpy(state[s], sc[s], dn[s], max_steps, on_done)      # (state[s]: a view)
            tally[p] += t
            packets[p] += dl[s].sum()
        if ended.any():
            orc.reset((ended != 0).astype(np.uint8))
        acts_on = np.where(ended != 0, center, obs).astype(np.int32)
    return acts_on, tally, packets


def fixed_policy(D, sender, duration):
    """The table that always assigns ``sender`` for ``duration``, whatever it sees."""
    p = np.zeros((3, D * MAX_DURATION))
    p[:, sender * MAX_DURATION + duration] = 1.0
    return actions.policy_cdf(p)


def new_oracle(D, n, **cfg):
    """``cfg``: default_config's layout arguments (positions, rrm_pos, start_time, ...); none is the default layout."""
    from oracle.ct_oracle import CtOracle, default_config
    return CtOracle(n, D, config=default_config(D, **cfg), nthreads=4)


# ---- the oracle composition -----------------------------------------------------------------------------------------------------
def test_oracle_composition_scores_what_the_steps_delivered():
    """The neutral score is the unscored composition (tests/test_rollout_episodes.py's); a score over packets adds exactly
    w[d] * delivered per step, and the per-step packets sum to what the oracle's counter gained."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_rollout_episodes import oracle_episode_steps
    D, n, steps = 4, 64, 24
    rng = np.random.default_rng(3)
    cdf = actions.policy_cdf(rng.dirichlet(np.full(D * MAX_DURATION, 0.3), size=3))
    runs = []
    for score in (None, actions.make_score(D), actions.make_score(D, reward=3, delivered=[5, -7, 11, 13])):
        orc = new_oracle(D, n)
        obs, state = orc.reset(), np.zeros((n, 2), np.int32)
        if score is None:
            out, nxt, tally = oracle_episode_steps(orc, cdf, steps, 5, 0, 0, obs, state, 5, True)
            runs.append((out, None, nxt, tally, state, orc))
        else:
            out, plain, nxt, tally = oracle_scored_steps(orc, cdf, score, steps, 5, 0, 0, obs, state, 5, True)
            runs.append((out, plain, nxt, tally, state, orc))
    base, neutral, weighted = runs
    for a, b in zip(base[0], neutral[0][:6]):
        assert a.dtype == b.dtype and (a == b).all()
    assert (neutral[1] == neutral[0][3]).all() and (base[2] == neutral[2]).all() and (base[3] == neutral[3]).all()
    assert (base[4] == neutral[4]).all()
    out, plain = weighted[0], weighted[1]
    w = np.array([5, -7, 11, 13])
    assert (out[3] == 3 * plain + w[out[0]] * out[6]).all() and out[6].sum() > 0 and (out[6] >= 0).all()
    assert (out[6].sum(axis=0) == weighted[5].get("n_delivered")).all()            # (a reset leaves the counter alone)
    for i in (0, 1, 2, 4, 5, 6):                                                     # the score changes no trajectory
        assert (out[i] == neutral[0][i]).all()
    assert weighted[3][0] == base[3][0] and weighted[3][3] != base[3][3]


# ---- the motivating fact ----------------------------------------------------------------------------------------------------------
def test_the_builtin_return_cannot_rank_policies_and_delivered_packets_can():
    D, n, steps, episode = 4, 64, 32, 8
    rng = np.random.default_rng(11)
    tables = {"uniform": actions.policy_cdf(np.full((3, D * MAX_DURATION), 1.0 / (D * MAX_DURATION))),
              "random": actions.policy_cdf(rng.dirichlet(np.full(D * MAX_DURATION, 0.3), size=3)),
              "idle": fixed_policy(D, 2, 0), "s0_d19": fixed_policy(D, 0, 19), "s3_d5": fixed_policy(D, 3, 5)}
    packets = {}
    for name, cdf in tables.items():
        orc = new_oracle(D, n)
        obs, state = orc.reset(), np.zeros((n, 2), np.int32)
        out, plain, _, tally = oracle_scored_steps(orc, cdf, actions.make_score(D, reward=1, delivered=0), steps, 7, 0, 0, obs,
                                                   state, episode, True)
        ret = out[3].reshape(steps // episode, episode, n).sum(axis=1)               # every episode is `episode` steps long
        assert (out[5][episode - 1::episode] == 2).all() and tally[0] == n * steps // episode
        assert set(np.unique(ret).tolist()) <= {0, -PAYLOAD_VALUE}, name
        packets[name] = out[6].reshape(steps // episode, episode, n).sum(axis=1)
        if name == "idle":
            assert (ret == 0).all() and (packets[name] == 0).all()
    assert packets["s0_d19"].mean() > packets["s3_d5"].mean() > 0                  # what the return cannot see
    assert packets["uniform"].max() > packets["uniform"].min()


# ---- the helpers --------------------------------------------------------------------------------------------------------------------
def test_make_score_shapes_and_bounds():
    s = actions.make_score(4)
    assert s.dtype == np.int32 and s.shape == (33,) and s.tolist() == [1] + [0] * 32
    s = actions.make_score(3, reward=-2, delivered=7)
    assert s.tolist() == [-2, 7, 7, 7] + [0] * 29
    s = actions.make_score(2, reward=0, delivered=[actions.SCORE_W_MAX, -actions.SCORE_W_MAX])
    assert s.tolist() == [0, 1024, -1024] + [0] * 30
    assert actions.make_score(32, delivered=np.arange(32)).tolist() == [1] + list(range(32))
    for bad in (dict(num_devices=1), dict(num_devices=33), dict(num_devices=4, reward=1025), dict(num_devices=4, reward=-1025),
                dict(num_devices=4, delivered=1025), dict(num_devices=4, delivered=[1, 2, 3, -1025]),
                dict(num_devices=4, delivered=[1, 2, 3]), dict(num_devices=4, delivered=[[1, 2, 3, 4]]),
                dict(num_devices=4, delivered=0.5), dict(num_devices=4, reward=float("nan"))):
        with pytest.raises(ValueError):
            actions.make_score(**bad)


def test_score_numpy_on_a_hand_computed_row():
    score = actions.make_score(4, reward=3, delivered=[5, -7, 11, 13])
    got = actions.score_numpy(score, np.array([0, -2, 2, 0, -2], np.float32), np.array([0, 1, 2, 3, 3], np.int32),
                              np.array([4, 2, 0, 1, 9], np.int32))
    assert got.dtype == np.int32 and got.tolist() == [20, -6 - 14, 6, 13, -6 + 117]
    assert actions.score_numpy(actions.make_score(4), [-2.0, 2.0], [1, 0], [3, 4]).tolist() == [-2, 2]
    with pytest.raises(ValueError):
        actions.score_numpy(score[:5], [0], [0], [0])


# ---- argument validation ------------------------------------------------------------------------------------------------------------
def test_argument_validation_without_a_gpu(native_lib):
    from gymwipe_amd import _native as nat
    L = native_lib
    one = 16
    fake = C.c_void_p(4096)                                             # never dereferenced: validation comes first
    ep = nat.Episodes(5, 1, one, None)
    pop = nat.Population(3, 128, one, one)
    ok = nat.Score.from_buffer_copy(actions.make_score(4, 1, 3).tobytes())

    def image(**kw):
        w = actions.make_score(4, 1, 3).astype(np.int32)
        for i, v in kw.items():
            w[int(i[1:])] = v
        return nat.Score.from_buffer_copy(w.tobytes())

    def episodes(env=fake, steps=4, ep=ep, score=ok, ptrs=(one,) * 9):
        return L.gw_rollout_episodes_scored(env, steps, one, 1, 0, 0, C.byref(ep) if ep is not None else None,
                                            C.byref(score) if score is not None else None, *ptrs, None)

    def population(env=fake, steps=4, pop=pop, ep=ep, score=ok, prev=one, nxt=one):
        return L.gw_rollout_population_scored(env, steps, C.byref(pop) if pop is not None else None, 1, 0, 0,
                                              C.byref(ep) if ep is not None else None,
                                              C.byref(score) if score is not None else None, prev, nxt, None)

    for call in (episodes, population):
        assert call(env=None) == nat.EINVAL and b"env is NULL" in L.gw_last_error()
        assert call(score=None) == nat.EINVAL and b"NULL" in L.gw_last_error()
        assert call(ep=None) == nat.EINVAL and b"NULL" in L.gw_last_error()
        assert call(steps=-1) == nat.EINVAL and b"steps" in L.gw_last_error()
        for bad in (image(w0=nat.SCORE_W_MAX + 1), image(w0=-nat.SCORE_W_MAX - 1), image(w2=nat.SCORE_W_MAX + 1),
                    image(w32=-nat.SCORE_W_MAX - 1)):
            assert call(score=bad) == nat.EINVAL and b"weight" in L.gw_last_error()
            assert call(score=bad, steps=0) == nat.EINVAL
        assert call(score=image(w0=nat.SCORE_W_MAX, w4=-nat.SCORE_W_MAX), steps=0) == nat.OK
        assert call(steps=0) == nat.OK
    for i in range(9):                                                  # every pointer of the records form, delivered_dev last
        assert episodes(ptrs=(one,) * i + (None,) + (one,) * (8 - i)) == nat.EINVAL and b"NULL" in L.gw_last_error(), i
    assert population(pop=None) == nat.EINVAL and population(prev=None) == nat.EINVAL and population(nxt=None) == nat.EINVAL
    assert population(pop=nat.Population(0, 128, one, one)) == nat.EINVAL


# ---- the catalogue ------------------------------------------------------------------------------------------------------------------
def test_the_scored_instantiations_are_the_librarys(native_lib):
    from gymwipe_amd import _native
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import test_rollout_scored as rs
    from util import kernel_instantiations
    for family, cases in (("ct_rollout_policy_eps", rs.INSTANTIATIONS), ("ct_rollout_pop_eps", rs.POP_INSTANTIATIONS)):
        lib_set = kernel_instantiations(_native.LIB_PATH, family)
        assert len(lib_set) == 30, sorted(lib_set)
        assert sorted(lib_set - set(cases)) == [], "instantiations the catalogue does not name"
        assert sorted(set(cases) - lib_set) == [], "names for instantiations the library does not have"


# ---- the agent on the oracle ----------------------------------------------------------------------------------------------------------
# D = 2, P = 16 policies of M = 32 envs, 40 steps in episodes of 5, 6 generations, score = packets delivered (reward weight 0,
# one per packet), so a generation's mean fitness is its mean packets per episode.  Size and generation count picked here on
# the CPU, on the oracle alone: at P = 8, M = 16 two seeds of 0 .. 5 did not rise within 6 generations (seed 2: 11.09 -> 10.30);
# at this size every seed of 0 .. 4 rises by 1.2 or more (the narrowest, seed 3: 11.130 -> 12.398).  Seed 0, generation by
# generation: 11.058, 10.880, 11.149, 11.937, 13.046, 13.287 -- a gap of 2.2 where one generation to the next moves by 0.2 .. 1.1.
AGENT = dict(D=2, P=16, M=32, steps=40, episode_steps=5, generations=6, seed=0)


def oracle_agent(cfg=None):
    """PopulationSearchAgent ranking by delivered packets, with the oracle standing in for the GPU: one CtOracle for the whole
    run, reset before every generation as the default evaluate resets the env."""
    from gymwipe_amd.agents import PopulationSearchAgent
    cfg = cfg or AGENT
    D, P, M = cfg["D"], cfg["P"], cfg["M"]
    orc = new_oracle(D, P * M)
    score = actions.make_score(D, reward=0, delivered=1)

    def evaluate(cdfs, generation):
        obs = orc.reset()
        state = np.zeros((P * M, 2), np.int32)
        _, tally, _ = oracle_scored_population_steps(orc, cdfs, M, score, cfg["steps"], cfg["seed"], generation * cfg["steps"], 0,
                                                     obs, state, cfg["episode_steps"], True)
        return tally

    return PopulationSearchAgent(None, P, cfg["steps"], cfg["episode_steps"], seed=cfg["seed"], evaluate=evaluate,
                                 nb_actions=D * MAX_DURATION, score=score)


def test_population_search_by_delivered_packets_on_the_oracle():
    one, two = oracle_agent(), oracle_agent()
    h = one.fit(AGENT["generations"])
    two.fit(AGENT["generations"])
    assert one.score is not None and len(h) == AGENT["generations"]
    for x, y in zip(h, two.history):                                    # seeded and deterministic
        assert x["mean"] == y["mean"] and x["best"] == y["best"] and (x["fitness"] == y["fitness"]).all()
    assert (one.mu == two.mu).all() and (one.sigma == two.sigma).all()
    assert all(np.isfinite(e["fitness"]).all() and (e["fitness"] >= 0).all() for e in h)
    assert h[-1]["mean"] > h[0]["mean"], [e["mean"] for e in h]      # mean packets per episode (the figures: above AGENT)
