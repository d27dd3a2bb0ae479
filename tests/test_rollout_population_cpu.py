"""
gw_rollout_population, the part that needs no GPU: the CPU restatement of the per-policy draw
(actions.policy_sample_population_numpy), argument validation of the entry point, the catalogue of the fused family -- the
library's ct_rollout_pop_ep<DT, MODE> instantiations are exactly the cases tests/test_rollout_population.py runs -- and
agents.PopulationSearchAgent driven by the oracle alone (oracle_population_steps(): CtOracle.step with the numpy restatements),
which tests/test_rollout_population.py then expects of the GPU generation for generation.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from gymwipe_amd import actions

CENTER, MAX_DURATION = 65536, 20        # counter_traffic.py:35, envs/core.py:25 (the default configuration)


def oracle_population_steps(orc, cdfs, M, steps, seed, step0, env_id0, obs_prev, state, max_steps, on_done, center=CENTER):
    """The oracle under a population of policies with episodes: env i of ``orc`` runs table ``i // M``.  Returns the
    observation each env acts on next and the ``[P][EP_COLS]`` tally; ``state`` ({age, ret}, int32[n][2]) is updated in place."""
    n, P = orc.n, len(cdfs)
    assert n == P * M
    tally = np.zeros((P, actions.EP_COLS), np.int64)
    acts_on = np.asarray(obs_prev, np.int32).copy()
    for k in range(steps):
        d, u = actions.policy_sample_population_numpy(seed, env_id0, env_id0 + n, step0 + k, cdfs, M, acts_on, center, MAX_DURATION)
        obs, r, dn = orc.step(d, u)
        ended = np.empty(n, np.uint8)
        for p in range(P):
            s = slice(p * M, (p + 1) * M)
            ended[s], t = actions.episodes_numpy(state[s], r[s], dn[s], max_steps, on_done)      # (state[s]: a view)
            tally[p] += t
        if ended.any():
            orc.reset((ended != 0).astype(np.uint8))
        acts_on = np.where(ended != 0, center, obs).astype(np.int32)
    return acts_on, tally


# ---- the numpy restatement --------------------------------------------------------------------------------------------------
def hand_made_tables():
    """Three tables over A = 40 (D = 2): table 0 always draws action 3 from every class, table 1 action 0 / 25 / 39 by class,
    table 2 is uniform."""
    A = 40
    p = np.zeros((3, 3, A))
    p[0, :, 3] = 1.0
    p[1, 0, 0] = p[1, 1, 25] = p[1, 2, 39] = 1.0
    p[2] = 1.0 / A
    return actions.policy_cdf(p)


def test_population_draw_on_hand_made_rows():
    cdfs = hand_made_tables()
    assert cdfs.shape == (3, 3, 40) and cdfs.dtype == np.uint32
    M = 4
    obs = np.array([CENTER - 2, CENTER, CENTER + 2, CENTER] * 3, np.int32)
    dev, dur = actions.policy_sample_population_numpy(9, 100, 112, 7, cdfs, M, obs, CENTER, MAX_DURATION)
    assert dev.dtype == np.int32 and dur.dtype == np.int32 and dev.shape == dur.shape == (12,)
    assert dev[:4].tolist() == [0] * 4 and dur[:4].tolist() == [3] * 4                  # table 0: action 3 whatever is seen
    assert dev[4:8].tolist() == [0, 1, 1, 1] and dur[4:8].tolist() == [0, 5, 19, 5]     # table 1: by class
    for p in range(3):                                                                 # every slice: its table, ITS id range
        lo, hi = p * M, (p + 1) * M
        d, u = actions.policy_sample_numpy(9, 100 + lo, 100 + hi, 7, cdfs[p], obs[lo:hi], CENTER, MAX_DURATION)
        assert (dev[lo:hi] == d).all() and (dur[lo:hi] == u).all(), p
    # the uniform slice depends on the ids: env_lo shifts the stream, not the policy index
    d2, u2 = actions.policy_sample_population_numpy(9, 0, 12, 7, cdfs, M, obs, CENTER, MAX_DURATION)
    assert (d2[:8] == dev[:8]).all() and (u2[:8] == dur[:8]).all()
    assert ((d2[8:] != dev[8:]) | (u2[8:] != dur[8:])).any()
    # one policy over every env is policy_sample_numpy
    d1, u1 = actions.policy_sample_population_numpy(9, 100, 112, 7, cdfs[2:], 12, obs, CENTER, MAX_DURATION)
    d, u = actions.policy_sample_numpy(9, 100, 112, 7, cdfs[2], obs, CENTER, MAX_DURATION)
    assert (d1 == d).all() and (u1 == u).all()
    for bad in (lambda: actions.policy_sample_population_numpy(9, 0, 12, 7, cdfs, 5, obs, CENTER, MAX_DURATION),
                lambda: actions.policy_sample_population_numpy(9, 0, 12, 7, cdfs[0], 4, obs, CENTER, MAX_DURATION),
                lambda: actions.policy_sample_population_numpy(9, 0, 12, 7, cdfs, 4, obs[:8], CENTER, MAX_DURATION)):
        with pytest.raises(ValueError):
            bad()


# ---- argument validation ------------------------------------------------------------------------------------------------------
def test_argument_validation_without_a_gpu(native_lib):
    from gymwipe_amd import _native as nat
    L = native_lib
    one = 16
    fake = C.c_void_p(4096)                                             # never dereferenced: validation comes first
    ep = nat.Episodes(5, 1, one, None)                                  # ep->tally_dev may be NULL
    pop = nat.Population(3, 128, one, one)

    def call(env=fake, steps=4, pop=pop, ep=ep, prev=one, nxt=one):
        return L.gw_rollout_population(env, steps, C.byref(pop) if pop is not None else None, 1, 0, 0,
                                       C.byref(ep) if ep is not None else None, prev, nxt, None)

    assert call(env=None) == nat.EINVAL and b"env is NULL" in L.gw_last_error()
    assert call(pop=None) == nat.EINVAL and b"NULL" in L.gw_last_error()
    assert call(ep=None) == nat.EINVAL and b"NULL" in L.gw_last_error()
    assert call(prev=None) == nat.EINVAL and b"NULL" in L.gw_last_error()
    assert call(nxt=None) == nat.EINVAL and b"NULL" in L.gw_last_error()
    assert call(pop=nat.Population(3, 128, None, one)) == nat.EINVAL and b"NULL" in L.gw_last_error()
    assert call(pop=nat.Population(3, 128, one, None)) == nat.EINVAL and b"NULL" in L.gw_last_error()       # never NULL here
    assert call(ep=nat.Episodes(5, 1, None, one)) == nat.EINVAL and b"NULL" in L.gw_last_error()
    assert call(steps=-1) == nat.EINVAL and b"steps" in L.gw_last_error()
    assert call(ep=nat.Episodes(-1, 1, one, one)) == nat.EINVAL and b"max_steps" in L.gw_last_error()
    assert call(pop=nat.Population(0, 128, one, one)) == nat.EINVAL
    assert call(pop=nat.Population(3, 0, one, one)) == nat.EINVAL
    assert call(pop=nat.Population(-3, -128, one, one)) == nat.EINVAL
    # (P * M != num_envs needs a handle: tests/test_rollout_population.py)
    assert call(steps=0) == nat.OK
    assert call(steps=0, ep=nat.Episodes(0, 0, one, one)) == nat.OK


# ---- the catalogue --------------------------------------------------------------------------------------------------------------
def test_every_population_rollout_instantiation_has_a_gpu_case(native_lib):
    from gymwipe_amd import _native
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import test_rollout_population as rp
    from util import kernel_instantiations
    lib_set = kernel_instantiations(_native.LIB_PATH, "ct_rollout_pop_ep")
    assert len(lib_set) == 30, sorted(lib_set)
    assert sorted(lib_set - set(rp.INSTANTIATIONS)) == [], "instantiations without a case"
    assert sorted(set(rp.INSTANTIATIONS) - lib_set) == [], "cases for instantiations the library does not have"


# ---- the agent on the oracle ------------------------------------------------------------------------------------------------------
# D = 2, P = 8 policies of M = 16 envs, 40 steps in episodes of 5, 6 generations.  The seed was picked here on the CPU, on the
# oracle alone: every seed of 0 .. 15 raises the mean fitness (the narrowest gap, seed 10: -0.400 -> -0.254); seed 0 goes from
# -0.469 in generation 0 to -0.102 in generation 5 (-0.209, -0.123, -0.105, -0.111 in between), a gap of 0.37 where a return
# is at most 0 and the best policy of a generation scores -0.27 .. -0.03.
AGENT = dict(D=2, P=8, M=16, steps=40, episode_steps=5, generations=6, seed=0)


def oracle_agent(cfg=None):
    """PopulationSearchAgent with the oracle standing in for the GPU: one CtOracle for the whole run, reset before every
    generation as the default evaluate resets the env (counters and interpreter cleared, the clock not rewound)."""
    from gymwipe_amd.agents import PopulationSearchAgent
    from oracle.ct_oracle import CtOracle, default_config
    cfg = cfg or AGENT
    D, P, M = cfg["D"], cfg["P"], cfg["M"]
    orc = CtOracle(P * M, D, config=default_config(D), nthreads=4)

    def evaluate(cdfs, generation):
        obs = orc.reset()
        state = np.zeros((P * M, 2), np.int32)
        _, tally = oracle_population_steps(orc, cdfs, M, cfg["steps"], cfg["seed"], generation * cfg["steps"], 0, obs, state,
                                           cfg["episode_steps"], True)
        return tally

    return PopulationSearchAgent(None, P, cfg["steps"], cfg["episode_steps"], seed=cfg["seed"], evaluate=evaluate,
                                 nb_actions=D * MAX_DURATION)


def assert_same_history(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x["generation"] == y["generation"] and x["mean"] == y["mean"] and x["best"] == y["best"]
        assert x["fitness"].dtype == y["fitness"].dtype and (x["fitness"] == y["fitness"]).all(), x["generation"]


def test_population_search_agent_on_the_oracle():
    one, two = oracle_agent(), oracle_agent()
    h = one.fit(AGENT["generations"])
    two.fit(AGENT["generations"])
    assert [e["generation"] for e in h] == list(range(AGENT["generations"])) and one.generation == AGENT["generations"]
    assert_same_history(h, two.history)
    assert (one.mu == two.mu).all() and (one.sigma == two.sigma).all()
    assert all(e["fitness"].shape == (AGENT["P"],) and np.isfinite(e["fitness"]).all() for e in h)      # every policy ended episodes
    assert all(e["best"] == e["fitness"].max() and e["mean"] == e["fitness"].mean() for e in h)
    assert (one.sigma >= one.SIGMA_MIN).all() and one.policy_cdf().shape == (3, AGENT["D"] * MAX_DURATION)
    assert h[-1]["mean"] > h[0]["mean"], (h[0]["mean"], h[-1]["mean"])
