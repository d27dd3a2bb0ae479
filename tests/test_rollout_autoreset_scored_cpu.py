"""
gw_rollout_autoreset_scored, the part that needs no GPU: the oracle composition the GPU file compares against
(oracle_scored_autoreset_steps(): CtOracle.step on the staged rows, the difference of CtOracle.get("n_delivered") across the
step, actions.score_numpy, actions.episodes_numpy fed the score, CtOracle.reset(mask) -- tests/test_rollout_autoreset.py's
oracle_autoreset_steps() with the score), what it does with a rejected action (rejected_reference(): the three-env side oracle
of test_a_rejected_action_is_a_step_of_the_episode), argument validation of the entry point, the catalogue of the fused family
and the agent's argument rules.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from gymwipe_amd import actions

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_rollout_autoreset import N, oracle_autoreset_steps, staged_actions
from test_rollout_episodes import MAX_STEPS, new_oracle
from test_rollout_policy import CENTER, K_INST
from util import kernel_instantiations, STATE_FIELDS, STAT_FIELDS

NAMES = ("obs", "reward", "done", "ended", "delivered")
DTYPES = (np.int32, np.float32, np.uint8, np.uint8, np.int32)
BAD_STEP = 9


def delivered_now(orc):
    return orc.get("n_delivered").astype(np.int64).copy()


def case_score(D):
    """w_reward = 3 and a weight per sender, all distinct, the signs alternating."""
    return actions.make_score(D, reward=3, delivered=[(5 + 2 * d) * (-1 if d % 2 else 1) for d in range(D)])


def oracle_scored_autoreset_steps(orc, dev, dur, score, state, max_steps, on_done, center=CENTER):
    """The oracle on staged rows with episodes scored by ``score``: the five [K][n] outputs (``reward`` holds the score), the
    built-in reward [K][n] beside them, the observation each env acts on next and the episode tally; ``state`` ({age, ret},
    int32[n][2]) is updated in place."""
    K, n = dev.shape
    out = [np.empty((K, n), t) for t in DTYPES]
    plain = np.empty((K, n), np.float32)
    tally = np.zeros(actions.EP_COLS, np.int64)
    acts_on = None
    for k in range(K):
        before = delivered_now(orc)
        obs, r, dn = orc.step(dev[k], dur[k])
        dl = (delivered_now(orc) - before).astype(np.int32)
        sc = actions.score_numpy(score, r, dev[k], dl)
        ended, t = actions.episodes_numpy(state, sc, dn, max_steps, on_done)
        tally += t
        if ended.any():
            orc.reset((ended != 0).astype(np.uint8))
        for a, v in zip(out, (obs, sc.astype(np.float32), dn, ended, dl)):
            a[k] = v
        plain[k] = r
        acts_on = np.where(ended != 0, center, obs).astype(np.int32)
    return tuple(out), plain, acts_on, tally


def rejected_reference(D, score, K=K_INST, bad=(0, N // 2, N - 1)):
    """The composition around a rejected action: step BAD_STEP of the envs ``bad`` is outside the action space.  The oracle
    refuses such rows, so those envs come from a second oracle of three envs that skips the step but not its bookkeeping: the
    row repeats what the env acted on and its done, delivers 0 and scores 0, and is a step of the episode.  Returns the big
    oracle's run (its three columns are to be ignored) and the small one's."""
    bad = list(bad)
    dev, dur = staged_actions(D, K)
    big, small = new_oracle(D), new_oracle(D, n=3)
    big.reset()
    state_big = np.zeros((N, 2), np.int32)
    want, _, acts_big, _ = oracle_scored_autoreset_steps(big, dev, dur, score, state_big, MAX_STEPS, True)
    small.reset()
    state = np.zeros((3, 2), np.int32)
    rows = [np.empty((K, 3), t) for t in DTYPES]
    acts_on, dn_cur, ended_on_bad = np.full(3, CENTER, np.int32), np.zeros(3, np.uint8), None
    for k in range(K):
        d3, u3 = np.ascontiguousarray(dev[k, bad]), np.ascontiguousarray(dur[k, bad])
        if k == BAD_STEP:                                               # no step: nothing moved, nothing is delivered or scored
            obs, dn = acts_on.copy(), dn_cur.copy()
            dl, sc = np.zeros(3, np.int32), np.zeros(3, np.int32)
        else:
            before = delivered_now(small)
            obs, r, dn = small.step(d3, u3)
            dl = (delivered_now(small) - before).astype(np.int32)
            sc = actions.score_numpy(score, r, d3, dl)
        ended, _ = actions.episodes_numpy(state, sc, dn, MAX_STEPS, True)
        if ended.any():
            small.reset((ended != 0).astype(np.uint8))
        if k == BAD_STEP:
            ended_on_bad = ended.copy()
        for a, v in zip(rows, (obs, sc.astype(np.float32), dn, ended, dl)):
            a[k] = v
        acts_on = np.where(ended != 0, CENTER, obs).astype(np.int32)
        dn_cur = np.where(ended != 0, 0, dn).astype(np.uint8)
    if not (ended_on_bad == 2).any():
        raise RuntimeError("no env reached the step limit on the rejected step")
    if not (rows[4].sum(axis=0) > 0).all() or not (rows[1] != 0).any():
        raise RuntimeError("the three envs deliver or score nothing")
    return {"dev": dev, "dur": dur, "bad": bad, "others": np.setdiff1d(np.arange(N), bad), "want": want, "acts_big": acts_big,
            "state_big": state_big, "big": big, "rows": tuple(rows), "acts_on": acts_on, "state": state, "small": small}


# ---- 1. the composition ---------------------------------------------------------------------------------------------------------
def test_oracle_composition_scores_the_staged_steps():
    """The neutral score is the unscored composition (tests/test_rollout_autoreset.py's); a score over packets adds exactly
    w[device] * delivered per step, changes no trajectory, and the per-step packets sum to what the oracle's counter gained."""
    D, K = 4, 24
    dev, dur = staged_actions(D, K)
    weights = [5, -7, 11, 13]
    runs = []
    for score in (None, actions.make_score(D), actions.make_score(D, reward=3, delivered=weights)):
        orc = new_oracle(D)
        orc.reset()
        state = np.zeros((N, 2), np.int32)
        if score is None:
            out, nxt, tally = oracle_autoreset_steps(orc, dev, dur, state, MAX_STEPS, True)
            runs.append((out, None, nxt, tally, state, orc))
        else:
            out, plain, nxt, tally = oracle_scored_autoreset_steps(orc, dev, dur, score, state, MAX_STEPS, True)
            runs.append((out, plain, nxt, tally, state, orc))
    base, neutral, weighted = runs
    for a, b in zip(base[0], neutral[0][:4]):
        assert a.dtype == b.dtype and (a.view(np.uint8) == b.view(np.uint8)).all()
    assert (neutral[1] == neutral[0][1]).all() and (base[2] == neutral[2]).all() and (base[3] == neutral[3]).all()
    assert (base[4] == neutral[4]).all()
    out, plain = weighted[0], weighted[1]
    assert (plain == base[0][1]).all()
    assert (out[1] == 3 * plain + np.array(weights)[dev] * out[4]).all() and out[4].sum() > 0 and (out[4] >= 0).all()
    assert (out[1] != plain).any()
    for i in (0, 2, 3, 4):                                              # obs, done, ended, delivered: the score changes no trajectory
        assert (out[i] == neutral[0][i]).all()
    assert (weighted[2] == base[2]).all()
    for f in STATE_FIELDS + STAT_FIELDS:
        assert (weighted[5].get(f).view(np.uint8) == base[5].get(f).view(np.uint8)).all(), f
    assert (out[4].sum(axis=0) == weighted[5].get("n_delivered")).all()             # (a reset leaves the counter alone)
    assert weighted[3][:3].tolist() == base[3][:3].tolist() and weighted[3][0] > 0
    assert weighted[3][3] != base[3][3] and weighted[3][4] != base[3][4]


# ---- 2. a rejected action ---------------------------------------------------------------------------------------------------------
def test_a_rejected_action_in_the_composition_scores_0_and_delivers_0():
    ref = rejected_reference(4, case_score(4))
    obs, reward, done, ended, delivered = ref["rows"]
    assert (delivered[BAD_STEP] == 0).all() and (reward[BAD_STEP] == 0).all()
    assert (ended[BAD_STEP] == 2).any()                                 # still a step of the episode: it reaches the limit
    assert (obs[BAD_STEP] == np.where(ended[BAD_STEP - 1] != 0, CENTER, obs[BAD_STEP - 1])).all()
    ends = np.flatnonzero(ended[:, 0])                                   # every episode is MAX_STEPS rows long, the rejected row among them
    assert (np.diff(np.concatenate(([-1], ends))) == MAX_STEPS).all()
    assert (delivered.sum(axis=0) == ref["small"].get("n_delivered")).all()


# ---- 3. argument validation ---------------------------------------------------------------------------------------------------------
def test_argument_validation_without_a_gpu(native_lib):
    from gymwipe_amd import _native as nat
    L = native_lib
    one = 16
    fake = C.c_void_p(4096)                                             # never dereferenced: validation comes first
    ep = nat.Episodes(5, 1, one, None)                                  # tally_dev may be NULL
    ok = nat.Score.from_buffer_copy(actions.make_score(4, 1, 3).tobytes())

    def image(**kw):
        w = actions.make_score(4, 1, 3).astype(np.int32)
        for i, v in kw.items():
            w[int(i[1:])] = v
        return nat.Score.from_buffer_copy(w.tobytes())

    # gw_rollout_autoreset_scored(env, steps, device, duration, ep, score, obs_next, obs, reward, done, ended, delivered, stream)
    def call(env=fake, steps=4, ep=ep, score=ok, ptrs=(one,) * 8):
        return L.gw_rollout_autoreset_scored(env, steps, ptrs[0], ptrs[1], C.byref(ep) if ep is not None else None,
                                             C.byref(score) if score is not None else None, *ptrs[2:], None)

    assert call(env=None) == nat.EINVAL and b"env is NULL" in L.gw_last_error()
    assert call(ep=None) == nat.EINVAL and b"NULL" in L.gw_last_error()
    assert call(score=None) == nat.EINVAL and b"NULL" in L.gw_last_error()
    assert call(score=None, steps=0) == nat.EINVAL
    for hole in range(8):                                               # every pointer in turn, delivered_dev last
        ptrs = (one,) * hole + (None,) + (one,) * (7 - hole)
        assert call(ptrs=ptrs) == nat.EINVAL and b"NULL" in L.gw_last_error(), hole
        assert call(ptrs=ptrs, steps=0) == nat.EINVAL, hole             # (before steps == 0 is looked at)
    assert call(ep=nat.Episodes(5, 1, None, one)) == nat.EINVAL and b"NULL" in L.gw_last_error()
    assert call(steps=-1) == nat.EINVAL and b"steps" in L.gw_last_error()
    assert call(ep=nat.Episodes(-1, 1, one, one)) == nat.EINVAL and b"max_steps" in L.gw_last_error()
    for bad in (image(w0=nat.SCORE_W_MAX + 1), image(w0=-nat.SCORE_W_MAX - 1), image(w2=nat.SCORE_W_MAX + 1),
                image(w32=-nat.SCORE_W_MAX - 1)):
        assert call(score=bad) == nat.EINVAL and b"weight" in L.gw_last_error()
        assert call(score=bad, steps=0) == nat.EINVAL
    assert call(score=image(w0=nat.SCORE_W_MAX, w4=-nat.SCORE_W_MAX, w32=nat.SCORE_W_MAX), steps=0) == nat.OK
    assert call(steps=0) == nat.OK
    assert call(steps=0, ep=nat.Episodes(0, 0, one, None)) == nat.OK


# ---- 4. the catalogue ---------------------------------------------------------------------------------------------------------------
def test_the_scored_autoreset_instantiations_are_the_librarys(native_lib):
    from gymwipe_amd import _native
    import test_rollout_autoreset as ra
    import test_rollout_autoreset_scored as rs
    lib_set = kernel_instantiations(_native.LIB_PATH, "ct_rollout_sync_eps")
    assert len(lib_set) == 30, sorted(lib_set)
    assert sorted(lib_set - set(rs.INSTANTIATIONS)) == [], "instantiations without a case"
    assert sorted(set(rs.INSTANTIATIONS) - lib_set) == [], "cases for instantiations the library does not have"
    parent = kernel_instantiations(_native.LIB_PATH, "ct_rollout_sync_ep")
    assert len(parent) == 30 and parent == set(ra.INSTANTIATIONS), sorted(parent)


# ---- 5. the agent's argument rules ----------------------------------------------------------------------------------------------------
class _Space:
    def __init__(self, n):
        self.n = n


class _StubEnv:
    """What DqnCounterTrafficAgent's constructor reads of an env; any call into it fails the test."""
    num_envs, device, MAX_ASSIGN_DURATION, COUNTER_BOUND = 8, "cpu", 20, CENTER

    class action_space:
        spaces = {"device": _Space(4), "duration": _Space(20)}

    def __getattr__(self, name):
        raise AssertionError("the agent touched env.%s before checking its arguments" % name)


def test_the_agent_refuses_a_score_without_episode_steps():
    from gymwipe_amd.agents import DqnCounterTrafficAgent
    agent = DqnCounterTrafficAgent(_StubEnv(), memory_limit=64)
    score = actions.make_score(4, reward=0, delivered=1)
    with pytest.raises(ValueError, match="episode_steps"):
        agent.fit(4, score=score)
    with pytest.raises(ValueError, match="episode_steps"):
        agent.collect(4, score=score)
    assert agent.steps == 0 and agent.m_len == 0
