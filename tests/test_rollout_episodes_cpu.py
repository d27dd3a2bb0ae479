"""
gw_rollout_episodes / gw_rollout_episodes_stats / gw_transition_stats_ep, the part that needs no GPU: the CPU restatement of the
per-step bookkeeping (actions.episodes_numpy), transition_stats_numpy's `ended` argument, argument validation of the three
entry points, and the catalogue of the two fused families -- the library's ct_rollout_policy_ep<DT, MODE> and
ct_rollout_pstats_ep<DT, MODE> instantiations are exactly the cases tests/test_rollout_episodes.py runs.
"""
import ctypes as C
import os
import sys

import numpy as np

from gymwipe_amd import actions


def test_episodes_numpy_on_hand_made_rows():
    """Four envs, max_steps = 3, on_done set.  Ages before the step: 0, 2, 2, 1.
        env 0  age 1, no done                      -> goes on
        env 1  age 3 = max_steps, no done          -> ended by the step limit (2)
        env 2  age 3 = max_steps AND done          -> ended by done (1): done wins
        env 3  age 2, done                         -> ended by done (1)"""
    state = np.array([[0, 0], [2, 5], [2, -4], [1, 10]], np.int32)
    ended, tally = actions.episodes_numpy(state, np.array([2.0, -3.0, -6.0, 10.0], np.float32), np.array([0, 0, 1, 7], np.uint8), 3, True)
    assert ended.dtype == np.uint8 and ended.tolist() == [0, 2, 1, 1]
    assert state.tolist() == [[1, 2], [0, 0], [0, 0], [0, 0]]
    # episodes 3, by done 2, lengths 3 + 3 + 2, returns 2 - 10 + 20, squares 4 + 100 + 400
    assert tally.dtype == np.int64 and tally.tolist() == [3, 2, 8, 12, 504]
    assert len(tally) == actions.EP_COLS == 5


def test_episodes_numpy_carries_the_age_across_calls_and_honours_the_switches():
    state = np.zeros((2, 2), np.int32)
    total = np.zeros(5, np.int64)
    rows = []
    for k in range(7):                                                  # seven one-step calls, max_steps = 3: ends at k = 2, 5
        ended, t = actions.episodes_numpy(state, np.array([1.0, -1.0], np.float32), np.zeros(2, np.uint8), 3, True)
        rows.append(ended.tolist())
        total += t
    assert rows == [[0, 0], [0, 0], [2, 2], [0, 0], [0, 0], [2, 2], [0, 0]]
    assert state.tolist() == [[1, 1], [1, -1]] and total.tolist() == [4, 0, 12, 0, 36]
    # max_steps = 0: no step limit; on_done off: done is ignored -- age and ret only grow
    state = np.array([[9, 9], [0, 0]], np.int32)
    for _ in range(5):
        ended, t = actions.episodes_numpy(state, np.array([1.0, 0.0], np.float32), np.array([1, 1], np.uint8), 0, False)
        assert not ended.any() and not t.any()
    assert state.tolist() == [[14, 14], [5, 0]]
    ended, t = actions.episodes_numpy(state, np.array([1.0, 0.0], np.float32), np.array([0, 1], np.uint8), 0, True)
    assert ended.tolist() == [0, 1] and t.tolist() == [1, 1, 6, 0, 0] and state.tolist() == [[15, 15], [0, 0]]


def test_transition_stats_numpy_with_and_without_ended():
    """One env, three steps, D = 2 (A = 40), centre 65536.  It sees `at`, lands above; sees above -- or, where step 0 ended
    its episode, the reset's observation `at` -- and lands below; then the same question for step 2."""
    c = 65536
    rows = dict(obs_prev=[c], device=[[0], [1], [0]], duration=[[3], [4], [3]], obs=[[c + 2], [c - 2], [c]],
                reward=[[2.0], [0.0], [-2.0]], done=[[0], [0], [0]], center=c, max_duration=20, num_devices=2)
    plain = actions.transition_stats_numpy(**rows)
    assert plain[1, 3].tolist() == [1, 2, 4, 0, 0, 1, 0] and plain[2, 24].tolist() == [1, 0, 0, 1, 0, 0, 0]
    assert plain[0, 3].tolist() == [1, -2, 4, 0, 1, 0, 0] and plain[..., 0].sum() == 3
    assert (actions.transition_stats_numpy(ended=[[0], [0], [0]], **rows) == plain).all()
    assert (actions.transition_stats_numpy(ended=[[0], [0], [1]], **rows) == plain).all()       # the last row's flag: no step after it
    ep = actions.transition_stats_numpy(ended=[[2], [0], [0]], **rows)
    assert ep[1, 24].tolist() == [1, 0, 0, 1, 0, 0, 0] and not ep[2].any()                      # step 1 acted on `at`
    assert ep[1, 3].tolist() == plain[1, 3].tolist() and ep[0, 3].tolist() == plain[0, 3].tolist()
    ep = actions.transition_stats_numpy(ended=[[0], [1], [0]], **rows)
    assert ep[1, 3].tolist() == [2, 0, 8, 0, 1, 1, 0] and not ep[0].any()                       # step 2 acted on `at`


def test_argument_validation_without_a_gpu(native_lib):
    from gymwipe_amd import _native as nat
    L = native_lib
    one = C.c_void_p(16)
    fake = C.c_void_p(4096)                                             # never dereferenced: validation comes first
    ep = nat.Episodes(5, 1, 16, None)                                   # tally_dev may be NULL
    # gw_rollout_episodes(env, steps, cdf, seed, step0, env_id0, ep, obs_prev, obs_next, device, duration, obs, reward, done, ended, stream)
    nine = [one] * 9
    assert L.gw_rollout_episodes(None, 4, one, 1, 0, 0, C.byref(ep), *nine[1:], None) == nat.EINVAL
    assert b"env is NULL" in L.gw_last_error()
    assert L.gw_rollout_episodes(fake, -1, one, 1, 0, 0, C.byref(ep), *nine[1:], None) == nat.EINVAL
    for hole in range(9):
        ptrs = list(nine)
        ptrs[hole] = None
        rc = L.gw_rollout_episodes(fake, 4, ptrs[0], 1, 0, 0, C.byref(ep), *ptrs[1:], None)
        assert rc == nat.EINVAL and b"NULL" in L.gw_last_error(), hole
    assert L.gw_rollout_episodes(fake, 4, one, 1, 0, 0, None, *nine[1:], None) == nat.EINVAL
    assert L.gw_rollout_episodes(fake, 4, one, 1, 0, 0, C.byref(nat.Episodes(5, 1, None, 16)), *nine[1:], None) == nat.EINVAL
    assert b"NULL" in L.gw_last_error()
    assert L.gw_rollout_episodes(fake, 4, one, 1, 0, 0, C.byref(nat.Episodes(-1, 1, 16, 16)), *nine[1:], None) == nat.EINVAL
    assert b"max_steps" in L.gw_last_error()
    assert L.gw_rollout_episodes(fake, 0, one, 1, 0, 0, C.byref(ep), *nine[1:], None) == nat.OK
    # gw_rollout_episodes_stats(env, steps, cdf, seed, step0, env_id0, ep, obs_prev, obs_next, table, stream)
    assert L.gw_rollout_episodes_stats(None, 4, one, 1, 0, 0, C.byref(ep), one, one, one, None) == nat.EINVAL
    assert L.gw_rollout_episodes_stats(fake, -1, one, 1, 0, 0, C.byref(ep), one, one, one, None) == nat.EINVAL
    for hole in range(4):
        ptrs = [one] * 4
        ptrs[hole] = None
        rc = L.gw_rollout_episodes_stats(fake, 4, ptrs[0], 1, 0, 0, C.byref(ep), ptrs[1], ptrs[2], ptrs[3], None)
        assert rc == nat.EINVAL and b"NULL" in L.gw_last_error(), hole
    assert L.gw_rollout_episodes_stats(fake, 4, one, 1, 0, 0, None, one, one, one, None) == nat.EINVAL
    assert L.gw_rollout_episodes_stats(fake, 4, one, 1, 0, 0, C.byref(nat.Episodes(-1, 1, 16, 16)), one, one, one, None) == nat.EINVAL
    assert L.gw_rollout_episodes_stats(fake, 0, one, 1, 0, 0, C.byref(ep), one, one, one, None) == nat.OK
    # gw_transition_stats_ep(env, steps, obs_prev, device, duration, obs, reward, done, ended, table, stream)
    assert L.gw_transition_stats_ep(None, 4, *[one] * 8, None) == nat.EINVAL
    assert L.gw_transition_stats_ep(fake, -1, *[one] * 8, None) == nat.EINVAL
    for hole in range(8):
        ptrs = [one] * 8
        ptrs[hole] = None
        assert L.gw_transition_stats_ep(fake, 4, *ptrs, None) == nat.EINVAL and b"NULL" in L.gw_last_error(), hole
    assert L.gw_transition_stats_ep(fake, 0, *[one] * 8, None) == nat.OK


def test_every_episodic_rollout_instantiation_has_a_gpu_case(native_lib):
    from gymwipe_amd import _native
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import test_rollout_episodes as re_
    from util import kernel_instantiations
    for family, cases in (("ct_rollout_policy_ep", re_.INSTANTIATIONS), ("ct_rollout_pstats_ep", re_.STATS_INSTANTIATIONS)):
        lib_set = kernel_instantiations(_native.LIB_PATH, family)
        assert len(lib_set) == 30, sorted(lib_set)
        assert sorted(lib_set - set(cases)) == [], "instantiations without a case"
        assert sorted(set(cases) - lib_set) == [], "cases for instantiations the library does not have"
