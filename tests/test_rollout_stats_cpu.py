"""
gw_rollout_policy_stats / gw_transition_stats, the part that needs no GPU: the CPU restatement of the table
(actions.transition_stats_numpy), argument validation of both entry points, the catalogue of the fused family -- the library's
ct_rollout_pstats<DT, MODE> instantiations are exactly the cases tests/test_rollout_stats.py runs -- and the tabular agent's
Q-iteration against its closed form.
"""
import ctypes as C
import os
import sys
import types

import numpy as np

from gymwipe_amd import actions


def test_transition_stats_numpy_on_a_hand_computed_example():
    """Two envs, three steps, D = 2, max_duration = 20, centre 65536 (A = 40).  Worked by hand:
        env 0  sees 65536 (at),    takes (0, 3)  = 3,  lands above, reward  2,   done 0
               sees 65538 (above), takes (1, 19) = 39, lands at,    reward  3.6 -> 4, done 1
               sees 65536 (at),    takes (0, 3)  = 3,  lands below, reward -2.5 -> -2 (ties to even), done 0
        env 1  sees 65534 (below), takes (1, 0)  = 20, lands at,    reward -50 -> -10, done 2 (counts once)
               sees 65536 (at),    takes (2, 0): outside the action space, skipped
               sees 65536 (at: the skipped step's own observation), takes (0, 3) = 3, lands at, reward 0, done 0"""
    c = 65536
    t = actions.transition_stats_numpy(
        obs_prev=[c, c - 2],
        device=[[0, 1], [1, 2], [0, 0]], duration=[[3, 0], [19, 0], [3, 3]],
        obs=[[c + 2, c], [c, c], [c - 2, c]],
        reward=[[2.0, -50.0], [3.6, 7.0], [-2.5, 0.0]], done=[[0, 2], [1, 9], [0, 0]],
        center=c, max_duration=20, num_devices=2)
    assert t.dtype == np.int64 and t.shape == (3, 40, 7)
    want = np.zeros((3, 40, 7), np.int64)
    want[1, 3] = [3, 0, 8, 1, 1, 1, 0]            # rewards 2, -2, 0; next above, below, at
    want[2, 39] = [1, 4, 16, 0, 1, 0, 1]
    want[0, 20] = [1, -10, 100, 0, 1, 0, 1]
    assert (t == want).all(), np.argwhere(t != want).tolist()
    assert t[..., 0].sum() == 5                    # six rows, one skipped
    empty = actions.transition_stats_numpy([c, c], np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 2)),
                                           np.zeros((0, 2)), c, 20, 2)
    assert empty.shape == (3, 40, 7) and not empty.any()
    nan = actions.transition_stats_numpy([c], [[0]], [[0]], [[c]], [[np.nan]], [[0]], c, 20, 2)
    assert nan[1, 0].tolist() == [1, -10, 100, 0, 1, 0, 0]


def test_argument_validation_without_a_gpu(native_lib):
    from gymwipe_amd import _native as nat
    L = native_lib
    one = C.c_void_p(16)
    fake = C.c_void_p(4096)                                             # never dereferenced: validation comes first
    # gw_rollout_policy_stats(env, steps, cdf, seed, step0, env_id0, obs_prev, obs_last, return (may be NULL), table, stream)
    assert L.gw_rollout_policy_stats(None, 4, one, 1, 0, 0, one, one, one, one, None) == nat.EINVAL
    assert b"env is NULL" in L.gw_last_error()
    assert L.gw_rollout_policy_stats(fake, -1, one, 1, 0, 0, one, one, one, one, None) == nat.EINVAL
    for hole in range(4):
        ptrs = [one] * 4
        ptrs[hole] = None
        rc = L.gw_rollout_policy_stats(fake, 4, ptrs[0], 1, 0, 0, ptrs[1], ptrs[2], None, ptrs[3], None)
        assert rc == nat.EINVAL and b"NULL" in L.gw_last_error(), hole
    assert L.gw_rollout_policy_stats(fake, 0, one, 1, 0, 0, one, one, None, one, None) == nat.OK
    # gw_transition_stats(env, steps, obs_prev, device, duration, obs, reward, done, table, stream)
    assert L.gw_transition_stats(None, 4, one, one, one, one, one, one, one, None) == nat.EINVAL
    assert b"env is NULL" in L.gw_last_error()
    assert L.gw_transition_stats(fake, -1, one, one, one, one, one, one, one, None) == nat.EINVAL
    for hole in range(7):
        ptrs = [one] * 7
        ptrs[hole] = None
        assert L.gw_transition_stats(fake, 4, *ptrs, None) == nat.EINVAL and b"NULL" in L.gw_last_error(), hole
    assert L.gw_transition_stats(fake, 0, one, one, one, one, one, one, one, None) == nat.OK


def test_every_stats_rollout_instantiation_has_a_gpu_case(native_lib):
    from gymwipe_amd import _native
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import test_rollout_stats as rs
    from util import kernel_instantiations
    lib_set = kernel_instantiations(_native.LIB_PATH, "ct_rollout_pstats")
    assert len(lib_set) == 30, sorted(lib_set)
    assert sorted(lib_set - set(rs.INSTANTIATIONS)) == [], "instantiations without a case"
    assert sorted(set(rs.INSTANTIATIONS) - lib_set) == [], "cases for instantiations the library does not have"


def test_tabular_agent_learn_against_the_closed_form():
    """A made-up 3 x 4 table (D = 2 senders x 2 durations).  Class 0's visited pairs all lead to class 0 and class 2's to
    class 2, so their values are geometric series; class 1 mixes.  With gamma = 1/2:
        (0, a0): r = 1 always, never done           Q = 1 + Q/2                 -> 2       (the class's best action)
        (0, a1): r = -1, never done                 Q = -1 + V0/2               -> 0
        (2, a3): r = 4, done half of the time       Q = 4 + (1/2)(1/2) Q        -> 16/3
        (1, a2): r = 0, next 1/4 below 3/4 above    Q = (1/2)(V0/4 + 3 V2/4)    -> 1/4 + 2 = 9/4
    every other pair is unvisited and keeps the value it had (below the visited ones, so the maxima above stand)."""
    import torch
    from gymwipe_amd.agents import TabularCounterTrafficAgent
    env = types.SimpleNamespace(device=torch.device("cpu"), num_devices=2, config=types.SimpleNamespace(max_duration=2), _last=(None,))
    agent = TabularCounterTrafficAgent(env, gamma=0.5, tau=1.0)
    assert agent.q.shape == (3, 4) and agent.q.dtype == torch.float64 and agent.table.shape == (3, 4, 7)
    agent.q[:] = -7.0
    t = agent.table
    t[0, 0] = torch.tensor([8, 8, 8, 8, 0, 0, 0])
    t[0, 1] = torch.tensor([2, -2, 2, 2, 0, 0, 0])
    t[2, 3] = torch.tensor([6, 24, 96, 0, 0, 6, 3])
    t[1, 2] = torch.tensor([4, 0, 0, 1, 0, 3, 0])
    q = agent.learn(200).numpy()                                       # the slowest mode contracts by 1/2 per sweep
    want = np.full((3, 4), -7.0)
    want[0, 0], want[0, 1], want[2, 3], want[1, 2] = 2.0, 0.0, 16.0 / 3.0, 9.0 / 4.0
    assert np.abs(q - want).max() < 1e-12, q
    # one sweep from Q = 0 is the mean reward of the visited pairs
    one = TabularCounterTrafficAgent.q_iteration(torch.zeros((3, 4), dtype=torch.float64), t, 0.5, 1).numpy()
    assert one[0, 0] == 1.0 and one[0, 1] == -1.0 and one[2, 3] == 4.0 and one[1, 2] == 0.0 and one[1, 0] == 0.0
    # the policy's table: the Boltzmann rule on Q, through actions.policy_cdf
    p = torch.softmax(torch.clamp(agent.q / agent.tau, -500.0, 500.0), dim=-1)
    assert (agent.policy_cdf().numpy() == actions.policy_cdf(p.numpy()).astype(np.int64)).all()
