"""
The _delivered tallying calls (gw_rollout_policy_stats_delivered, gw_rollout_episodes_stats_delivered,
gw_transition_stats_delivered), the part that needs no GPU: the CPU restatement of the eight-column table
(actions.transition_stats_numpy(delivered=)) on hand-computed rows, actions.table_score against actions.score_numpy summed per
bin, argument validation of the three entry points, the catalogue of the two fused families (as many instantiations as their
parents), and the premise on the oracle alone: Q-iteration on the table's reward sums learns to idle, on its packet sums it
learns to deliver.
"""
import ctypes as C
import os
import sys

import numpy as np

from gymwipe_amd import actions

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_rollout_scored_cpu import CENTER, MAX_DURATION, new_oracle, oracle_scored_steps      # noqa: E402


def test_transition_stats_numpy_with_delivered_on_a_hand_computed_example():
    """tests/test_rollout_stats_cpu.py's two envs and three steps (D = 2, A = 40), with packets per step:
        env 0  (at,    a = 3)   delivered -3 -> 0          env 1  (below, a = 20)  delivered 65 535
               (above, a = 39)  delivered  70 000 -> 65 535       (2, 0): outside the action space, skipped (its 9 with it)
               (at,    a = 3)   delivered  4                      (at,    a = 3)   delivered 0
    Columns 0-6 are the parent's; column 7 sums the clamped counts."""
    c = 65536
    rows = dict(obs_prev=[c, c - 2],
                device=[[0, 1], [1, 2], [0, 0]], duration=[[3, 0], [19, 0], [3, 3]],
                obs=[[c + 2, c], [c, c], [c - 2, c]],
                reward=[[2.0, -50.0], [3.6, 7.0], [-2.5, 0.0]], done=[[0, 2], [1, 9], [0, 0]],
                center=c, max_duration=20, num_devices=2)
    t = actions.transition_stats_numpy(delivered=[[-3, 65535], [70000, 9], [4, 0]], **rows)
    assert actions.TSD_COLS == 8 and t.dtype == np.int64 and t.shape == (3, 40, 8)
    want = np.zeros((3, 40, 8), np.int64)
    want[1, 3] = [3, 0, 8, 1, 1, 1, 0, 4]
    want[2, 39] = [1, 4, 16, 0, 1, 0, 1, 65535]
    want[0, 20] = [1, -10, 100, 0, 1, 0, 1, 65535]
    assert (t == want).all(), np.argwhere(t != want).tolist()
    assert (t[..., :7] == actions.transition_stats_numpy(**rows)).all()
    # ended rows: env 0's step 1 ended its episode, so its step 2 acted on the reset's observation -- class 1 whatever obs[1] says
    rows["obs"] = [[c + 2, c], [c + 2, c], [c - 2, c]]
    ended = [[0, 0], [1, 0], [0, 0]]
    e = actions.transition_stats_numpy(ended=ended, delivered=[[1, 2], [3, 4], [5, 6]], **rows)
    assert e[1, 3].tolist() == [3, 0, 8, 1, 1, 1, 0, 1 + 5 + 6] and e[2, 39, 7] == 3 and e[0, 20, 7] == 2
    assert e[..., 7].sum() == 1 + 2 + 3 + 5 + 6                                  # the skipped row's 4 is not counted
    assert (e[..., :7] == actions.transition_stats_numpy(ended=ended, **rows)).all()
    without = actions.transition_stats_numpy(delivered=[[1, 2], [3, 4], [5, 6]], **rows)
    assert without[2, 3, 7] == 5 and without[1, 3, 7] == 1 + 6                    # (no ended: step 2 of env 0 saw obs[1], above)
    empty = actions.transition_stats_numpy([c, c], *[np.zeros((0, 2))] * 5, c, 20, 2, delivered=np.zeros((0, 2)))
    assert empty.shape == (3, 40, 8) and not empty.any()


def test_table_score_is_the_sum_of_the_step_scores_per_bin():
    rng = np.random.default_rng(17)
    D, md, n, steps = 5, 7, 33, 40
    A = D * md
    dev = rng.integers(-1, D + 1, (steps, n)).astype(np.int32)
    dur = rng.integers(-1, md + 1, (steps, n)).astype(np.int32)
    values = np.array([CENTER - 2, CENTER, CENTER + 2], np.int32)
    obs, obs_prev = values[rng.integers(0, 3, (steps, n))], values[rng.integers(0, 3, n)]
    rew = rng.integers(-10, 11, (steps, n)).astype(np.float32)
    done = (rng.random((steps, n)) < 0.2).astype(np.uint8)
    dl = rng.integers(0, 12, (steps, n)).astype(np.int32)
    table = actions.transition_stats_numpy(obs_prev, dev, dur, obs, rew, done, CENTER, md, D, delivered=dl)
    ok = (dev >= 0) & (dev < D) & (dur >= 0) & (dur < md)
    seen = np.concatenate([obs_prev[None], obs[:-1]])
    row = ((np.sign(seen.astype(np.int64) - CENTER) + 1) * A + dev.astype(np.int64) * md + dur)[ok]
    for score in (actions.make_score(D), actions.make_score(D, reward=0, delivered=1),
                  actions.make_score(D, reward=-3, delivered=[5, -7, 11, 0, 1024])):
        want = np.zeros(3 * A, np.int64)
        np.add.at(want, row, actions.score_numpy(score, rew[ok], dev[ok], dl[ok]).astype(np.int64))
        got = actions.table_score(table, score, md)
        assert got.dtype == np.int64 and got.shape == (3, A)
        assert (got == want.reshape(3, A)).all()
    assert (actions.table_score(table, actions.make_score(D), md) == table[..., 1]).all()      # the neutral score: the reward sums
    import torch
    tt = actions.table_score(torch.from_numpy(table), actions.make_score(D, reward=2, delivered=[1, 2, 3, 4, 5]), md)
    assert tt.dtype == torch.int64
    assert (tt.numpy() == actions.table_score(table, actions.make_score(D, reward=2, delivered=[1, 2, 3, 4, 5]), md)).all()
    for bad in (table[..., :7], table[:2]):
        try:
            actions.table_score(bad, actions.make_score(D), md)
        except ValueError:
            continue
        raise AssertionError("a table of shape %s was accepted" % (bad.shape,))


def test_argument_validation_without_a_gpu(native_lib):
    from gymwipe_amd import _native as nat
    L = native_lib
    one = C.c_void_p(16)
    fake = C.c_void_p(4096)                                             # never dereferenced: validation comes first
    ep = nat.Episodes(5, 1, 16, None)
    # gw_rollout_policy_stats_delivered(env, steps, cdf, seed, step0, env_id0, obs_prev, obs_last, return (may be NULL), table, stream)
    f = L.gw_rollout_policy_stats_delivered
    assert f(None, 4, one, 1, 0, 0, one, one, one, one, None) == nat.EINVAL and b"env is NULL" in L.gw_last_error()
    assert f(fake, -1, one, 1, 0, 0, one, one, one, one, None) == nat.EINVAL and b"steps < 0" in L.gw_last_error()
    for hole in range(4):
        ptrs = [one] * 4
        ptrs[hole] = None
        assert f(fake, 4, ptrs[0], 1, 0, 0, ptrs[1], ptrs[2], None, ptrs[3], None) == nat.EINVAL, hole
        assert b"gw_rollout_policy_stats_delivered: NULL" in L.gw_last_error(), hole
    assert f(fake, 0, one, 1, 0, 0, one, one, None, one, None) == nat.OK
    # gw_rollout_episodes_stats_delivered(env, steps, cdf, seed, step0, env_id0, ep, obs_prev, obs_next, table, stream)
    g = L.gw_rollout_episodes_stats_delivered
    assert g(None, 4, one, 1, 0, 0, C.byref(ep), one, one, one, None) == nat.EINVAL and b"env is NULL" in L.gw_last_error()
    assert g(fake, -1, one, 1, 0, 0, C.byref(ep), one, one, one, None) == nat.EINVAL
    for hole in range(4):
        ptrs = [one] * 4
        ptrs[hole] = None
        assert g(fake, 4, ptrs[0], 1, 0, 0, C.byref(ep), ptrs[1], ptrs[2], ptrs[3], None) == nat.EINVAL, hole
        assert b"gw_rollout_episodes_stats_delivered: NULL" in L.gw_last_error(), hole
    assert g(fake, 4, one, 1, 0, 0, None, one, one, one, None) == nat.EINVAL
    assert g(fake, 4, one, 1, 0, 0, C.byref(nat.Episodes(5, 1, None, None)), one, one, one, None) == nat.EINVAL
    assert g(fake, 4, one, 1, 0, 0, C.byref(nat.Episodes(-1, 1, 16, None)), one, one, one, None) == nat.EINVAL
    assert b"max_steps" in L.gw_last_error()
    assert g(fake, 0, one, 1, 0, 0, C.byref(ep), one, one, one, None) == nat.OK
    # gw_transition_stats_delivered(env, steps, obs_prev, device, duration, obs, reward, done, ended (may be NULL), delivered, table, stream)
    h = L.gw_transition_stats_delivered
    assert h(None, 4, *[one] * 9, None) == nat.EINVAL and b"env is NULL" in L.gw_last_error()
    assert h(fake, -1, *[one] * 9, None) == nat.EINVAL
    for hole in (0, 1, 2, 3, 4, 5, 7, 8):
        ptrs = [one] * 9
        ptrs[hole] = None
        assert h(fake, 4, *ptrs, None) == nat.EINVAL and b"gw_transition_stats_delivered: NULL" in L.gw_last_error(), hole
    assert h(fake, 0, *[one] * 9, None) == nat.OK
    ptrs = [one] * 9
    ptrs[6] = None                                                      # ended may be NULL
    assert h(fake, 0, *ptrs, None) == nat.OK


def test_the_delivered_families_have_their_parents_instantiations(native_lib):
    from gymwipe_amd import _native
    from util import kernel_instantiations

    def args_of(family):
        names = kernel_instantiations(_native.LIB_PATH, family)
        assert all(n.startswith(family + "<") for n in names)
        return sorted(n[len(family):] for n in names)

    for family, parent, count in (("ct_rollout_pstats_d", "ct_rollout_pstats", 30), ("ct_rollout_pstats_epd", "ct_rollout_pstats_ep", 30),
                                  ("transition_stats_rows_d", "transition_stats_rows", 4)):
        assert len(args_of(parent)) == count, (parent, args_of(parent))
        assert args_of(family) == args_of(parent), family


# ---- the premise --------------------------------------------------------------------------------------------------------------
def greedy(q):
    """The table that always takes each class's best action."""
    p = np.zeros(q.shape)
    p[np.arange(3), q.argmax(axis=1)] = 1.0
    return actions.policy_cdf(p)


def test_reward_sums_teach_idleness_and_packet_sums_teach_delivery():
    """D = 4, 64 envs, the default configuration: a uniform policy for 96 steps in episodes of 8, its transitions tallied as
    transition_stats_numpy(delivered=) tallies them; Q-iteration (gamma 0.9, 50 sweeps) once on the table's reward sums and
    once on its packet sums; each greedy policy run for 96 further steps on an oracle of its own."""
    import torch
    from gymwipe_amd.agents import TabularCounterTrafficAgent
    D, n, steps, episode, seed = 4, 64, 96, 8, 5
    A = D * MAX_DURATION
    neutral = actions.make_score(D)

    def run(cdf, step0):
        orc = new_oracle(D, n)
        obs, state = orc.reset(), np.zeros((n, 2), np.int32)
        out, plain, _, tally = oracle_scored_steps(orc, cdf, neutral, steps, seed, step0, 0, obs, state, episode, True)
        assert (out[3] == plain).all() and tally[0] > 0
        return obs, out, tally

    obs0, out, tally = run(actions.policy_cdf(np.full((3, A), 1.0 / A)), 0)
    table = actions.transition_stats_numpy(obs0, *out[:5], CENTER, MAX_DURATION, D, ended=out[5], delivered=out[6])
    assert table[..., 0].sum() == steps * n and table[..., 7].sum() == out[6].sum()
    per_episode = {"uniform": out[6].sum() / tally[0]}
    most = int(out[6].max())
    q0, t = torch.zeros((3, A), dtype=torch.float64), torch.from_numpy(table)
    sums = {"reward": None, "packets": actions.table_score(t, actions.make_score(D, reward=0, delivered=1), MAX_DURATION)}
    assert (sums["packets"].numpy() == table[..., 7]).all()
    for name, r_sum in sums.items():
        q = TabularCounterTrafficAgent.q_iteration(q0, t, 0.9, 50, r_sum=r_sum).numpy()
        _, got, tl = run(greedy(q), steps)
        per_episode[name] = got[6].sum() / tl[0]
        most = max(most, int(got[6].max()))
    print("packets per episode: %s; most in one step: %d" % (per_episode, most))
    assert per_episode["reward"] == 0.0                                 # it idles after every reset
    assert per_episode["packets"] > per_episode["uniform"] > 0.0
    assert 0 < most <= actions.TSD_DELIVERED_MAX
