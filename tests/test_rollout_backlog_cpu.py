"""
gw_rollout_backlog, the part that needs no GPU: the restatement of the scheduler's choice (actions.backlog_sample_numpy) on
hand-computed rows, the oracle composition the GPU file compares against (oracle_backlog_steps(): CtOracle.get("qlen"),
backlog_sample_numpy, CtOracle.step, the difference of CtOracle.get("n_delivered") across the step, actions.score_numpy,
actions.episodes_numpy fed the score, CtOracle.reset(mask)), the premise that the scheduler out-delivers every fixed-duration
round-robin at a moderate load, argument validation of the entry point and the catalogue of the fused family.

Fresh envs are identical and the scheduler is deterministic, so every case first runs a prologue (oracle_prologue() here,
gpu_prologue() in the GPU file): PROLOGUE steps of util.action_stream actions, then a reset of every third env.
"""
import ctypes as C
import os
import sys

import numpy as np

from gymwipe_amd import actions

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from util import action_stream, kernel_instantiations

CENTER, MAX_DURATION = 65536, 20        # counter_traffic.py:35, envs/core.py:25 (the default configuration)
NAMES = ("obs", "reward", "done", "ended", "delivered", "device", "duration", "seen_len")
DTYPES = (np.int32, np.float32, np.uint8, np.uint8, np.int32, np.int32, np.int32, np.int32)
PROLOGUE = 6
MODERATE = 0.02                         # counter_interval at which the queues stay between 0 and 14


def new_oracle(D, n, counter_interval=None, mult=None, start_time=None, positions=None, rrm_pos=None):
    from oracle.ct_oracle import CtOracle, default_config
    cfg = default_config(D, positions=positions, mult=mult, rrm_pos=rrm_pos, start_time=start_time)
    if counter_interval is not None:
        cfg.counter_interval = counter_interval
    return CtOracle(n, D, config=cfg, nthreads=8)


def prologue_actions(D, n):
    return action_stream(29 + D, PROLOGUE, n, D)


def prologue_mask(n):
    return (np.arange(n) % 3 == 0).astype(np.uint8)


def oracle_prologue(orc):
    dev, dur = prologue_actions(orc.D, orc.n)
    orc.reset()
    for k in range(PROLOGUE):
        orc.step(dev[k], dur[k])
    orc.reset(prologue_mask(orc.n))


def delivered_now(orc):
    return orc.get("n_delivered").astype(np.int64).copy()


def oracle_chosen_steps(orc, choose, score, steps, state, max_steps, on_done, center=CENTER):
    """The oracle with episodes scored by ``score`` under actions ``choose(k, qlen) -> (device, duration, seen_len)``: the
    eight [steps][n] outputs in NAMES' order, the observation each env acts on next and the episode tally; ``state``
    ({age, ret}, int32[n][2]) is updated in place."""
    n = orc.n
    out = [np.empty((steps, n), t) for t in DTYPES]
    tally = np.zeros(actions.EP_COLS, np.int64)
    acts_on = None
    for k in range(steps):
        d, u, seen = choose(k, orc.get("qlen"))
        before = delivered_now(orc)
        obs, r, dn = orc.step(d, u)
        dl = (delivered_now(orc) - before).astype(np.int32)
        sc = actions.score_numpy(score, r, d, dl)
        ended, t = actions.episodes_numpy(state, sc, dn, max_steps, on_done)
        tally += t
        if ended.any():
            orc.reset((ended != 0).astype(np.uint8))
        for a, v in zip(out, (obs, sc.astype(np.float32), dn, ended, dl, d, u, seen)):
            a[k] = v
        acts_on = np.where(ended != 0, center, obs).astype(np.int32)
    return tuple(out), acts_on, tally


def oracle_backlog_steps(orc, policy, score, steps, state, max_steps, on_done, center=CENTER):
    return oracle_chosen_steps(orc, lambda k, q: actions.backlog_sample_numpy(policy, q, MAX_DURATION), score, steps, state,
                               max_steps, on_done, center)


def case_policy(D):
    """Non-uniform weights with one zero (sender 1; not at D = 2, where sender 0 would be chosen at every step), and a table
    that is neither monotone nor inside the action space everywhere: 255 at L = 7 and from L = 90 on."""
    w = [3 + (5 * i) % 7 for i in range(D)]
    if D > 2:
        w[1] = 0
    table = np.minimum(MAX_DURATION - 1, 3 * np.arange(actions.QUEUE_CAP + 1) + 1)
    table[7] = 255
    table[90:] = 255
    return actions.make_backlog_policy(D, w, table)


# ---- 1. the restatement -----------------------------------------------------------------------------------------------------------
def test_backlog_sample_numpy_on_hand_computed_rows():
    table = np.arange(actions.QUEUE_CAP + 1) % 16          # duration_of_len[L] = L mod 16
    table[100] = 13
    table[9] = 255
    pol = actions.make_backlog_policy(4, [2, 1, 0, 3], table)
    q = np.array([[3, 6, 50, 2],      # 6, 6, 0, 6: a tie between senders 0, 1 and 3 goes to 0; L = 3
                  [0, 0, 77, 0],      # every priority is 0 (the only backlog has weight 0): sender 0, L = 0
                  [1, 5, 100, 1],     # the zero-weight sender's full queue is passed over: 2, 5, 0, 3 -> sender 1, L = 5
                  [0, 0, 0, 100],     # L = 100 reads the table's last entry
                  [0, 9, 0, 1],       # 0, 9, 0, 3 -> sender 1, L = 9: the entry 255 clamps to max_duration - 1
                  [0, 0, 0, 0]])
    dev, dur, seen = actions.backlog_sample_numpy(pol, q, MAX_DURATION)
    assert dev.tolist() == [0, 0, 1, 3, 1, 0] and seen.tolist() == [3, 0, 5, 100, 9, 0]
    assert dur.tolist() == [3, 0, 5, 13, MAX_DURATION - 1, 0]
    assert dev.dtype == dur.dtype == seen.dtype == np.int32
    assert actions.backlog_sample_numpy(pol, q, 4)[1].tolist() == [3, 0, 3, 3, 3, 0]       # another max_duration, another clamp
    # all-zero weights give sender 0 whatever the queues hold
    zero = actions.make_backlog_policy(4, 0, table)
    dev, dur, seen = actions.backlog_sample_numpy(zero, q, MAX_DURATION)
    assert dev.tolist() == [0] * 6 and seen.tolist() == q[:, 0].tolist()
    # the default policy: the longest queue (lowest index of a tie), for min(19, 4 L)
    dev, dur, seen = actions.backlog_sample_numpy(actions.make_backlog_policy(4), q, MAX_DURATION)
    assert dev.tolist() == [2, 2, 2, 3, 1, 0] and dur.tolist() == [19, 19, 19, 19, 19, 0]
    assert actions.backlog_sample_numpy(actions.make_backlog_policy(4), np.array([[1, 2, 4, 4]]), MAX_DURATION)[1].tolist() == [16]


def test_make_backlog_policy_image_and_argument_rules():
    import pytest
    from gymwipe_amd import _native as nat
    pol = actions.make_backlog_policy(3, [1, 0, actions.SCORE_W_MAX])
    assert pol.dtype == np.uint8 and pol.shape == (actions.BACKLOG_BYTES,) == (4 * nat.MAX_DEVICES + nat.QUEUE_CAP + 1,)
    assert C.sizeof(nat.BacklogPolicy) == actions.BACKLOG_BYTES + 3                       # (padded to the int32's alignment)
    rec = nat.BacklogPolicy.from_buffer_copy(pol.tobytes() + b"\0\0\0")
    assert list(rec.w_len)[:4] == [1, 0, actions.SCORE_W_MAX, 0] and not any(list(rec.w_len)[4:])
    assert list(rec.duration_of_len) == [min(MAX_DURATION - 1, 4 * L) for L in range(nat.QUEUE_CAP + 1)]
    for bad in (dict(num_devices=1), dict(num_devices=33), dict(num_devices=3, weights=-1),
                dict(num_devices=3, weights=actions.SCORE_W_MAX + 1), dict(num_devices=3, weights=[1, 2]),
                dict(num_devices=3, weights=0.5), dict(num_devices=3, duration_of_len=[1] * 100),
                dict(num_devices=3, duration_of_len=[256] * 101)):
        with pytest.raises(ValueError):
            actions.make_backlog_policy(**bad)


# ---- 2. the premise -----------------------------------------------------------------------------------------------------------------
def test_the_scheduler_out_delivers_every_fixed_duration_round_robin_at_a_moderate_load():
    """D = 4, counter_interval = 0.02, 32 envs after the prologue, 96 steps in episodes of 8: the composition with the default
    policy delivers strictly more packets than round-robin senders at each fixed duration.  Counts of this run: backlog 23 895
    packets; round-robin 0 at duration 1, 2 943 at 3, 5 378 at 6, 9 634 at 10, 18 126 at 19 (a margin of 32 %)."""
    D, n, K, E = 4, 32, 96, 8
    neutral = actions.make_score(D)

    def run(choose):
        orc = new_oracle(D, n, MODERATE)
        oracle_prologue(orc)
        out, _, tally = oracle_chosen_steps(orc, choose, neutral, K, np.zeros((n, 2), np.int32), E, True)
        assert tally[0] == n * (K // E)
        return int(out[4].sum()), out

    pol = actions.make_backlog_policy(D)
    backlog, out = run(lambda k, q: actions.backlog_sample_numpy(pol, q, MAX_DURATION))
    assert len({tuple(out[5][:, e]) for e in range(n)}) > 1, "every env does the same: the prologue did not tell them apart"
    assert int(out[7].max()) < actions.QUEUE_CAP // 2                                      # the moderate load: no queue near its cap
    counts = {}
    for fixed in (1, 3, 6, 10, 19):
        counts[fixed], _ = run(lambda k, q: (np.full(n, k % D, np.int32), np.full(n, fixed, np.int32), q[:, k % D].astype(np.int32)))
    print("backlog %d, round-robin %s" % (backlog, counts))
    assert all(backlog > c for c in counts.values()), (backlog, counts)


def test_the_composition_replays_its_own_actions():
    """Staging the recorded device / duration rows gives every other output and the state again (what the GPU call promises
    of gw_rollout_autoreset_scored)."""
    from util import STATE_FIELDS, STAT_FIELDS
    D, n, K = 4, 48, 20
    pol, score = case_policy(D), actions.make_score(D, reward=2, delivered=[1, 3, 5, 7])
    a, b = new_oracle(D, n, MODERATE), new_oracle(D, n, MODERATE)
    oracle_prologue(a)
    oracle_prologue(b)
    sa, sb = np.zeros((n, 2), np.int32), np.zeros((n, 2), np.int32)
    out, nxt, tally = oracle_backlog_steps(a, pol, score, K, sa, 5, True)
    rep, nxt2, tally2 = oracle_chosen_steps(b, lambda k, q: (out[5][k], out[6][k], q[np.arange(n), out[5][k]].astype(np.int32)),
                                            score, K, sb, 5, True)
    for name, x, y in zip(NAMES, out, rep):
        assert x.dtype == y.dtype and (x.view(np.uint8) == y.view(np.uint8)).all(), name
    assert (nxt == nxt2).all() and (tally == tally2).all() and (sa == sb).all() and tally[0] > 0
    assert (out[5] != 1).all() and len(np.unique(out[5])) == D - 1                         # the zero-weight sender is never chosen
    assert (out[6] == MAX_DURATION - 1).any() and (out[6] < MAX_DURATION).all()
    for f in STATE_FIELDS + STAT_FIELDS:
        assert (a.get(f).view(np.uint8) == b.get(f).view(np.uint8)).all(), f


# ---- 3. argument validation ---------------------------------------------------------------------------------------------------------
def test_argument_validation_without_a_gpu(native_lib):
    from gymwipe_amd import _native as nat
    L = native_lib
    one = 16
    fake = C.c_void_p(4096)                                             # never dereferenced: validation comes first
    ep = nat.Episodes(5, 1, one, None)                                  # tally_dev may be NULL
    ok_score = nat.Score.from_buffer_copy(actions.make_score(4, 1, 3).tobytes())

    def policy(**kw):
        p = nat.BacklogPolicy.from_buffer_copy(actions.make_backlog_policy(4, [1, 2, 0, 3]).tobytes() + b"\0\0\0")
        for i, v in kw.items():
            p.w_len[int(i[1:])] = v
        return p

    def score(**kw):
        w = actions.make_score(4, 1, 3).astype(np.int32)
        for i, v in kw.items():
            w[int(i[1:])] = v
        return nat.Score.from_buffer_copy(w.tobytes())

    # gw_rollout_backlog(env, steps, pol, ep, score, obs_next, device_out, duration_out, seen_len, obs, reward, done, ended,
    #                    delivered, stream)
    def call(env=fake, steps=4, pol=policy(), ep=ep, score=ok_score, ptrs=(one,) * 9):
        return L.gw_rollout_backlog(env, steps, C.byref(pol) if pol is not None else None, C.byref(ep) if ep is not None else None,
                                    C.byref(score) if score is not None else None, *ptrs, None)

    assert call(env=None) == nat.EINVAL and b"env is NULL" in L.gw_last_error()
    assert call(pol=None) == nat.EINVAL and b"NULL" in L.gw_last_error()
    assert call(pol=None, steps=0) == nat.EINVAL
    assert call(ep=None) == nat.EINVAL and b"NULL" in L.gw_last_error()
    assert call(ep=None, steps=0) == nat.EINVAL
    for hole in range(9):                                               # every pointer in turn, delivered_dev last
        ptrs = (one,) * hole + (None,) + (one,) * (8 - hole)
        assert call(ptrs=ptrs) == nat.EINVAL and b"NULL" in L.gw_last_error(), hole
        assert call(ptrs=ptrs, steps=0) == nat.EINVAL, hole             # (before steps == 0 is looked at)
    assert call(ep=nat.Episodes(5, 1, None, one)) == nat.EINVAL and b"NULL" in L.gw_last_error()
    assert call(steps=-1) == nat.EINVAL and b"steps" in L.gw_last_error()
    assert call(ep=nat.Episodes(-1, 1, one, one)) == nat.EINVAL and b"max_steps" in L.gw_last_error()
    for bad in (policy(w0=-1), policy(w0=nat.SCORE_W_MAX + 1), policy(w3=-5), policy(w31=nat.SCORE_W_MAX + 1), policy(w17=-1)):
        assert call(pol=bad) == nat.EINVAL and b"w_len" in L.gw_last_error()
        assert call(pol=bad, steps=0) == nat.EINVAL
    for bad in (score(w0=nat.SCORE_W_MAX + 1), score(w2=-nat.SCORE_W_MAX - 1), score(w32=nat.SCORE_W_MAX + 1)):
        assert call(score=bad) == nat.EINVAL and b"weight" in L.gw_last_error()
        assert call(score=bad, steps=0) == nat.EINVAL
    assert call(steps=0) == nat.OK
    assert call(steps=0, score=None) == nat.OK                          # NULL: the built-in reward
    assert call(steps=0, pol=policy(w0=nat.SCORE_W_MAX, w31=nat.SCORE_W_MAX, w5=0), ep=nat.Episodes(0, 0, one, None)) == nat.OK
    any_bytes = policy()
    for i in range(nat.QUEUE_CAP + 1):
        any_bytes.duration_of_len[i] = 255 - i
    assert call(steps=0, pol=any_bytes) == nat.OK                       # any byte in duration_of_len is valid


# ---- 4. the catalogue ---------------------------------------------------------------------------------------------------------------
def test_the_backlog_instantiations_are_the_librarys(native_lib):
    from gymwipe_amd import _native
    import test_rollout_backlog as rb
    lib_set = kernel_instantiations(_native.LIB_PATH, "ct_rollout_backlog")
    assert len(lib_set) == 30, sorted(lib_set)
    assert sorted(lib_set - set(rb.INSTANTIATIONS)) == [], "instantiations without a case"
    assert sorted(set(rb.INSTANTIATIONS) - lib_set) == [], "cases for instantiations the library does not have"
