"""Seeded packet erasures of the control loop on the GPU (gw_ctrl_set_loss): the loss instantiations of the step kernel and of the
fused rollout kernels against the event-driven model of tests/ctrl_loss_model.py, bit for bit, over every state field, the
controller's two, the disturbance's three and the loss's four (``loss``, ``loss_key``, ``loss_count``, ``lost``).  Loss set i
runs under disturbance set i and gain set i, so all three rules run together.  A reset env is a freshly constructed model that
goes on drawing where the old one stopped.  The fixtures are defined in tests/ctrl_loss_model.py and qualified on the model
alone in tests/test_ctrl_loss_cpu.py (every link loses decoded packets and delivers others, both ending causes occur, draws
fall on transmissions the PHY rejected, four wrong rules are told apart).  What this file does as the gains' and the
disturbance's do is in tests/ctrl_gpu_harness.py; what belongs to the loss alone is asserted here.  Every test calls
``set_loss``: none passes without it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctrl_gpu_harness as h
import ctrl_loss_model as lm
import ctrl_pid_model as pm
from ctrl_fixtures import ALL_FIELDS, T, assert_same, schedules_of
from ctrl_tiers import DIST, LOSS

LOSS_STATE = h.state_fields(LOSS)
MODEL_FIELDS = h.model_fields(LOSS)
THR = h.THR


# ---- 1. step -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("plant", [None, "dense"])
@pytest.mark.parametrize("seed,start,period", [(1, 20, 10), (2, 0, 3), (3, 50, 1)])
def test_step_with_per_env_loss_matches_the_model(seed, start, period, plant):
    r = h.step_matches_the_model(LOSS, 70, seed, start, period, plant)
    gi = r.gi
    assert_same(r.first["loss"], THR[gi], "thresholds as set")
    assert_same(r.first["loss_key"], r.lkey, "keys as set")
    assert (r.first["loss_count"] == 0).all() and (r.first["lost"] == 0).all()
    for k, got in enumerate(r.seen):
        assert_same(got["loss_count"], got["n_tx"], ("one draw per transmission", k))
    assert not (r.final["flags"] & 3).any()
    lost = r.final["lost"]
    assert (lost[gi == 0] == 0).all() and (lost[gi == 5] > 0).all()


@pytest.mark.gpu
def test_step_where_the_phy_rejects_commands_still_draws_for_them():
    """ctrl_fixtures.LAYOUTS["same_distance"]: no command decodes at the actuator; each takes its draw."""
    from test_control_loop_edges import K, PERIOD, SEED, START
    r = h.step_matches_the_model(LOSS, K, SEED, START, PERIOD, layout=lm.FAILING_LAYOUT)
    for k, got in enumerate(r.seen):
        assert_same(got["loss_count"], got["n_tx"], ("one draw per transmission", k))
    st = r.final
    assert (st["received"][:, 1] == 0).all() and (st["lost"][:, 3] > 0).any()          # nothing arrived; commands were erased too


# ---- 2. - 4. the fused rollouts, and K / 2 + K / 2 = K ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rollout_with_episodes_under_loss_matches_the_wrapper_and_splits():
    r = h.rollout_matches_the_wrapper(LOSS, lm.SHORT_MAX_STEPS)
    assert (r.st["loss_count"] > r.st["n_tx"]).sum() > 256                      # resets happened, and the count ran on
    assert (r.mid["loss_count"] > 0).all()               # the halves: the record is handle state, as age and cost are


@pytest.mark.gpu
def test_rollout_schedules_under_loss_matches_the_wrapper_and_splits():
    h.rollout_schedules_matches_the_wrapper(LOSS, lm.MAX_STEPS)


@pytest.mark.gpu
def test_rollout_feedback_under_loss_matches_the_wrapper_with_and_without_rows():
    h.rollout_feedback_matches_the_wrapper(LOSS, lm.MAX_STEPS)


# ---- 5. a partial block in the fused kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rollout_at_seventy_envs_matches_the_model_step_for_step():
    h.rollout_at_seventy_envs(LOSS)


# ---- 6. zero thresholds on a switched handle are the disturbance's handle ---------------------------------------------------------------------
@pytest.mark.gpu
def test_zero_thresholds_equal_a_handle_that_only_set_the_disturbance():
    one, two = h.fused_env(DIST), h.fused_env(DIST)
    one.set_loss(np.zeros(4))                            # default keys; `two` stays on the disturbance's kernels
    d, u = h.fused_actions()
    fields = tuple(f for f in LOSS_STATE if f not in ("loss_key", "loss_count"))
    walked = np.zeros(pm.N_FUSED, np.uint64)             # transmissions of the episodes that have ended

    def same_state(what):
        a, b = h.state_of(LOSS, one), h.state_of(LOSS, two)
        h.assert_states_equal(LOSS, a, b, what, fields)
        assert (b["loss_count"] == 0).all() and (b["loss_key"] == 0).all() and (b["lost"] == 0).all(), what   # never read or written
        assert (a["lost"] == 0).all() and (a["loss"] == 0).all(), what
        return a

    h.twin_steps(one, two, d, u, 0, 12)
    st = same_state("step")
    assert_same(st["loss_count"], st["n_tx"].astype(np.uint64), "one draw per transmission")
    assert (st["loss_count"] > 0).all()
    # the sum of n_tx over the episodes walked: one step per call from here on, n_tx read before each reset takes it away
    for k in range(12, 24):
        before = one.get_state("n_tx").astype(np.uint64)
        ended = h.twin_rollout(one, two, d[k:k + 1], u[k:k + 1], ("rollout", k))[0].cpu().numpy() != 0
        count = one.get_state("loss_count")
        now = one.get_state("n_tx").astype(np.uint64)
        walked[ended] = count[ended]                     # an ended env's count is everything it ever sent
        assert_same(count, walked + now, ("loss_count is the sum of n_tx over the episodes walked", k))
        assert (now[~ended] >= before[~ended]).all()
    assert (walked > 0).any()
    moved = same_state("rollout")["loss_count"]
    assert h.twin_rollout(one, two, d[24:], u[24:]).any()
    after = same_state("rollout")["loss_count"]
    assert (after > moved).all()
    h.twin_schedules(one, two)
    moved, after = after, same_state("schedules")["loss_count"]
    assert (after > moved).all()
    h.twin_feedback(one, two, record=True)
    moved, after = after, same_state("feedback")["loss_count"]
    assert (after > moved).all()
    h.twin_feedback(one, two, record=False)
    moved, after = after, same_state("feedback without rows")["loss_count"]
    assert (after > moved).all()
    one.close(), two.close()


# ---- 7. common random numbers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_equal_records_walk_equal_trajectories_wherever_the_envs_sit():
    A, C = h.A, h.C

    def differ(weights, nkey, lkey):
        lkey[C] ^= np.uint64(1)                          # C: everything as A but the loss key
    ang, st = h.equal_records_walk_equal_trajectories(LOSS, differ)
    assert st["lost"][A].all()
    # (the final x may agree: both envs were reset five steps before the end, face the same noise, and differ in x only once
    # a command reaches one and not the other)
    assert (ang[:, C] != ang[:, A]).any() and (st["lost"][C] != st["lost"][A]).any()


# ---- 8., 9. set_loss with a mask, mid-run; reset ------------------------------------------------------------------------------------------------
MASKED = (13, 22, 31, 40, 63, 64, 69)               # sets 1, 2, 3, 5, 7 in the full block, its last lane, the partial block's first and last
NEW_P = (0.2, 0.35, 0.15, 0.45)
NEW_THR = tuple(lm.threshold(v) for v in NEW_P)


def _new_keys(N):
    from gymwipe_amd import actions
    return actions.make_ctrl_loss(np.zeros(4), N, seed=7654321)[1]


@pytest.mark.gpu
def test_set_loss_with_a_mask_mid_run_touches_the_masked_records_and_nothing_else():
    keys = _new_keys(h.N70)

    def change(model, e):                                # the new thresholds and key, the counts from 0
        model.loss.thr, model.loss.key, model.loss.n, model.loss.lost = list(NEW_THR), int(keys[e]), 0, [0, 0, 0, 0]
    r = h.masked_set_mid_run(LOSS, MASKED, lambda env, mask: env.set_loss(NEW_P, keys, mask=mask), change, own=lm.LOSS_FIELDS)
    m = r.m
    assert (r.before["loss_count"] > 0).all()
    assert_same(r.after["loss"][m], np.tile(np.array(NEW_THR, np.uint32), (m.sum(), 1)), "masked thresholds")
    assert_same(r.after["loss_key"][m], keys[m], "masked keys")
    assert (r.after["loss_count"][m] == 0).all() and (r.after["lost"][m] == 0).all()
    assert (r.st["loss_count"][m] < r.st["n_tx"][m]).all()


@pytest.mark.gpu
def test_reset_leaves_thresholds_key_and_counts_and_the_erasures_continue_the_sequence():
    r = h.reset_mid_run(LOSS, MASKED)
    m = r.m
    for f in lm.LOSS_FIELDS + ("disturbance", "noise_key", "noise_count", "gains"):
        assert_same(r.after[f], r.before[f], ("survives a reset", f))
    assert (r.after["now"][m] == 0).all() and (r.after["n_tx"][m] == 0).all() and (r.after["loss_count"][m] > 0).all()
    assert (r.st["loss_count"][m] > r.st["n_tx"][m]).all()


# ---- 10. every announcement lost ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_with_every_announcement_erased_nothing_is_ever_received():
    K, max_steps = lm.STEPS, lm.MAX_STEPS
    _, gi, _, _ = pm.fused_layout()
    sch = schedules_of(pm.P, pm.ROLLOUT_L)
    env = h.fused_env(LOSS)
    tally, _ = env.rollout_schedules(T(sch), (max_steps, lm.FAIL_DEG), K)
    st = h.state_of(LOSS, env)
    sel = gi == lm.ALL_LOST
    assert sel.sum() == 64 and (st["loss"][sel][:, :2] == 0xFFFFFFFF).all()
    assert not (st["flags"][sel] & 3).any()                                     # no step of these envs was flagged
    assert (st["received"][sel] == 0).all()
    count = st["loss_count"][sel]
    assert_same(count, (st["lost"][sel][:, 0].astype(np.uint64) + st["lost"][sel][:, 1].astype(np.uint64)), "every draw an erased announcement")
    assert (count == K).all() and (st["lost"][sel][:, 2:] == 0).all()           # one announcement per unflagged step, no data packet
    assert (tally.cpu().numpy()[sel][:, 2] == K).all()
    assert (st["received"][gi == 0] > 0).any()
    env.close()


# ---- 11. refusals and surface ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_set_loss_refusals_come_before_any_launch_and_the_env_has_the_new_verbs():
    import torch
    import gymwipe_amd
    from gymwipe_amd import _native as nat
    from gymwipe_amd import actions
    N = 128
    some = torch.zeros((N, 4), dtype=torch.int32, device="cuda")
    keys = torch.zeros(N, dtype=torch.int64, device="cuda")
    fields = (("loss", (N, 4), np.uint32), ("loss_key", (N,), np.uint64), ("loss_count", (N,), np.uint64), ("lost", (N, 4), np.uint32))
    bad = [([0.1, 0.0, 0.0], None), (np.zeros((N - 1, 4)), None), (np.zeros(4), np.zeros(N, np.int64)),
           (np.zeros(4), np.zeros(N - 1, np.uint64)), (np.zeros(4), torch.zeros(N, dtype=torch.int32)),
           (np.array(["a", "b", "c", "d"]), None)]
    env, L = h.refusals_come_before_any_launch(LOSS, "set_loss", fields, [some, keys], ["thr_dev", "key_dev"], bad)
    for f in lm.LOSS_FIELDS:
        assert (env.get_state(f) == 0).all()
    # the refusals switched nothing: the handle still walks with an untouched one
    twin = gymwipe_amd.make("VecControlLoop-v0", num_envs=N)
    act = {"device": torch.zeros(N, dtype=torch.int32), "duration": torch.full((N,), 19, dtype=torch.int32)}
    env.step(act), twin.step(act)
    for f in ALL_FIELDS:
        assert_same(env.get_state(f), twin.get_state(f), ("unswitched", f))
    twin.close()
    top = np.full(N, 0x8000000000000001, np.uint64)      # keys with the top bit set, both ways in; probabilities beyond [0, 1]
    env.set_loss((0.0, 0.5, 2.0, -1.0), top, mask=torch.arange(N) < 64)
    env.set_loss(torch.full((N, 4), 2.0 ** -32, dtype=torch.float64, device="cuda"), T(top.view(np.int64) + 1).cuda(), mask=np.arange(N) >= 96)
    lo, hi = (np.arange(N) < 64), (np.arange(N) >= 96)
    want = np.where(lo[:, None], np.array([0, 2 ** 31, 2 ** 32 - 1, 0], np.uint32), np.where(hi[:, None], np.uint32(1), np.uint32(0)))
    assert_same(env.get_state("loss"), want.astype(np.uint32), "thresholds")
    assert_same(env.get_state("loss_key"), np.where(lo, top, np.where(hi, top + np.uint64(1), np.uint64(0))), "keys")
    buf = np.empty(N * 3)                                 # a wrong size is refused, as for every field
    for f in (b"loss", b"loss_key", b"loss_count", b"lost"):
        assert L.gw_ctrl_get_state(env._h, f, buf.ctypes.data, buf.nbytes) == nat.EFIELD
    env.close()
    env = gymwipe_amd.make("VecControlLoop-v0", num_envs=N, loss=(0.5, 0.5, 0.5, 0.5))
    assert (env.get_state("loss") == 2 ** 31).all()
    assert_same(env.get_state("loss_key"), actions.make_ctrl_loss(np.zeros(4), N)[1], "the default keys")
    assert (env.get_state("loss_key") != actions.make_ctrl_disturbance(np.zeros(4), N)[1]).all()      # not the disturbance's
    for _ in range(4):
        env.step(act)
    assert_same(env.get_state("loss_count"), env.get_state("n_tx").astype(np.uint64), "count")
    lost = env.get_state("lost")
    assert len({r.tobytes() for r in lost}) > N // 4     # the envs do not share one sequence
    r = actions.ctrl_loss_numpy(env.get_state("loss_key"), np.uint64(0))        # the first announcement of every env, by the helper
    assert r.dtype == np.uint32 and ((r < 2 ** 31) <= (lost[:, 0] >= 1)).all() and (r < 2 ** 31).any() and (r >= 2 ** 31).any()
    env.close()
