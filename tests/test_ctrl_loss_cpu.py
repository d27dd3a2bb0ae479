"""Seeded packet erasures of the control loop, CPU tier: the numpy restatement of the draw against the pure-Python one the model
uses (tests/ctrl_loss_model.py), the conversion from probabilities, the model at zero thresholds against the disturbance model,
``actions.make_ctrl_loss``, the observed rate, what the loss does to a ranking of schedules, and the fixtures of the GPU tests
qualified on the model alone -- they must be able to tell a kernel that draws only for decoded packets, restarts the count at
a reset, uses one threshold for all links or leaves an erased packet in its queue from a right one."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctrl_dist_model as cd
import ctrl_loss_model as lm
import ctrl_pid_model as pm
import ctrl_tiers as ct
from ctrl_tiers import DIST, LOSS


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all(bits(a) == bits(b))) if b.dtype == np.float64 else bool(np.all(a == b))


# ---- 1. the draw ---------------------------------------------------------------------------------------------------------------------------
KEYS = (0, 1, 2, 0x8000000000000000, 0xFFFFFFFFFFFFFFFF, 0x9E3779B97F4A7C15, 0xA0761D6478BD642F, 0x8000000000000001, lm.SEED64,
        2 ** 63 + 12345)
COUNTS = tuple(range(40)) + tuple(2 ** 32 - 20 + i for i in range(40)) + (2 ** 31 - 1, 2 ** 31, 2 ** 40 + 12345, 2 ** 63, 2 ** 64 - 1) \
    + tuple(int(v) for v in np.random.default_rng(5).integers(0, 2 ** 63, 915, dtype=np.uint64) * 2 + 1)


def test_numpy_draw_equals_the_pure_python_restatement():
    from gymwipe_amd import actions
    assert len(KEYS) * len(COUNTS) == 10000 and any(k >= 2 ** 63 for k in KEYS)
    assert any(c < 2 ** 32 for c in COUNTS) and any(c >= 2 ** 32 for c in COUNTS)
    got = actions.ctrl_loss_numpy(np.array(KEYS, np.uint64)[:, None], np.array(COUNTS, np.uint64)[None, :])
    assert got.shape == (len(KEYS), len(COUNTS)) and got.dtype == np.uint32
    want = np.array([[lm.draw(k, c) for c in COUNTS] for k in KEYS], np.uint64)
    assert (got == want).all()
    assert len(set(got.ravel().tolist())) > 0.99 * got.size
    assert actions.ctrl_loss_numpy(np.uint64(7), np.uint64(9)).shape == ()       # scalars in, a scalar out
    # written out by hand from the rule, so that both restatements cannot be wrong together: key 0, n 0 is the mixer's output
    # for z = 0x9E3779B97F4A7C15 (splitmix64's first output for state 0, top 32 bits 0xE220A839), and with
    # key = 0x9E37... ^ 0xA076..., n = 1 the mixer sees z = 2 * 0x9E37...: splitmix64's second output
    assert lm.draw(0, 0) == 0xE220A839
    assert lm.draw(0x9E3779B97F4A7C15 ^ 0xA0761D6478BD642F, 1) == 0x6E789E6A
    # the loss and the disturbance under one key do not draw the same sequence
    w = actions.ctrl_noise_numpy(np.uint64(lm.SEED64), np.arange(1, 1000, dtype=np.uint64))
    r = actions.ctrl_loss_numpy(np.uint64(lm.SEED64), np.arange(1, 1000, dtype=np.uint64))
    assert ((w * 2.0 ** 31).astype(np.int64).astype(np.uint32) != r).all()


# ---- 2. the conversion ---------------------------------------------------------------------------------------------------------------------
def test_threshold_conversion_at_the_ends_and_beyond():
    from gymwipe_amd import actions
    t = actions.ctrl_loss_threshold([0.0, 1.0, 0.5, 2.0 ** -32, -0.25, 1.5, float("inf"), float("-inf"), float("nan"), 0.25, 1.0 - 2.0 ** -33,
                                     2.0 ** -33])
    assert t.dtype == np.uint32
    assert t.tolist() == [0, 0xFFFFFFFF, 0x80000000, 1, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0, 0x40000000, 0xFFFFFFFF, 0]
    assert actions.ctrl_loss_threshold(np.full((3, 4), 0.5)).shape == (3, 4) and actions.ctrl_loss_threshold(0.5).shape == ()
    assert [lm.threshold(p) for p in (0.0, 1.0, 0.5, 2.0 ** -32, 0.3)] == actions.ctrl_loss_threshold([0.0, 1.0, 0.5, 2.0 ** -32, 0.3]).tolist()


def test_make_ctrl_loss_lays_sets_and_keys_as_the_disturbance_helper_does():
    from gymwipe_amd import actions
    thr, key = actions.make_ctrl_loss(lm.P_SETS, pm.N_FUSED, seed=lm.SEED, envs_per_set=pm.PER_SET)
    assert thr.shape == (512, 4) and thr.dtype == np.uint32 and key.shape == (512,) and key.dtype == np.uint64
    assert (thr == lm.thr_array()[pm.fused_layout()[1]]).all()
    assert key.tolist() == [cd.key_of(lm.SEED64, e) for e in range(512)]
    p, gi, b, _ = pm.fused_layout()                                             # the fused fixture's keys through the helper
    assert (actions.make_ctrl_loss(np.zeros(4), 512, seed=lm.SEED, streams=(p * lm.G + gi) * 2 + b)[1] == ct.fused_keys(lm.SEED64)).all()
    thr, key = actions.make_ctrl_loss((0.5, 0.0, 1.0, 0.25), 6)
    assert (thr == [0x80000000, 0, 0xFFFFFFFF, 0x40000000]).all()
    _, dkey = actions.make_ctrl_disturbance(np.zeros(4), 6)
    assert key.tolist() == [cd.key_of(actions.CTRL_LOSS_DEFAULT_SEED, e) for e in range(6)] and (key != dkey).all()
    _, key = actions.make_ctrl_loss(np.zeros(4), 512, seed=9, streams=np.arange(512) % 128)      # common random numbers
    assert (key.reshape(4, 128) == key[:128]).all() and len(set(key[:128].tolist())) == 128
    for bad in (lambda: actions.make_ctrl_loss(lm.P_SETS, 100), lambda: actions.make_ctrl_loss([(0.5, 0.0, 0.0)], 8),
                lambda: actions.make_ctrl_loss(np.zeros(4), 8, streams=np.arange(7))):
        with pytest.raises(ValueError):
            bad()


# ---- 3. the model at zero thresholds ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plant", [None, "dense"])
def test_zero_thresholds_give_the_disturbance_model_field_for_field(plant):
    K, seed, start, period = 70, 1, 20, 10
    assert lm.THR_SETS[0] == (0, 0, 0, 0)
    dev, dur, want, _ = ct.step_streams(DIST, plant, K, seed, start, period)
    dev2, dur2, got, _ = ct.step_streams(LOSS, plant, K, seed, start, period)
    assert (dev == dev2).all() and (dur == dur2).all()
    for k in range(K):
        for f, w in want[k].items():
            assert same(got[k][f][0], w[0]), (plant, k, f)
        assert (got[k]["loss_count"] == got[k]["n_tx"]).all() and (got[k]["lost"][0] == 0).all()     # the model's n_tx equals n
    assert (got[-1]["loss_count"][0] > 70).all() and (got[-1]["loss_count"][lm.ALL_LOST] == 70).all()


def test_zero_thresholds_give_the_disturbance_models_fused_references():
    zero = (0, 0, 0, 0)
    a, b = ct.schedule_streams(LOSS, lm.MAX_STEPS, thr=zero), ct.schedule_streams(DIST, cd.MAX_STEPS)
    assert same(a.tally, b.tally) and same(a.ang, b.ang) and same(a.ended, b.ended)
    for f, w in b.final.items():
        assert same(a.final[f], w), f
    assert (a.final["lost"] == 0).all() and (a.final["loss_count"] >= a.final["n_tx"].astype(np.uint64)).all()


# ---- 4. conditions on the fixtures ---------------------------------------------------------------------------------------------------------
def _fused(case):
    if case == "staged":
        r = ct.episode_streams(LOSS, lm.SHORT_MAX_STEPS)
        return r.ang, r.ended, r.final, r.envs
    if case == "schedules":
        r = ct.schedule_streams(LOSS, lm.MAX_STEPS)
        return r.ang, r.ended, r.final, r.envs
    r = ct.feedback_streams(LOSS, lm.MAX_STEPS)
    return r.rows["angle"], r.rows["ended"], r.final, r.envs


@pytest.mark.parametrize("case", ["staged", "schedules", "feedback"])
def test_fused_fixtures_lose_and_deliver_on_every_link_and_end_by_both_causes(case):
    ang, ended, final, envs = _fused(case)
    assert np.isfinite(ang).all() and np.abs(ang).max() < 2000.0, np.abs(ang).max()     # nothing the int32 observation clamps
    erased_decoded = np.sum([e.model.loss.erased_decoded for e in envs], 0)
    delivered = np.sum([e.model.loss.delivered for e in envs], 0)
    print(case, "erased though decoded", erased_decoded.tolist(), "delivered", delivered.tolist(),
          "ended by limit", int(((ended & 1) != 0).sum()), "by angle", int(((ended & 2) != 0).sum()))
    assert (erased_decoded >= 1).all() and (delivered >= 1).all()
    assert ((ended & 1) != 0).sum() >= 1 and ((ended & 2) != 0).sum() >= 1
    assert (final["loss"] == lm.thr_array()[None, :, None, :]).all() and len(set(final["loss_key"].ravel().tolist())) == 64
    assert (final["loss_count"] > final["n_tx"]).sum() >= 32                     # the count ran on across resets
    for i, env in enumerate(envs):                                              # the record counts what the model's hooks saw
        r = env.model.loss
        assert r.n == len(r.sent) and sum(r.lost) == sum(1 for p in r.sent if p.loss_erased)
    # the set with 0xFFFFFFFF on the announcements: no draw of that fixture is 0xFFFFFFFF, so every announcement is erased
    sel = final["loss_count"][:, lm.ALL_LOST]
    for p in range(lm.P):
        for b in range(2):
            key = int(final["loss_key"][p, lm.ALL_LOST, b])
            assert all(lm.draw(key, n) != 0xFFFFFFFF for n in range(int(sel[p, b]) + 8))
    assert (final["received"][:, lm.ALL_LOST] == 0).all() and (sel == lm.STEPS).all()
    assert (final["lost"][:, lm.ALL_LOST, :, :2].sum(-1) == lm.STEPS).all()


def test_failing_link_step_fixture_draws_for_transmissions_the_phy_rejected():
    from test_control_loop_edges import K, PERIOD, SEED, START
    _, _, steps, models = ct.step_streams(LOSS, None, K, SEED, START, PERIOD, layout=lm.FAILING_LAYOUT)
    rejected = sum(m.loss.rejected_draws for row in models for m in row)
    commands = sum(1 for row in models for m in row for p in m.loss.sent if p.loss_link == 3)
    print("draws on rejected transmissions", rejected, "commands sent", commands)
    assert rejected >= 1 and commands >= 1
    assert all(not p.loss_decoded for row in models for m in row for p in m.loss.sent if p.loss_link == 3)    # no command decodes
    last = steps[-1]
    assert (last["received"][..., 1] == 0).all() and (last["lost"][..., 3] > 0).any() and (last["loss_count"] == last["n_tx"]).all()


def test_step_fixture_is_bounded_and_loses_on_every_link():
    _, _, steps, models = ct.step_streams(LOSS, None, 70, 1, 20, 10)
    ang = np.array([w["ang"] for w in steps])
    assert np.isfinite(ang).all() and np.abs(ang).max() < 2000.0, np.abs(ang).max()
    last = steps[-1]
    assert (last["lost"][0] == 0).all() and (last["lost"][5] > 0).all() and (last["received"][lm.ALL_LOST] == 0).all()
    assert (last["lost"][1][:, 2:] == 0).all() and (last["lost"][2][:, :2] == 0).all()       # announcement-only, data-only


# ---- 5. the wrong rules are told apart -----------------------------------------------------------------------------------------------------
COMPARED = ("x", "u", "angle_deg", "received", "n_tx", "qlen", "loss_count", "lost")


def _differs(a, b):
    return [f for f in COMPARED if not same(a[f], b[f])]


@pytest.mark.parametrize("wrong", ["phy_only", "one_thr", "no_pop", "restart_n"])
def test_a_wrong_rule_would_be_caught(wrong):
    """Each wrong rule differs from the right one in a compared field of a fixture: ``phy_only`` on the failing-link step case
    (on the default geometry every packet decodes and it is the right rule), the others on the schedule case."""
    if wrong == "phy_only":
        from test_control_loop_edges import K, PERIOD, SEED, START
        right = ct.step_streams(LOSS, None, K, SEED, START, PERIOD, layout=lm.FAILING_LAYOUT).steps[-1]
        other = ct.step_streams(LOSS, None, K, SEED, START, PERIOD, layout=lm.FAILING_LAYOUT, mode="phy_only").steps[-1]
    else:
        right = ct.schedule_streams(LOSS, lm.MAX_STEPS).final
        kw = {"restart_loss_n": True} if wrong == "restart_n" else {"mode": wrong}
        other = ct.schedule_streams(LOSS, lm.MAX_STEPS, **kw).final
    fields = _differs(other, right)
    print(wrong, "moves", fields)
    assert fields, wrong
    assert "x" in fields or "lost" in fields or "loss_count" in fields


# ---- 6. the observed rate ---------------------------------------------------------------------------------------------------------------------
def test_observed_rate_of_one_key_over_65536_draws():
    """One key, n = 2^16 draws at p = 0.25: lost is binomial(n, p), standard deviation sqrt(n p (1 - p)) = 110.9."""
    from gymwipe_amd import actions
    n, p = 1 << 16, 0.25
    thr = int(actions.ctrl_loss_threshold(p))
    key = cd.key_of(lm.SEED64, 0)
    r = actions.ctrl_loss_numpy(np.uint64(key), np.arange(n, dtype=np.uint64))
    lost = int((r < thr).sum())
    print("lost %d of %d, expected %.0f, sd %.1f" % (lost, n, p * n, math.sqrt(n * p * (1 - p))))
    assert abs(lost - p * n) <= 5.0 * math.sqrt(n * p * (1 - p))
    rec = lm.LossRecord((thr, 0, 0, 0), key)                                     # and the model's own counter agrees on a prefix
    assert sum(rec.take(0) for _ in range(4096)) == int((r[:4096] < thr).sum()) == rec.lost[0] and rec.n == 4096


# ---- 7. what the loss does ---------------------------------------------------------------------------------------------------------------------
PREMISE_SCHEDULES = ([(0, 19), (1, 19)], [(0, 3), (1, 3)])
PREMISE_KEYS = (1, 2, 3, 4)
PREMISE_NOISE_KEY = 1


def mean_abs_angle(schedule, p, key, steps=120):
    """Time-weighted mean |angle| in degrees of the default model from 0.05 rad with u0 = 0 under gains (0.1, 0, 0), disturbance
    weights (0, 0, 0, 0.01) on one noise key, loss probabilities ``p`` on loss key ``key``."""
    m = pm.PidControlLoopModel(x0=(0.0, 0.0, 0.05, 0.0), u0=0.0, gains=(0.1, 0.0, 0.0))
    cd.disturb(m, (0.0, 0.0, 0.0, 0.01), PREMISE_NOISE_KEY)
    lm.attach(m, [lm.threshold(v) for v in p], key)
    area = elapsed = 0.0
    for k in range(steps):
        d, u = schedule[k % len(schedule)]
        before = m.sim.now
        deg = m.step(d, u)[3]["Sensor angle"]
        dt = m.sim.now - before
        area, elapsed = area + math.fabs(deg) * dt, elapsed + dt
    assert m.loss.n == len(m.world.band.log)
    return area / elapsed


def test_loss_changes_which_schedule_wins_and_the_links_are_unequal():
    """The figures README quotes, pinned to 3 significant digits as the model gives them."""
    none, half = (0.0, 0.0, 0.0, 0.0), (0.5, 0.5, 0.5, 0.5)
    calm = [mean_abs_angle(s, none, 1) for s in PREMISE_SCHEDULES]
    lossy = np.array([[mean_abs_angle(s, half, k) for k in PREMISE_KEYS] for s in PREMISE_SCHEDULES])
    ann = np.array([mean_abs_angle(PREMISE_SCHEDULES[0], (0.5, 0.5, 0.0, 0.0), k) for k in PREMISE_KEYS])
    data = np.array([mean_abs_angle(PREMISE_SCHEDULES[0], (0.0, 0.0, 0.5, 0.5), k) for k in PREMISE_KEYS])
    print("calm", ["%.3g" % v for v in calm])
    print("p = 0.5", [["%.3g" % v for v in row] for row in lossy])
    print("19/19, announcements only", ["%.3g" % v for v in ann], "mean %.3g" % ann.mean())
    print("19/19, data only", ["%.3g" % v for v in data], "mean %.3g" % data.mean())
    assert ["%.3g" % v for v in calm] == PIN_CALM, calm
    assert [["%.3g" % v for v in row] for row in lossy] == PIN_LOSSY, lossy
    assert ["%.3g" % v for v in ann] == PIN_ANN and ["%.3g" % v for v in data] == PIN_DATA, (ann, data)
    assert calm[0] < calm[1] and (lossy[0] > lossy[1]).all()                     # the ranking turns over, on every key
    assert ann.mean() > 2.0 * data.mean()                                       # the announcement links hurt most
    spread = lossy[0].max() - lossy[0].min()                                    # one candidate over four keys ...
    assert spread > abs(calm[0] - calm[1])                                      # ... against the gap the calm channel shows
    assert bits(mean_abs_angle(PREMISE_SCHEDULES[0], none, 7)) == bits(calm[0]) # at p = 0 the key does not matter


# as the model gives them: schedules 19/19 and 3/3; keys 1..4
PIN_CALM = ["0.96", "1.12"]
PIN_LOSSY = [["2.96", "2.6", "4.5", "5.12"], ["1.69", "1.96", "1.74", "1.85"]]
PIN_ANN = ["2.78", "2.53", "4.38", "2.93"]                 # mean 3.16
PIN_DATA = ["0.983", "0.992", "1.01", "0.99"]              # mean 0.993
