"""
gw_ctrl_rollout_feedback, the part that needs no GPU: the refusals (answered before any device call) and the struct sizes, the
helpers of gymwipe_amd.actions, the conditions tests/test_ctrl_feedback.py rests on -- on the event-driven model its fixture
policies visit every bin, resets land in several bins, episodes end by both causes and angles stay inside the int32
observation's range -- the premise that a feedback scheduler trades airtime against time-weighted error while the per-step sum
of |angle| favours whoever takes short steps, and the new kernels' freedom from scratch memory.
"""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

from gymwipe_amd import actions

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctrl_feedback_model as fm
from util import private_segments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. argument refusals ------------------------------------------------------------------------------------------------------------
def test_argument_refusals_without_a_gpu(native_lib):
    from gymwipe_amd import _native as nat
    L = native_lib
    one = 16
    fake = C.c_void_p(4096)                                              # never dereferenced: validation comes first
    good_ep = nat.CtrlEpisodes(5, 0, 90.0)
    all_rows = dict(device_out_dev=one, duration_out_dev=one, obs_dev=one, reward_dev=one, angle_deg_dev=one, ended_dev=one)

    def call(env=fake, steps=4, P=4, B=3, Ls=8, flags=1, edges=one, sched=one, ep=good_ep, rows=None, tally=one, fb=True):
        f = nat.CtrlFeedback(P, B, Ls, flags, edges, sched)
        r = nat.CtrlFeedbackRows(**rows) if rows is not None else None
        return L.gw_ctrl_rollout_feedback(env, steps, C.byref(f) if fb else None, C.byref(ep) if ep is not None else None,
                                          C.byref(r) if r is not None else None, tally, None)

    def refused(what, **kw):
        """GW_EINVAL with `what` in the message, and the same with steps == 0: refusals come before it is looked at."""
        assert call(**kw) == nat.EINVAL and what in L.gw_last_error(), (kw, L.gw_last_error())
        if "steps" not in kw:
            assert call(steps=0, **kw) == nat.EINVAL, kw
        return True

    assert refused(b"handle is NULL", env=None)
    assert refused(b"fb is NULL", fb=False)
    assert refused(b"ep is NULL", ep=None)
    assert refused(b"NULL", tally=None)
    assert refused(b"NULL", sched=None)
    assert refused(b"edges_dev", edges=None) and refused(b"edges_dev", edges=None, B=2)
    assert refused(b"steps", steps=-1) and refused(b"steps", steps=-(2 ** 31))
    assert refused(b"max_steps", ep=nat.CtrlEpisodes(-1, 0, 0.0))
    for P in (0, -1):
        assert refused(b"P must be >= 1", P=P), P
    for B in (0, -1, 9, 1000):
        assert refused(b"[1, 8]", B=B), B
    for Ls in (0, -1, 65, 1000):
        assert refused(b"[1, 64]", Ls=Ls), Ls
    for hole in ("device_out_dev", "duration_out_dev", "obs_dev", "reward_dev", "ended_dev"):
        assert refused(b"rows", rows=dict(all_rows, **{hole: None})), hole
    # what is allowed: B == 1 without edges, rows without the angle, either key, both limits off; steps == 0 reads no handle
    assert call(steps=0) == nat.OK and call(steps=0, rows=all_rows) == nat.OK
    assert call(steps=0, B=1, edges=None) == nat.OK and call(steps=0, rows=dict(all_rows, angle_deg_dev=None)) == nat.OK
    assert call(steps=0, flags=0) == nat.OK and call(steps=0, ep=nat.CtrlEpisodes(0, 0, -1.0)) == nat.OK
    for B, Ls in ((1, 1), (8, 64), (1, 64), (8, 1)):
        assert call(steps=0, B=B, Ls=Ls) == nat.OK, (B, Ls)
    # (num_envs / P not a whole multiple of 64 -> GW_EUNSUPPORTED needs a handle: tests/test_ctrl_feedback.py)
    assert C.sizeof(nat.CtrlFeedback) == 32 and nat.CtrlFeedback.edges_dev.offset == 16 and nat.CtrlFeedback.sched_dev.offset == 24
    assert C.sizeof(nat.CtrlFeedbackRows) == 48 and nat.CtrlFeedbackRows.ended_dev.offset == 40
    assert (nat.CTRL_FB_MAX_BINS, nat.CTRL_FB_COLS, nat.CTRL_FB_ABS) == (8, 8, 1)
    assert (actions.CTRL_FB_MAX_BINS, actions.CTRL_FB_COLS) == (8, 8)


# ---- 2. the helpers ------------------------------------------------------------------------------------------------------------------
def test_make_ctrl_feedback_pads_as_the_schedules_do():
    sched, edges = actions.make_ctrl_feedback([[[(0, 0)], [(0, 19), (1, 5), (0, 7)]], [[(1, 3), (0, 2)], [(1, 9)]]], [[4], [-7]])
    assert sched.dtype == np.uint8 and sched.shape == (2, 2, 3, 2) and edges.dtype == np.int32 and edges.shape == (2, 1)
    assert sched[0, 0].tolist() == [[0, 0]] * 3 and sched[0, 1].tolist() == [[0, 19], [1, 5], [0, 7]]
    assert sched[1, 0].tolist() == [[1, 3], [0, 2], [1, 3]] and sched[1, 1].tolist() == [[1, 9]] * 3
    assert edges.tolist() == [[4], [-7]]
    for p in range(2):                                                   # each policy is make_ctrl_schedules of its bins
        assert (sched[p] == actions.make_ctrl_schedules([[[(0, 0)], [(0, 19), (1, 5), (0, 7)]], [[(1, 3), (0, 2)], [(1, 9)]]][p], 3)).all()
    sched, edges = actions.make_ctrl_feedback([[[(0, 1), (1, 2)]]], [[]], L=5)           # B == 1: no edges
    assert sched.shape == (1, 1, 5, 2) and edges.shape == (1, 0) and sched[0, 0].tolist() == [[0, 1], [1, 2], [0, 1], [1, 2], [0, 1]]
    sched, edges = actions.make_ctrl_feedback([[[(0, 0)]] * 8] * 3, [[5, -5, 2 ** 31 - 1, -2 ** 31, 0, 1, 2]] * 3, L=64)
    assert sched.shape == (3, 8, 64, 2) and edges.shape == (3, 7) and edges[0, 2] == 2 ** 31 - 1 and edges[0, 3] == -2 ** 31
    one = [[(0, 1)]]
    for bad in (dict(policies=[], edges=[]), dict(policies=[[]], edges=[[]]), dict(policies=[[[]]], edges=[[]]),
                dict(policies=[one * 9], edges=[[0] * 8]), dict(policies=[one * 2, one * 3], edges=[[0], [0, 1]]),
                dict(policies=[one * 2], edges=[[]]), dict(policies=[one * 2], edges=[[0, 1]]), dict(policies=[one * 2], edges=[[0], [1]]),
                dict(policies=[one], edges=[[]], L=0), dict(policies=[one], edges=[[]], L=65), dict(policies=[[[(0, 1)] * 3]], edges=[[]], L=2),
                dict(policies=[[[(0, 256)]]], edges=[[]]), dict(policies=[[[(-1, 0)]]], edges=[[]]), dict(policies=[one * 2], edges=[[2 ** 31]])):
        with pytest.raises(ValueError):
            actions.make_ctrl_feedback(**bad)


def test_ctrl_feedback_numpy_restates_rules_one_to_three():
    rad = math.pi / 180.0
    # two policies of three bins over L = 4, two envs each; bytes outside the action space in policy 1
    sched = np.zeros((2, 3, 4, 2), np.uint8)
    for b in range(3):
        for j in range(4):
            sched[0, b, j] = b % 2, 4 * b + j                            # durations 0 .. 11 name (bin, entry)
            sched[1, b, j] = 2 + b, 18 + 4 * b + j                       # devices 2 .. 4, durations 18 .. 29
    edges = np.array([[3, 30], [30, 3]], np.int32)                       # sorted, and the same edges unsorted
    angle = np.array([2.5, -45.5, 29.5, -3.5]) * rad
    age = np.array([0, 5, 2, 7])
    dev, dur, bins = actions.ctrl_feedback_numpy(sched, edges, angle, age, 2, True)
    assert dev.dtype == dur.dtype == bins.dtype == np.int32
    assert bins.tolist() == [0, 2, 1, 1]                                 # |o| = 2, 45, 29, 3: unsorted edges count the same
    assert dev.tolist() == [0, 0, 1, 1] and dur.tolist() == [0, 9, 19, 19]
    dev, dur, bins = actions.ctrl_feedback_numpy(sched, edges, angle, age, 2, False)     # signed: o = 2, -45, 29, -3
    assert bins.tolist() == [0, 0, 1, 0] and dur.tolist() == [0, 1, 19, 19]
    assert actions.ctrl_feedback_numpy(sched, edges, angle, age, 4, True)[2].tolist() == [0, 2, 1, 1]    # one policy's envs: the other's unread
    assert actions.ctrl_feedback_numpy(sched, edges, angle, age, 2, True, max_duration=7)[1].tolist() == [0, 6, 6, 6]
    # an edge counts when it is at or below the key, and the observation truncates toward zero
    e1 = np.array([[1]], np.int32)
    s1 = actions.make_ctrl_feedback([[[(0, 1)], [(0, 2)]]], [[1]])[0]
    for deg, want_abs, want_signed in ((0.999, 0, 0), (1.0, 1, 1), (1.999, 1, 1), (-0.999, 0, 0), (-1.0, 1, 0), (-1.999, 1, 0)):
        got = [actions.ctrl_feedback_numpy(s1, e1, [math.radians(deg)], [0], 1, k)[2][0] for k in (True, False)]
        assert got == [want_abs, want_signed], deg
        assert [fm.bin_of([1], fm.observed_key(math.radians(deg), k)) for k in (True, False)] == got, deg
    # every byte 2 .. 255 in either place
    every = np.zeros((1, 1, 1, 2), np.uint8)
    none = np.zeros((1, 0), np.int32)
    for b in range(2, 256):
        every[0, 0, 0] = b, b
        dev, dur, bins = actions.ctrl_feedback_numpy(every, none, [0.3], [0], 1, True)
        assert dev.tolist() == [1] and dur.tolist() == [min(b, 19)] and bins.tolist() == [0]
        assert actions.ctrl_feedback_numpy(every, none, [0.3], [3], 1, False, max_duration=7)[1].tolist() == [min(b, 6)]
    # the key's clamp: +-1e9 degrees and beyond, the infinities and NaN
    wide = np.array([[-10 ** 9, -10 ** 9 + 1, 10 ** 9, 10 ** 9 - 1, 0, 1, 2]], np.int32)
    s8 = actions.make_ctrl_feedback([[[(0, b)] for b in range(8)]], wide.tolist())[0]
    huge = [1e9 * rad * 1.000001, 1e300, np.inf, -1e9 * rad * 1.000001, -1e300, -np.inf, np.nan, 0.0]
    keys = [fm.observed_key(a, False) for a in huge]
    assert keys == [10 ** 9] * 3 + [-10 ** 9] * 4 + [0]
    _, dur, bins = actions.ctrl_feedback_numpy(s8, wide, huge, [0] * 8, 8, False)
    assert bins.tolist() == [7, 7, 7, 1, 1, 1, 1, 3] and dur.tolist() == bins.tolist()
    assert bins.tolist() == [fm.bin_of(wide[0], k) for k in keys]
    _, _, bins = actions.ctrl_feedback_numpy(s8, wide, huge, [0] * 8, 8, True)           # |o| = 1e9 for all but the last
    assert bins.tolist() == [7] * 7 + [3] and [fm.observed_key(a, True) for a in huge] == [10 ** 9] * 7 + [0]
    for bad in (dict(sched=sched.astype(np.int32), edges=edges), dict(sched=sched[0], edges=edges), dict(sched=sched, edges=edges.astype(np.int64)),
                dict(sched=sched, edges=edges[:, :1])):
        with pytest.raises(ValueError):
            actions.ctrl_feedback_numpy(x_angle_rad=angle, age=age, envs_per_policy=2, abs_key=True, **bad)


def test_the_helper_and_the_model_choose_the_same_actions_on_the_fixtures():
    """gymwipe_amd.actions.ctrl_feedback_numpy against the rows the model wrapper took, at every step of every fixture."""
    import test_ctrl_rollout as g
    for name in fm.FIXTURES:
        sched, edges, abs_key = fm.fixture_arrays(name)
        _, rows, _, _ = fm.fixture_streams(name)
        for s in range(g.STREAMS):
            env = fm.wrapper(s)
            for k in range(12):
                dev, dur, b = actions.ctrl_feedback_numpy(sched[None], edges[None], [env.model.plant.x[2]], [env.age], 1, abs_key)
                assert (dev[0], dur[0], b[0]) == (rows["device"][k, s], rows["duration"][k, s], rows["bin"][k, s]), (name, s, k)
                env.step(dev[0], dur[0], fm.MAX_STEPS, fm.FAIL_DEG)


# ---- 3. the conditions the GPU tests rest on, on the model alone --------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fm.FIXTURES))
def test_the_fixture_policies_visit_every_bin_and_end_episodes_by_both_causes(name):
    B = len(fm.FIXTURES[name][2])
    for abs_key, max_steps in ((None, fm.MAX_STEPS), (None, fm.SHORT_MAX_STEPS)) + (((True, fm.MAX_STEPS), (False, fm.SHORT_MAX_STEPS)) if B == 3 else ()):
        tally, rows, final, reset_bins = fm.fixture_streams(name, abs_key, max_steps)
        visits = np.bincount(rows["bin"].ravel(), minlength=B)
        by_fail, by_limit = int(((rows["ended"] & 2) != 0).sum()), int(((rows["ended"] & 1) != 0).sum())
        worst = float(np.abs(rows["angle"]).max())
        print(name, abs_key, max_steps, "visits", visits.tolist(), "resets into", np.bincount(reset_bins, minlength=B).tolist(),
              "by fail_deg", by_fail, "by the limit", by_limit, "worst", worst)
        assert worst < 1e6
        assert by_fail == int(tally[:, 1].sum()) and int(tally[:, 0].sum()) == int((rows["ended"] != 0).sum())
        assert (tally[:, 2] == fm.STEPS).all() and (tally[:, 7] == (rows["bin"] == 0).sum(0)).all()
        assert (tally[:, 4] == rows["duration"].sum(0)).all() and (tally[:, 5] > 0).all() and (tally[:, 6] > 0).all()
        assert rows["device"].min() >= 0 and rows["device"].max() <= 1 and rows["duration"].min() >= 0 and rows["duration"].max() <= 19
        if abs_key is None:                                              # the fixture under its own key: what it was made for; the
            assert by_fail >= 3 and by_limit >= 3, (by_fail, by_limit)   # other key only serves the launches of three policies
            assert (visits >= 10).all(), visits
            assert len(set(reset_bins)) >= 2, set(reset_bins)


def test_the_wrapper_reads_the_clock_before_the_reset():
    """dt of a step that ends an episode is the step's own length, although the model is a fresh one (clock 0) afterwards."""
    env = fm.FeedbackControlLoop(x0=(0.0, 0.0, 1.5, 0.0), u0=0.0)
    twin = fm.EpisodicControlLoop(x0=(0.0, 0.0, 1.5, 0.0), u0=0.0)
    clock, seen = 0.0, 0
    for k in range(9):
        out = env.step(0, 19, max_steps=3, fail_deg=90.0)
        assert out == twin.step(0, 19, max_steps=3, fail_deg=90.0) and env.state() == twin.state()
        if out[3]:
            seen += 1
            assert env.model.sim.now == 0.0 and env.last_dt > 0.019 and clock + env.last_dt > 0.019
            clock = 0.0
        else:
            assert env.last_dt == env.model.sim.now - clock
            clock = env.model.sim.now
    assert seen >= 3
    tally, rows, _ = fm.run_feedback(fm.FeedbackControlLoop(), np.array([[[0, 0], [7, 200]]], np.uint8), np.zeros(0, np.int32), True, 10, 4, 0.0)
    assert tally[:3] == [2.0, 0.0, 10.0] and tally[4] == 5 * 19.0 and tally[7] == 10.0
    assert rows["duration"].tolist() == [0, 19, 0, 19] * 2 + [0, 19] and rows["device"].tolist() == [0, 1, 0, 1] * 2 + [0, 1]
    elapsed = area = 0.0
    for k in range(10):
        elapsed, area = elapsed + rows["dt"][k], area + math.fabs(rows["angle"][k]) * rows["dt"][k]
    assert tally[5] == elapsed and tally[6] == area


# ---- 4. the premise, pinned on the model ---------------------------------------------------------------------------------------------
def _premise(policy, edges):
    """One env of the default plant with B / 57.3 from x0 = (0, 0, 0.3, 0), u0 = 0, no episode limits, under `policy` with the key
    |o|.  Returns the sum of |angle| over the first 60 steps and, over the steps it takes the clock to reach 1.2 s, the
    time-weighted mean |angle|, the duration units assigned and that number of steps."""
    from oracle import des_model as dm
    A, B = dm.default_plant_matrices()
    env = fm.FeedbackControlLoop(x0=(0.0, 0.0, 0.3, 0.0), u0=0.0, A=A, B=[-b / 57.3 for b in B])
    sched, edg = actions.make_ctrl_feedback([policy], [edges])
    tally, rows, _ = fm.run_feedback(env, sched[0], edg[0], True, 150, 0, 0.0)
    per_step = elapsed = area = 0.0
    for k in range(60):
        per_step = per_step + math.fabs(rows["angle"][k])
    n = airtime = 0
    while elapsed < 1.2:
        elapsed, area, airtime, n = elapsed + rows["dt"][n], area + math.fabs(rows["angle"][n]) * rows["dt"][n], airtime + int(rows["duration"][n]), n + 1
    return per_step, area / elapsed, airtime, n


def test_a_feedback_scheduler_trades_airtime_against_time_weighted_error():
    """Alternating sensor and controller at duration 19 against leaving the band alone while |obs| <= 1: the per-step sum of
    |angle| calls the feedback policy more than twice as good, because its idle steps are short; weighted by time the two are
    within a quarter of a percent, alternating ahead, and what feedback buys is airtime.  The digits pinned are the model's."""
    alt = _premise([[(0, 19), (1, 19)]], [])
    fb = _premise([[(0, 0)], [(0, 19), (1, 19)]], [2])
    print("alternating %r\nfeedback    %r" % (alt, fb))
    assert alt[0] == pytest.approx(519.7198122291716, rel=1e-12) and fb[0] == pytest.approx(232.41862450375064, rel=1e-12)
    assert alt[1] == pytest.approx(8.744655734908934, rel=1e-12) and fb[1] == pytest.approx(8.759183344951303, rel=1e-12)
    assert (alt[2], alt[3]) == (1121, 59) and (fb[2], fb[3]) == (1064, 115)
    assert fb[0] < alt[0] and alt[1] < fb[1]                             # the ordering flips between the two metrics
    assert fb[2] < alt[2]


# ---- 5. no scratch -------------------------------------------------------------------------------------------------------------------
def test_the_feedback_kernels_use_no_scratch_memory_and_are_plain_functions(tmp_path):
    kernels = private_segments(tmp_path, "ctrl_rollout_feedback.hip")
    csrc = os.path.join(ROOT, "gymwipe_amd", "csrc")
    variants = ("", "_pid", "_dist", "_loss")                            # default, + gains, + disturbance, + loss: all in this file
    for want in ["ctrl_rollout_fb%s%s_kernel" % (shape, v) for shape in ("", "_rows") for v in variants]:
        assert any(want in n for n in kernels), (want, sorted(kernels))
    assert len(kernels) == 2 * len(variants) and all(v == 0 for v in kernels.values()), kernels
    source = open(os.path.join(csrc, "ctrl_rollout_feedback.hip")).read()
    source = re.sub(r"//[^\n]*", "", source)
    assert len(re.findall(r"__global__", source)) == len(kernels)
    assert not re.search(r"template\s*<[^>]*>\s*(?:__launch_bounds__\(\d+\)\s*)?__global__", source), "a templated kernel"
    assert not re.search(r"__global__[^;{(]*template", source)
