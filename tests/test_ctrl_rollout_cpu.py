"""
gw_ctrl_set_initial / gw_ctrl_reset / gw_ctrl_rollout / gw_ctrl_rollout_schedules, the part that needs no GPU: the refusals of
the four entry points (answered before any device call), the schedule helpers of gymwipe_amd.actions, the premise -- on the
event-driven model, the band schedule decides what the plant does, and the data tests/test_ctrl_rollout.py runs on ends episodes
by both causes and stays inside the int32 observation's range -- and the fused kernels' freedom from scratch memory.
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from gymwipe_amd import actions

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ctrl_episodes_model import EpisodicControlLoop, run_schedule
from util import private_segments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. argument refusals ------------------------------------------------------------------------------------------------------------
def test_argument_refusals_without_a_gpu(native_lib):
    from gymwipe_amd import _native as nat
    L = native_lib
    one = 16
    fake = C.c_void_p(4096)                                              # never dereferenced: validation comes first
    ep = nat.CtrlEpisodes(5, 0, 90.0)

    def rollout(env=fake, steps=4, ep=ep, ptrs=(one,) * 4, angle=one, ended=one):
        device, duration, obs, reward = ptrs
        return L.gw_ctrl_rollout(env, steps, device, duration, C.byref(ep) if ep is not None else None, obs, reward, angle, ended, None)

    def schedules(env=fake, steps=4, sched=one, P=4, Ls=8, ep=ep, tally=one):
        return L.gw_ctrl_rollout_schedules(env, steps, sched, P, Ls, C.byref(ep) if ep is not None else None, tally, None)

    assert L.gw_ctrl_set_initial(None, one, one, None, None) == nat.EINVAL and b"handle is NULL" in L.gw_last_error()
    assert L.gw_ctrl_set_initial(fake, None, one, None, None) == nat.EINVAL and b"x0_dev is NULL" in L.gw_last_error()
    assert L.gw_ctrl_reset(None, None, None, None) == nat.EINVAL and b"handle is NULL" in L.gw_last_error()

    assert rollout(env=None) == nat.EINVAL and b"handle is NULL" in L.gw_last_error()
    assert rollout(steps=-1) == nat.EINVAL and b"steps" in L.gw_last_error()
    assert rollout(ep=nat.CtrlEpisodes(-1, 0, 0.0)) == nat.EINVAL and b"max_steps" in L.gw_last_error()
    for hole in range(4):                                                # device, duration, obs, reward in turn
        ptrs = (one,) * hole + (None,) + (one,) * (3 - hole)
        assert rollout(ptrs=ptrs) == nat.EINVAL and b"NULL" in L.gw_last_error(), hole
        assert rollout(ptrs=ptrs, steps=0) == nat.EINVAL, hole           # (before steps == 0 is looked at)
    assert rollout(ended=None) == nat.EINVAL and b"ended_dev" in L.gw_last_error()        # required with episodes ...
    assert rollout(ended=None, ep=None, steps=0) == nat.OK                                # ... and only with them
    assert rollout(steps=0) == nat.OK and rollout(steps=0, angle=None) == nat.OK
    assert rollout(steps=0, ep=nat.CtrlEpisodes(0, 0, 0.0)) == nat.OK and rollout(steps=0, ep=nat.CtrlEpisodes(0, 0, -1.0)) == nat.OK

    assert schedules(env=None) == nat.EINVAL and b"handle is NULL" in L.gw_last_error()
    assert schedules(ep=None) == nat.EINVAL and b"ep is NULL" in L.gw_last_error()
    assert schedules(ep=None, steps=0) == nat.EINVAL
    assert schedules(sched=None) == nat.EINVAL and b"NULL" in L.gw_last_error()
    assert schedules(tally=None) == nat.EINVAL and b"NULL" in L.gw_last_error()
    assert schedules(steps=-3) == nat.EINVAL and b"steps" in L.gw_last_error()
    assert schedules(ep=nat.CtrlEpisodes(-2, 0, 0.0)) == nat.EINVAL and b"max_steps" in L.gw_last_error()
    for P in (0, -1):
        assert schedules(P=P) == nat.EINVAL and b"P must be >= 1" in L.gw_last_error(), P
        assert schedules(P=P, steps=0) == nat.EINVAL, P
    for Ls in (0, -1, 65, 1000):
        assert schedules(Ls=Ls) == nat.EINVAL and b"[1, 64]" in L.gw_last_error(), Ls
        assert schedules(Ls=Ls, steps=0) == nat.EINVAL, Ls
    for Ls in (1, 64):
        assert schedules(Ls=Ls, steps=0) == nat.OK
    # (num_envs / P not a whole multiple of 64 -> GW_EUNSUPPORTED needs a handle: tests/test_ctrl_rollout.py)
    assert C.sizeof(nat.CtrlEpisodes) == 16 and nat.CtrlEpisodes.fail_deg.offset == 8


# ---- 2. the schedule helpers ---------------------------------------------------------------------------------------------------------
def test_make_ctrl_schedules_pads_cyclically_and_the_restatement_clamps():
    s = actions.make_ctrl_schedules([[(0, 19), (1, 5), (0, 7)], [(1, 3)], [(0, 1), (1, 2)]])
    assert s.dtype == np.uint8 and s.shape == (3, 3, 2)
    assert s[0].tolist() == [[0, 19], [1, 5], [0, 7]] and s[1].tolist() == [[1, 3]] * 3 and s[2].tolist() == [[0, 1], [1, 2], [0, 1]]
    s = actions.make_ctrl_schedules([[(0, 1), (1, 2)], [(1, 9)]], L=5)
    assert s.shape == (2, 5, 2) and s[0].tolist() == [[0, 1], [1, 2], [0, 1], [1, 2], [0, 1]] and (s[1] == [1, 9]).all()
    assert actions.make_ctrl_schedules([[(0, 0)]] * 7, L=64).shape == (7, 64, 2)
    for bad in (dict(schedules=[]), dict(schedules=[[]]), dict(schedules=[[(0, 1)] * 65]), dict(schedules=[[(0, 1)]], L=0),
                dict(schedules=[[(0, 1)]], L=65), dict(schedules=[[(0, 1)] * 3], L=2), dict(schedules=[[(0, 256)]]),
                dict(schedules=[[(-1, 0)]])):
        with pytest.raises(ValueError):
            actions.make_ctrl_schedules(**bad)
    # the restatement: entry age % L of schedule e // M; device clamped to {0, 1}, duration to [0, max_duration - 1]
    raw = np.zeros((2, 4, 2), np.uint8)
    raw[0, :, 0], raw[0, :, 1] = [0, 1, 2, 255], [0, 19, 20, 255]
    raw[1, :, 0], raw[1, :, 1] = [1, 0, 7, 1], [3, 2, 100, 21]
    age = np.array([0, 1, 2, 3, 4, 5, 6, 7])
    dev, dur = actions.ctrl_schedule_numpy(raw, age, 4)                  # envs 0-3 on schedule 0, 4-7 on schedule 1
    assert dev.dtype == dur.dtype == np.int32
    assert dev.tolist() == [0, 1, 1, 1, 1, 0, 1, 1] and dur.tolist() == [0, 19, 19, 19, 3, 2, 19, 19]
    every = np.zeros((1, 1, 2), np.uint8)
    for b in range(2, 256):                                              # every byte 2 .. 255 in either place
        every[0, 0] = b, b
        dev, dur = actions.ctrl_schedule_numpy(every, [0], 1)
        assert dev.tolist() == [1] and dur.tolist() == [min(b, 19)]
        dev, dur = actions.ctrl_schedule_numpy(every, [0], 1, max_duration=7)
        assert dur.tolist() == [min(b, 6)]
    with pytest.raises(ValueError):
        actions.ctrl_schedule_numpy(raw.astype(np.int32), age, 4)


# ---- 3. the premise, pinned on the model ---------------------------------------------------------------------------------------------
def _sum_of_angles(schedule, steps=120):
    env = EpisodicControlLoop()                                          # default plant, x0 = (0, 0, 0.05, 0)
    for k in range(steps):
        env.step(*schedule[k % len(schedule)], max_steps=0, fail_deg=0.0)
    assert env.age == steps
    return env.cost


def test_the_band_schedule_decides_what_the_plant_does():
    """Sum of |angle in degrees| over 120 steps of a cyclic schedule, on the model: the digits pinned are the model's."""
    idle = _sum_of_angles([(0, 0)])
    sensor_only = _sum_of_angles([(0, 19)])
    alt5 = _sum_of_angles([(0, 5), (1, 5)])
    alt19 = _sum_of_angles([(0, 19), (1, 19)])
    print("idle %r, sensor only %r, alternating 5 %r, alternating 19 %r" % (idle, sensor_only, alt5, alt19))
    assert idle == pytest.approx(357.3865112231606, rel=1e-12)
    assert sensor_only == pytest.approx(235.64236457665595, rel=1e-12)
    assert alt5 == pytest.approx(13020.252397794644, rel=1e-12)
    assert alt19 == pytest.approx(1098448649.0640342, rel=1e-12)
    assert sensor_only < idle < alt5 < alt19


def test_the_gpu_tests_data_ends_episodes_by_both_causes_and_stays_in_range():
    import test_ctrl_rollout as g
    import test_control_loop as cl
    # test 3: random action streams, max_steps = 7, fail_deg = 90
    _, _, _, _, ang, ended, final = g.episode_streams()
    assert ((ended & 1) != 0).sum() >= 3 and ((ended & 2) != 0).sum() >= 3, ((ended & 1).sum(), (ended >> 1).sum())
    assert ((ended == 1).any() and (ended == 2).any()) and (final["age"] > 0).any()
    assert np.abs(ang).max() < 1e6
    # test 4: the schedules, max_steps = 25, fail_deg = 90
    by_limit = by_fail = 0
    for P, L in ((4, 3), (2, 64), (1, 1), (4, 1)):
        _, tally, dev, dur, _, worst = g.schedule_streams(P, L)
        by_fail += int(tally[:, :, 1].sum())
        by_limit += int((tally[:, :, 0] - tally[:, :, 1]).sum())
        assert worst < 1e6, (P, L, worst)
        assert (tally[:, :, 2] == g.SCHED_STEPS).all() and dev.min() >= 0 and dev.max() <= 1 and 0 <= dur.min() and dur.max() <= 19
    assert by_limit >= 3 and by_fail >= 3, (by_limit, by_fail)
    # tests 1, 2 and "both limits off": the streams of tests/test_control_loop.py, and fresh models of X0S stepped without episodes
    for plant, seed in ((None, 20), ("dense", 21)):
        _, _, steps = cl.model_streams(plant, 40, seed, g.START, g.PERIOD)
        assert max(np.abs(w["ang"]).max() for w in steps) < 1e6
    dev, dur, _ = cl.model_streams(None, 40, 20, g.START, g.PERIOD)
    for s in range(g.STREAMS):
        env = g.wrapper(s)
        assert max(abs(env.step(dev[k, s], dur[k, s], episodes=False)[2]) for k in range(10, 20)) < 1e6


def test_the_wrapper_restates_the_episode_rule():
    """age / cost / both bits / the reset to a fresh model, on a case small enough to follow."""
    env = EpisodicControlLoop(x0=(0.0, 0.0, 1.5, 0.0), u0=0.0)           # 85.9 degrees, falling
    fresh = EpisodicControlLoop(x0=(0.0, 0.0, 1.5, 0.0), u0=0.0).state()
    age, cost, seen = 0, 0.0, set()
    for k in range(12):
        _, _, deg, ended = env.step(0, 19, max_steps=3, fail_deg=90.0)
        age, cost = age + 1, cost + abs(deg)
        assert ended == (1 if age == 3 else 0) | (2 if abs(deg) > 90.0 else 0)
        seen.add(ended)
        if ended:
            assert env.last_cost == cost and env.age == 0 and env.cost == 0.0 and env.state() == fresh
            age, cost = 0, 0.0
        else:
            assert env.age == age and env.cost == cost
    assert seen - {0}, seen
    both = EpisodicControlLoop(x0=(0.0, 0.0, 1.6, 0.0), u0=0.0)          # 91.7 degrees and falling
    assert both.step(0, 19, max_steps=1, fail_deg=90.0)[3] == 3          # both bits may be set
    tally, worst, taken = run_schedule(EpisodicControlLoop(), np.array([[0, 0], [7, 200]], np.uint8), 10, 4, 0.0)
    assert tally[:3] == [2.0, 0.0, 10.0] and taken.tolist() == [[0, 0], [1, 19], [0, 0], [1, 19]] * 2 + [[0, 0], [1, 19]]


# ---- 4. no scratch -------------------------------------------------------------------------------------------------------------------
def test_the_fused_control_loop_kernels_use_no_scratch_memory_and_are_plain_functions(tmp_path):
    kernels = private_segments(tmp_path, "ctrl_rollout.hip")
    csrc = os.path.join(ROOT, "gymwipe_amd", "csrc")
    for want in ("ctrl_rollout_kernel", "ctrl_rollout_sched_kernel", "ctrl_reset_kernel", "ctrl_set_initial_kernel"):
        assert any(want in n for n in kernels), (want, sorted(kernels))
    assert all(v == 0 for v in kernels.values()), kernels
    source = open(os.path.join(csrc, "ctrl_rollout.hip")).read()
    source = re.sub(r"//[^\n]*", "", source)
    assert len(re.findall(r"__global__", source)) == len(kernels)
    assert not re.search(r"template\s*<[^>]*>\s*(?:__launch_bounds__\(\d+\)\s*)?__global__", source), "a templated kernel"
    assert not re.search(r"__global__[^;{(]*template", source)
