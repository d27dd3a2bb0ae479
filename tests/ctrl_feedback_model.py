"""Test infrastructure, not a test: angle-feedback band schedulers on top of oracle/des_model.ControlLoopModel, restating rules
1-6 of gw_ctrl_rollout_feedback (include/gymwipe_amd.h), and the fixtures tests/test_ctrl_feedback.py runs on.

Before each step the env looks at its own pendulum: ``deg = x[2] * (180.0 / 3.141592653589793)`` of its CURRENT state (what its
last step reported, or its own ``x0`` after a reset), ``o = int32(fmin(fmax(deg, -1e9), 1e9))`` (NaN gives -1e9), the key is
``o`` or ``|o|``, the bin is the number of the policy's edges at or below the key (sorted or not), and the action is entry
``age % L`` of that bin's schedule, bytes clamped where they are read.  The step and the episode rule are
``EpisodicControlLoop``'s; ``FeedbackControlLoop`` restates its step because that one replaces the model inside the call, and the
clock BEFORE the reset is what ``dt`` needs.  The tally is eight running f64 per env in step order: the schedule call's four,
then the durations assigned, ``elapsed`` (sum of dt), ``area`` (``area + fabs(deg_k) * dt``) and the steps taken in bin 0.

The fixtures (four policies on X0S / U0S / START / PERIOD of tests/test_ctrl_rollout.py, 8 models standing for N envs) are
checked on the model alone in tests/test_ctrl_feedback_cpu.py: every bin of every policy is visited, resets land in several
bins, episodes end by both causes, and angles stay far inside the int32 observation's range."""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ctrl_episodes_model import MAX_DURATION, EpisodicControlLoop

DEG_PER_RAD = 180.0 / 3.141592653589793
COLS = 8
STEPS, MAX_STEPS, FAIL_DEG = 60, 25, 90.0
SHORT_MAX_STEPS = 7                                        # where the step limit's share of the endings matters

# name -> (abs_key, edges, one cyclic schedule per bin).  Policy 2 carries bytes outside the action space; policy 4 has four
# bins and unsorted edges.
FIXTURES = {
    1: (True, (3, 30), ([(0, 0)], [(0, 19), (1, 5)], [(0, 19), (1, 19)])),
    2: (True, (2, 8), ([(0, 19), (0, 19), (1, 3)], [(1, 19), (0, 7), (0, 19)], [(0, 0), (9, 250), (0, 19)])),
    3: (False, (-10, 10), ([(0, 19), (1, 19)], [(0, 3), (0, 0)], [(1, 19), (0, 19)])),
    4: (False, (40, -40, 0), ([(0, 5)], [(1, 5)], [(0, 19)], [(1, 19)])),
}


class FeedbackControlLoop(EpisodicControlLoop):
    """``EpisodicControlLoop`` whose step also reports ``dt``: the model's clock after the step, before any reset, minus its
    clock before the step."""

    def step(self, device, duration, max_steps=0, fail_deg=0.0):
        before = self.model.sim.now
        obs, rew, _, info = self.model.step(int(device), int(duration))
        self.last_dt = self.model.sim.now - before
        deg = info["Sensor angle"]
        ended = 0
        self.age += 1
        self.cost = self.cost + math.fabs(deg)
        if max_steps > 0 and self.age == max_steps:
            ended |= 1
        if fail_deg > 0 and math.fabs(deg) > fail_deg:
            ended |= 2
        if ended:
            self.last_cost = self.cost
            self.reset()
        return obs, rew, deg, ended


def observed_key(angle_rad, abs_key):
    """Rule 1: the int32 observation of an angle in radians, clamped at +-1e9 and defined for NaN; or its absolute value."""
    deg = angle_rad * DEG_PER_RAD
    if deg != deg:                                         # fmax(NaN, -1e9) is -1e9
        o = -10 ** 9
    else:
        o = int(min(max(deg, -1e9), 1e9))                  # int() truncates toward zero, as the cast does
    return abs(o) if abs_key else o


def bin_of(edges, key):
    """Rule 2: how many edges lie at or below the key."""
    return sum(1 for v in edges if int(v) <= key)


def run_feedback(env, sched, edges, abs_key, steps, max_steps, fail_deg, max_duration=MAX_DURATION):
    """``steps`` steps of ``env`` under one policy (``sched`` uint8[B][L][2], ``edges`` int32[B - 1]).  Returns the tally as eight
    floats, the rows {device, duration, obs, reward, angle, ended, bin, dt} and the bins in which the env stood right after a
    reset."""
    sched, edges = np.asarray(sched), np.asarray(edges)
    assert sched.dtype == np.uint8 and sched.ndim == 3 and sched.shape[2] == 2 and edges.shape == (sched.shape[0] - 1,)
    L = sched.shape[1]
    n_ended = n_failed = n_bin0 = 0
    cost_ended = airtime = elapsed = area = 0.0
    rows = {"device": np.empty(steps, np.int32), "duration": np.empty(steps, np.int32), "obs": np.empty(steps, np.int64),
            "reward": np.empty(steps, np.float32), "angle": np.empty(steps, np.float64), "ended": np.empty(steps, np.uint8),
            "bin": np.empty(steps, np.int32), "dt": np.empty(steps, np.float64)}
    reset_bins = []
    after_reset = False
    for k in range(steps):
        b = bin_of(edges, observed_key(env.model.plant.x[2], abs_key))
        if after_reset:
            reset_bins.append(b)
        n_bin0 += b == 0
        d, u = sched[b, env.age % L]
        d, u = min(int(d), 1), min(int(u), max_duration - 1)
        obs, rew, deg, ended = env.step(d, u, max_steps, fail_deg)
        dt = env.last_dt
        airtime = airtime + float(u)
        elapsed = elapsed + dt
        area = area + math.fabs(deg) * dt
        after_reset = bool(ended)
        if ended:
            n_ended += 1
            n_failed += ended >> 1
            cost_ended = cost_ended + env.last_cost
        for name, v in (("device", d), ("duration", u), ("obs", obs), ("reward", np.float32(rew)), ("angle", deg), ("ended", ended),
                        ("bin", b), ("dt", dt)):
            rows[name][k] = v
    return [float(n_ended), float(n_failed), float(steps), cost_ended, airtime, elapsed, area, float(n_bin0)], rows, reset_bins


def fixture_arrays(name, L=None):
    """Fixture ``name`` as ``(sched uint8[B][L][2], edges int32[B - 1], abs_key)``."""
    from gymwipe_amd import actions
    abs_key, edges, bins = FIXTURES[name]
    sched, edg = actions.make_ctrl_feedback([list(bins)], [list(edges)], L)
    return sched[0], edg[0], abs_key


def wrapper(s, **kw):
    import ctrl_fixtures as g
    return FeedbackControlLoop(x0=g.X0S[s], u0=g.U0S[s], start=g.START, period=g.PERIOD, **kw)


def fixture_streams(name, abs_key=None, max_steps=MAX_STEPS, steps=STEPS):
    """The reference: fixture ``name`` on each of the 8 streams (``abs_key`` None: the fixture's own key).  Returns the tally
    [8][8], the rows {field: [K][8]}, the states after the last step {field: [8]...} and the bins resets landed in.  Computed
    once, never modified."""
    return _fixture_streams(name, FIXTURES[name][0] if abs_key is None else bool(abs_key), max_steps, steps)


@functools.lru_cache(maxsize=None)
def _fixture_streams(name, key, max_steps, steps):
    import ctrl_fixtures as g
    sched, edges, _ = fixture_arrays(name)
    tally = np.empty((g.STREAMS, COLS), np.float64)
    rows, states, reset_bins = None, [], []
    for s in range(g.STREAMS):
        env = wrapper(s)
        tally[s], r, rb = run_feedback(env, sched, edges, key, steps, max_steps, FAIL_DEG)
        if rows is None:
            rows = {f: np.empty((steps, g.STREAMS), v.dtype) for f, v in r.items()}
        for f, v in r.items():
            rows[f][:, s] = v
        states.append(env.state())
        reset_bins += rb
    final = g.rows_of(states)
    for v in (tally,) + tuple(rows.values()) + tuple(final.values()):
        v.setflags(write=False)
    return tally, rows, final, tuple(reset_bins)
