"""Test infrastructure, not a test: episodes on top of oracle/des_model.ControlLoopModel, restating the rules of
gw_ctrl_reset / gw_ctrl_rollout / gw_ctrl_rollout_schedules (include/gymwipe_amd.h).

``EpisodicControlLoop`` holds an env's own ``x0`` / ``u0``, the running episode's ``age`` and ``cost`` and a model.  A step
steps the model, then ``age += 1`` and ``cost += fabs(deg)`` (one running f64 sum), then the env has ended if
``fail_deg > 0 and fabs(deg) > fail_deg`` (bit 1) or ``max_steps > 0 and age == max_steps`` (bit 0); on an end the model is
replaced by a FRESH one built from the same ``x0`` / ``u0`` and ``age`` / ``cost`` restart at 0.  A reset env is a freshly
constructed model: that is the whole specification of reset.
``run_schedule`` restates the schedule call: the env acts on entry ``age % L`` of its schedule, bytes clamped where they are read
(device to {0, 1}, duration to [0, max_duration - 1]), and tallies {episodes ended, of those by fail_deg, steps taken, sum of
the costs of the ended episodes}."""
import math

import numpy as np

from oracle import des_model as dm

MAX_DURATION = 20                            # envs/core.py:25
FIELDS = ("now", "x", "u", "angle_deg", "rx_power", "qlen", "received", "n_tx", "commands", "substeps")


class EpisodicControlLoop:
    def __init__(self, x0=(0.0, 0.0, 0.05, 0.0), u0=0.1, **model_kw):
        self.x0, self.u0, self.kw = tuple(float(v) for v in x0), float(u0), dict(model_kw)
        self.reset()

    def reset(self):
        self.model = dm.ControlLoopModel(x0=self.x0, u0=self.u0, **self.kw)
        self.age, self.cost = 0, 0.0

    def step(self, device, duration, max_steps=0, fail_deg=0.0, episodes=True):
        """One step; returns ``(obs, reward, angle_deg, ended)``.  ``episodes=False``: the plain step, age and cost untouched."""
        obs, rew, _, info = self.model.step(int(device), int(duration))
        deg = info["Sensor angle"]
        ended = 0
        if episodes:
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

    def state(self):
        """The model's snapshot in the layout of ``VecControlLoopEnv.get_state``, with ``age`` and ``cost``."""
        s = self.model.snapshot()
        assert s["qlen"][2] == 0
        return {"now": s["now"], "x": s["x"], "u": s["u"], "angle_deg": s["angle_deg"], "rx_power": s["rx_power"],
                "qlen": s["qlen"][:2], "received": s["received"][1:], "n_tx": s["n_tx"], "commands": s["commands"],
                "substeps": s["substeps"], "age": self.age, "cost": self.cost}


def run_schedule(env, schedule, steps, max_steps, fail_deg, max_duration=MAX_DURATION):
    """``steps`` steps of ``env`` under the cyclic ``schedule`` (uint8[L][2]); returns the tally as four floats, the
    largest |angle| met and the actions taken, int32[steps][2]."""
    schedule = np.asarray(schedule)
    assert schedule.dtype == np.uint8 and schedule.ndim == 2 and schedule.shape[1] == 2
    L = schedule.shape[0]
    n_ended = n_failed = 0
    cost_ended, worst = 0.0, 0.0
    taken = np.empty((steps, 2), np.int32)
    for k in range(steps):
        d, u = schedule[env.age % L]
        taken[k] = min(int(d), 1), min(int(u), max_duration - 1)
        _, _, deg, ended = env.step(taken[k, 0], taken[k, 1], max_steps, fail_deg)
        worst = max(worst, math.fabs(deg))
        if ended:
            n_ended += 1
            n_failed += ended >> 1
            cost_ended = cost_ended + env.last_cost
    return [float(n_ended), float(n_failed), float(steps), cost_ended], worst, taken
