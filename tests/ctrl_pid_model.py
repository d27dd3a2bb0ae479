"""Test infrastructure, not a test: oracle/des_model.ControlLoopModel with the controller of gw_ctrl_set_gains
(include/gymwipe_amd.h) -- the reference's ``control()`` (control/inverted_pendulum.py:46-69) on gains of the model's own.  The rule, the gain sets and
the fused cases' layout are stated here; tests/ctrl_tiers.py builds the references from them.

The controller's process is a closure inside ``ControlLoopModel.__init__``, so ``PidControlLoopModel`` restates that constructor
with the one process changed (nothing is patched at import time); ``feedback``, ``step`` and ``snapshot`` are inherited.  At a
control tick -- tick ``k >= start`` with ``(k - start) % period == 0`` -- and in this order:

    e    = fabs(ang)                                              # abs(sp - angle), sp = 0
    pid  = ((kp * e) + (ki * (e + last))) + (kd * (e - last))     # Python evaluates this association, and never contracts
    last = e                                                      # also when nothing is sent
    if ang != 0.0: send (pid if ang < 0.0 else -pid) to the actuator; commands += 1

``last_err`` is 0 in a fresh model; a reset env is a fresh model with the same gains.  With gains (1, 0, 0) the model equals
``ControlLoopModel`` snapshot for snapshot (tests/test_ctrl_gains_cpu.py).

The gain sets tests/test_ctrl_gains.py runs on are defined here and qualified on the model alone in tests/test_ctrl_gains_cpu.py."""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ctrl_fixtures import EP_SEED, STREAMS
from oracle import des_model as dm

DEFAULT_GAINS = (1.0, 0.0, 0.0)


class PidControlLoopModel(dm.ControlLoopModel):
    def __init__(self, positions=((0.0, 0.0), (0.0, -1.0), (0.5, 0.0)), rrm_pos=(0.0, 1.0), start=20, period=10,
                 A=None, B=None, x0=(0.0, 0.0, 0.05, 0.0), u0=0.1, counter_interval=None, gains=DEFAULT_GAINS,
                 keep_last_err=None):
        if A is None:
            A, B = dm.default_plant_matrices()
            B = [-b for b in B]
        self.world = dm.World()
        self.sim = sim = self.world.sim
        self.plant = dm.LinearPlant(A, B, x0, u0)
        self.devs = [dm.NetDevice(self.world, n, x, y) for n, (x, y) in zip(("Sensor", "Controller", "Actuator"), positions)]
        sensor, controller, actuator = self.devs
        self.angle_deg = 0.0
        self.start, self.period = start, period
        self.tick = 0
        self.n_cmd = 0
        self.interval = interval = dm.COUNTER_INTERVAL if counter_interval is None else counter_interval
        self.wake = 0.0
        self.gains = tuple(float(v) for v in gains)
        # keep_last_err: only the CPU qualification uses it -- a "reset" that wrongly keeps the controller's last error
        self.last_err = 0.0 if keep_last_err is None else float(keep_last_err)

        def sensor_proc():
            while True:
                sensor.send(dm.Blob(self.plant.x[2], 2), controller.mac_addr)
                self.plant.step()
                self.wake = sim.now + interval
                yield sim.timeout(interval)

        def controller_proc():
            k = 0
            while True:
                if k >= self.start and (k - self.start) % self.period == 0:
                    kp, ki, kd = self.gains               # read at every tick: a test may change them mid-run, as set_gains does
                    ang, last = self.angle_deg, self.last_err
                    e = math.fabs(ang)
                    pid = ((kp * e) + (ki * (e + last))) + (kd * (e - last))
                    self.last_err = e
                    if ang != 0.0:
                        controller.send(dm.Blob(pid if ang < 0.0 else -pid, 1), actuator.mac_addr)
                        self.n_cmd += 1
                k += 1
                self.tick = k
                yield sim.timeout(interval)

        def receiver(dev, on_receive):
            def loop():
                while True:
                    cmd = dm.Cmd(sim, "RECEIVE", duration=100)
                    dev.mac.net_in.trigger(cmd)
                    res = yield cmd.done
                    if res is not None:
                        on_receive(res)
            sim.process(loop())

        sim.process(sensor_proc())
        sim.process(controller_proc())
        self.got = [0, 0, 0]

        def at_controller(packet):
            self.angle_deg = math.degrees(packet.payload.value)
            self.got[1] += 1

        def at_actuator(packet):
            self.plant.u = packet.payload.value
            self.got[2] += 1
        receiver(controller, at_controller)
        receiver(actuator, at_actuator)
        idx2mac = {i: d.mac_addr for i, d in enumerate(self.devs)}
        self.rrm = dm.RrmDevice(self.world, "RRM", rrm_pos[0], rrm_pos[1], idx2mac, dm._NullInterp())

    def snapshot(self):
        s = dm.ControlLoopModel.snapshot(self)
        s["gains"], s["last_error"] = list(self.gains), self.last_err
        return s


# ---- fixtures of tests/test_ctrl_gains.py ---------------------------------------------------------------------------------------------------
# 8 gain sets: the default first (its envs must behave as an unswitched handle's), then sets in which each of the three gains
# matters; 57 / 26 / 12, the reference author's other gains, diverge within a few commands and are not among them.
GAIN_SETS = ((1.0, 0.0, 0.0), (0.1, 0.0, 0.0), (0.02, 0.005, 0.05), (0.15, 0.03, 0.2), (0.05, 0.01, 0.0), (0.1, 0.0, 0.2),
             (0.08, 0.02, 0.1), (0.03, 0.0, -0.05))
G = len(GAIN_SETS)
STEPS, MAX_STEPS, SHORT_MAX_STEPS, FAIL_DEG = 60, 25, 7, 90.0
P, N_FUSED, PER_SET = 4, 512, 16                         # the fused cases: 4 schedules x 128 envs, 16 envs per gain set in a row
ROLLOUT_L = 3                                              # the schedules of the fused cases: test_ctrl_rollout.schedules_of(4, 3)
FB_NAMES = (1, 2, 3, 4)                                    # ... and their policies: ctrl_feedback_model.FIXTURES


def gains_array():
    return np.array(GAIN_SETS, np.float64)


def fused_layout():
    """The fused cases' envs: schedule (or policy) ``p = e // 128``, gain set ``g = (e // 16) % 8`` -- a 64-env block holds four
    sets, and ``actions.make_ctrl_gains(GAIN_SETS, 512, 16)`` is this layout -- and stream ``(3 g + e % 2 + 2 p) % 8``: every gain
    set meets every stream, and a (p, g) pair meets two, so that 64 models per case stand for the 512 envs.  Returns (p, g, b,
    stream), int64[512] each, b = e % 2."""
    e = np.arange(N_FUSED)
    p, g, b = e // (N_FUSED // P), (e // PER_SET) % G, e % 2
    return p, g, b, (3 * g + b + 2 * p) % 8


def fused_stream(p, g, b):
    return (3 * g + b + 2 * p) % 8


def episode_actions():
    """test_ctrl_rollout.episode_streams' random actions, [K][8]."""
    rng = np.random.default_rng(EP_SEED)
    dev = rng.integers(0, 2, (STEPS, STREAMS)).astype(np.int32)
    dur = rng.integers(0, 20, (STEPS, STREAMS)).astype(np.int32)
    return dev, dur


@functools.lru_cache(maxsize=None)
def feedback_policies():
    """The four policies of ctrl_feedback_model.FIXTURES as one call's arrays (key |o|): sched uint8[4][4][L][2], edges
    int32[4][3].  Fixtures 1-3 have three bins; they get a fourth behind an edge no key reaches."""
    import ctrl_feedback_model as fm
    from gymwipe_amd import actions
    pols, edges = [], []
    for name in FB_NAMES:
        _, edg, bins = fm.FIXTURES[name]
        bins, edg = list(bins), list(edg)
        while len(bins) < 4:
            bins.append([(1, 19)])
            edg.append(2 ** 31 - 1)
        pols.append(bins)
        edges.append(edg)
    return actions.make_ctrl_feedback(pols, edges)
