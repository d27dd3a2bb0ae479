"""Test infrastructure, not a test: oracle/des_model.ControlLoopModel with the controller of gw_ctrl_set_gains
(include/gymwipe_amd.h) -- the reference's ``control()`` (control/inverted_pendulum.py:46-69) on gains of the model's own -- and
the two episode wrappers whose ``reset()`` builds it.

The controller's process is a closure inside ``ControlLoopModel.__init__``, so ``PidControlLoopModel`` restates that constructor
with the one process changed (nothing is patched at import time); ``feedback``, ``step`` and ``snapshot`` are inherited.  At a
control tick -- tick ``k >= start`` with ``(k - start) % period == 0`` -- and in this order:

    e    = fabs(ang)                                              # abs(sp - angle), sp = 0
    pid  = ((kp * e) + (ki * (e + last))) + (kd * (e - last))     # Python evaluates this association, and never contracts
    last = e                                                      # also when nothing is sent
    if ang != 0.0: send (pid if ang < 0.0 else -pid) to the actuator; commands += 1

``last_err`` is 0 in a fresh model; a reset env is a fresh model with the same gains.  With gains (1, 0, 0) the model equals
``ControlLoopModel`` snapshot for snapshot (tests/test_ctrl_gains_cpu.py).

The fixtures tests/test_ctrl_gains.py runs on are defined here and qualified on the model alone in tests/test_ctrl_gains_cpu.py."""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ctrl_episodes_model import EpisodicControlLoop
from ctrl_feedback_model import FeedbackControlLoop
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


class _PidReset:
    """``reset()`` of both wrappers: a fresh PidControlLoopModel of the env's own x0 / u0 and gains.  ``keep_last``: the wrong
    reset the CPU qualification compares against -- the new model starts from the old one's last error."""
    keep_last, model = False, None

    def reset(self):
        kw = dict(self.kw)
        if self.keep_last and self.model is not None:
            kw["keep_last_err"] = self.model.last_err
        self.model = PidControlLoopModel(x0=self.x0, u0=self.u0, **kw)
        self.age, self.cost = 0, 0.0

    def state(self):
        s = EpisodicControlLoop.state(self)
        s["gains"], s["last_error"] = list(self.model.gains), self.model.last_err
        return s


class EpisodicPidLoop(_PidReset, EpisodicControlLoop):
    """``EpisodicControlLoop`` on the PID model: ``EpisodicPidLoop(x0, u0, gains=..., start=..., period=...)``."""


class FeedbackPidLoop(_PidReset, FeedbackControlLoop):
    """``FeedbackControlLoop`` on the PID model."""


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


def _g():
    import test_ctrl_rollout as g
    return g


def _rows(states):
    """test_ctrl_rollout._rows with the two f64 fields of the controller."""
    out = _g()._rows([{f: v for f, v in st.items() if f not in ("gains", "last_error")} for st in states])
    out["gains"] = np.array([st["gains"] for st in states], np.float64)
    out["last_error"] = np.array([st["last_error"] for st in states], np.float64)
    return out


def _frozen(*arrays):
    for v in arrays:
        v.setflags(write=False)


@functools.lru_cache(maxsize=None)
def step_streams(plant, K, seed, start, period, gains=GAIN_SETS):
    """test_control_loop.model_streams on the PID model: the same 8 action streams through one model per (gain set, stream).
    Returns the actions [K][8] and per step {field: [G][8]...}."""
    from test_control_loop import DENSE_CTRL, STREAMS
    rng = np.random.default_rng(seed)
    dev = rng.integers(0, 2, (K, STREAMS)).astype(np.int32)
    dur = rng.integers(0, 20, (K, STREAMS)).astype(np.int32)
    kw = {} if plant is None else {"A": DENSE_CTRL["A"].tolist(), "B": DENSE_CTRL["B"].tolist(), "x0": tuple(DENSE_CTRL["x0"]),
                                   "u0": DENSE_CTRL["u0"]}
    models = [[PidControlLoopModel(start=start, period=period, gains=gs, **kw) for _ in range(STREAMS)] for gs in gains]
    steps = []
    for k in range(K):
        fb = [[m.step(int(dev[k, s]), int(dur[k, s])) for s, m in enumerate(row)] for row in models]
        sn = [[m.snapshot() for m in row] for row in models]
        want = {"obs": np.array([[f[0] for f in r] for r in fb], np.int64),
                "rew": np.array([[np.float32(f[1]) for f in r] for r in fb], np.float32),
                "ang": np.array([[f[3]["Sensor angle"] for f in r] for r in fb], np.float64)}
        for f in ("now", "x", "u", "angle_deg", "rx_power", "gains", "last_error"):
            want[f] = np.array([[q[f] for q in r] for r in sn], np.float64)
        want["qlen"] = np.array([[q["qlen"][:2] for q in r] for r in sn], np.int64)
        want["received"] = np.array([[q["received"][1:] for q in r] for r in sn], np.int64)
        for f in ("n_tx", "commands", "substeps"):
            want[f] = np.array([[q[f] for q in r] for r in sn], np.int64)
        _frozen(*want.values())
        steps.append(want)
    _frozen(dev, dur)
    return dev, dur, steps


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


def episodic(s, gains, cls=EpisodicPidLoop, keep_last=False):
    g = _g()
    env = cls(x0=g.X0S[s], u0=g.U0S[s], start=g.START, period=g.PERIOD, gains=gains)
    env.keep_last = keep_last
    return env


def episode_actions():
    """test_ctrl_rollout.episode_streams' random actions, [K][8]."""
    g = _g()
    rng = np.random.default_rng(g.EP_SEED)
    dev = rng.integers(0, 2, (STEPS, g.STREAMS)).astype(np.int32)
    dur = rng.integers(0, 20, (STEPS, g.STREAMS)).astype(np.int32)
    return dev, dur


def run_episodes(s, gains, max_steps, keep_last=False):
    """Stream s of ``episode_actions`` through one wrapper: the rows (obs, reward, angle, ended) and the wrapper."""
    dev, dur = episode_actions()
    env = episodic(s, gains, keep_last=keep_last)
    rows = [env.step(dev[k, s], dur[k, s], max_steps, FAIL_DEG) for k in range(STEPS)]
    return rows, env


@functools.lru_cache(maxsize=None)
def episode_streams(max_steps):
    """The staged-action case's reference: every (gain set, stream).  Returns the actions [K][8], the outputs and ``ended``
    [K][G][8], and the final state {field: [G][8]...}."""
    S = _g().STREAMS
    dev, dur = episode_actions()
    obs, rew = np.empty((STEPS, G, S), np.int64), np.empty((STEPS, G, S), np.float32)
    ang, ended = np.empty((STEPS, G, S), np.float64), np.empty((STEPS, G, S), np.uint8)
    states = []
    for i, gs in enumerate(GAIN_SETS):
        for s in range(S):
            rows, env = run_episodes(s, gs, max_steps)
            for k, (o, r, a, e) in enumerate(rows):
                obs[k, i, s], rew[k, i, s], ang[k, i, s], ended[k, i, s] = o, np.float32(r), a, e
            states.append(env.state())
    final = {f: v.reshape((G, S) + v.shape[1:]) for f, v in _rows(states).items()}
    _frozen(dev, dur, obs, rew, ang, ended, *final.values())
    return dev, dur, obs, rew, ang, ended, final


def run_schedule(p, s, gains, max_steps, keep_last=False):
    """ctrl_episodes_model.run_schedule for schedule p of ``schedules_of(P, ROLLOUT_L)``, keeping every angle.  Returns the
    tally, the angles, ``ended`` per step and the wrapper."""
    from ctrl_episodes_model import MAX_DURATION
    sch = _g().schedules_of(P, ROLLOUT_L)[p]
    env = episodic(s, gains, keep_last=keep_last)
    n_ended = n_failed = 0
    cost_ended = 0.0
    ang, ended = np.empty(STEPS), np.empty(STEPS, np.uint8)
    for k in range(STEPS):
        d, u = sch[env.age % ROLLOUT_L]
        _, _, ang[k], e = env.step(min(int(d), 1), min(int(u), MAX_DURATION - 1), max_steps, FAIL_DEG)
        ended[k] = e
        if e:
            n_ended += 1
            n_failed += e >> 1
            cost_ended = cost_ended + env.last_cost
    return [float(n_ended), float(n_failed), float(STEPS), cost_ended], ang, ended, env


@functools.lru_cache(maxsize=None)
def schedule_streams(max_steps):
    """The schedule case's reference, for every (p, g, b) of ``fused_layout``.  Returns the schedules, the tally [P][G][2][4],
    the final state {field: [P][G][2]...}, and the angles and ``ended`` [K][P][G][2]."""
    sch = _g().schedules_of(P, ROLLOUT_L)
    tally = np.empty((P, G, 2, 4), np.float64)
    ang, ended = np.empty((STEPS, P, G, 2), np.float64), np.empty((STEPS, P, G, 2), np.uint8)
    states = []
    for p in range(P):
        for i, gs in enumerate(GAIN_SETS):
            for b in range(2):
                tally[p, i, b], ang[:, p, i, b], ended[:, p, i, b], env = run_schedule(p, fused_stream(p, i, b), gs, max_steps)
                states.append(env.state())
    final = {f: v.reshape((P, G, 2) + v.shape[1:]) for f, v in _rows(states).items()}
    _frozen(tally, ang, ended, *final.values())
    return sch, tally, final, ang, ended


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


@functools.lru_cache(maxsize=None)
def feedback_streams(max_steps):
    """The feedback case's reference, for every (p, g, b) of ``fused_layout``.  Returns the tally [P][G][2][8], the rows
    {field: [K][P][G][2]} and the final state {field: [P][G][2]...}."""
    import ctrl_feedback_model as fm
    sched, edg = feedback_policies()
    tally = np.empty((P, G, 2, fm.COLS), np.float64)
    rows, states = None, []
    for p in range(P):
        for i, gs in enumerate(GAIN_SETS):
            for b in range(2):
                env = episodic(fused_stream(p, i, b), gs, cls=FeedbackPidLoop)
                tally[p, i, b], r, _ = fm.run_feedback(env, sched[p], edg[p], True, STEPS, max_steps, FAIL_DEG)
                if rows is None:
                    rows = {f: np.empty((STEPS, P, G, 2), v.dtype) for f, v in r.items()}
                for f, v in r.items():
                    rows[f][:, p, i, b] = v
                states.append(env.state())
    final = {f: v.reshape((P, G, 2) + v.shape[1:]) for f, v in _rows(states).items()}
    _frozen(tally, *rows.values(), *final.values())
    return tally, rows, final
