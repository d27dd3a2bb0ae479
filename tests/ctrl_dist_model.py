"""Test infrastructure, not a test: the control-loop model with the plant of gw_ctrl_set_disturbance (include/gymwipe_amd.h) --
``oracle/des_model.LinearPlant`` whose substep ends with one draw of counter-based noise -- and the two episode wrappers whose
``reset()`` hands the old plant's record to the fresh model.

``DisturbedPlant.step()`` runs the parent's substep ``nx = A x + B u`` and then, in pure Python integers and floats:

    z  = key ^ (n * 0xD1B54A32D192ED03)                       (mod 2^64)
    z += 0x9E3779B97F4A7C15
    z  = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
    z  = (z ^ (z >> 27)) * 0x94D049BB133111EB
    z ^= z >> 31
    w  = (signed 32-bit reading of z >> 32) * 2^-31            every operation exact
    x[i] = nx[i] + g[i] * w                                    Python rounds the product, then the sum
    n += 1

``disturb(model, g, key, n)`` assigns such a plant to ``model.plant`` of a built ``PidControlLoopModel``: the sensor's process, the
actuator's delivery and the snapshot all look the attribute up when they run.  A reset env is a fresh model whose plant goes on
drawing where the old one stopped: ``g``, ``key`` and ``n`` survive, everything else is new.  ``restart_n`` is the wrong reset
the CPU qualification compares against.

The fixtures tests/test_ctrl_disturbance.py runs on are defined here and qualified on the model alone in
tests/test_ctrl_disturbance_cpu.py."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctrl_pid_model as pm
from ctrl_episodes_model import EpisodicControlLoop
from ctrl_feedback_model import FeedbackControlLoop
from oracle import des_model as dm

M64 = (1 << 64) - 1
STREAM_STEP = 0x9E3779B97F4A7C15


def noise(key, n):
    """The rule's ``w`` for one key and count, Python integers throughout."""
    z = (key ^ ((n * 0xD1B54A32D192ED03) & M64)) & M64
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    top = z >> 32
    return float(top - (1 << 32) if top >= (1 << 31) else top) * 2.0 ** -31


def key_of(seed, stream):
    """``actions.make_ctrl_disturbance``'s key of one stream number, restated."""
    return (int(seed) ^ ((int(stream) * STREAM_STEP) & M64)) & M64


class DisturbedPlant(dm.LinearPlant):
    def __init__(self, A, B, x0, u0, g=(0.0, 0.0, 0.0, 0.0), key=0, n=0):
        dm.LinearPlant.__init__(self, A, B, x0, u0)
        self.g, self.key, self.n = tuple(float(v) for v in g), int(key), int(n)

    def step(self):
        dm.LinearPlant.step(self)                          # nx = A x + B u, substeps += 1
        w = noise(self.key, self.n)
        self.x = [self.x[i] + self.g[i] * w for i in range(4)]
        self.n += 1


def disturb(model, g, key, n=0):
    """Replace the plant of a built model by a disturbed one in the same state; returns the model."""
    old = model.plant
    model.plant = DisturbedPlant(old.A, old.B, old.x, old.u, g, key, n)
    model.plant.substeps = old.substeps
    return model


def snapshot_of(model):
    s = model.snapshot()
    s["disturbance"], s["noise_key"], s["noise_count"] = list(model.plant.g), model.plant.key, model.plant.n
    return s


class _DistReset(pm._PidReset):
    """``reset()`` of both wrappers: a fresh PidControlLoopModel of the env's own x0 / u0 and gains, disturbed by the env's own
    ``g`` and ``key`` from the count the old plant had reached.  ``restart_n``: the wrong reset -- every episode replays the
    sequence from 0."""

    def __init__(self, x0=(0.0, 0.0, 0.05, 0.0), u0=0.1, g=(0.0, 0.0, 0.0, 0.0), key=0, restart_n=False, **model_kw):
        self.g, self.key, self.restart_n = tuple(float(v) for v in g), int(key), restart_n
        super().__init__(x0=x0, u0=u0, **model_kw)

    def reset(self):
        n = 0 if self.model is None or self.restart_n else self.model.plant.n
        pm._PidReset.reset(self)
        disturb(self.model, self.g, self.key, n)

    def state(self):
        s = pm._PidReset.state(self)
        s["disturbance"], s["noise_key"], s["noise_count"] = list(self.model.plant.g), self.model.plant.key, self.model.plant.n
        return s


class EpisodicDistLoop(_DistReset, EpisodicControlLoop):
    """``EpisodicControlLoop`` on the disturbed PID model: ``EpisodicDistLoop(x0, u0, g=, key=, gains=, start=, period=)``."""


class FeedbackDistLoop(_DistReset, FeedbackControlLoop):
    """``FeedbackControlLoop`` on the disturbed PID model."""


# ---- fixtures of tests/test_ctrl_disturbance.py ---------------------------------------------------------------------------------------------
# 8 weight sets: none first (its envs must walk the undisturbed trajectory), each plant state alone, then mixtures of both
# signs.  Set i runs under pm.GAIN_SETS[i]: the disturbance instantiations are PID instantiations, and both rules are exercised.
G_SETS = ((0.0, 0.0, 0.0, 0.0), (0.01, 0.0, 0.0, 0.0), (0.0, 0.01, 0.0, 0.0), (0.0, 0.0, 0.002, 0.0), (0.0, 0.0, 0.0, 0.01),
          (0.001, 0.002, 0.0005, 0.01), (0.0, 0.0, 0.0, 0.05), (-0.002, 0.0, 0.001, -0.02))
G = len(G_SETS)
assert G == pm.G
SEED = 0xC0FFEE0DDF00D5EED                                   # wider than 64 bits: the helper takes its low 64
SEED64 = SEED & M64
STEPS, MAX_STEPS, SHORT_MAX_STEPS, FAIL_DEG = pm.STEPS, pm.MAX_STEPS, pm.SHORT_MAX_STEPS, pm.FAIL_DEG
P, N_FUSED, PER_SET = pm.P, pm.N_FUSED, pm.PER_SET


def g_array():
    return np.array(G_SETS, np.float64)


def _rows(states):
    """ctrl_pid_model._rows with the three fields of the disturbance."""
    out = pm._rows([{f: v for f, v in st.items() if f not in ("disturbance", "noise_key", "noise_count")} for st in states])
    out["disturbance"] = np.array([st["disturbance"] for st in states], np.float64)
    out["noise_key"] = np.array([st["noise_key"] for st in states], np.uint64)
    out["noise_count"] = np.array([st["noise_count"] for st in states], np.uint64)
    return out


def step_noise_stream(gi, s):
    """The step cases' noise stream number of (weight set, action stream): one per pair, so that 64 models stand for N envs."""
    return int(gi) * 8 + int(s)


def step_model(plant, start, period, gi, s, g=None):
    from test_control_loop import DENSE_CTRL
    kw = {} if plant is None else {"A": DENSE_CTRL["A"].tolist(), "B": DENSE_CTRL["B"].tolist(), "x0": tuple(DENSE_CTRL["x0"]),
                                   "u0": DENSE_CTRL["u0"]}
    m = pm.PidControlLoopModel(start=start, period=period, gains=pm.GAIN_SETS[gi], **kw)
    return disturb(m, G_SETS[gi] if g is None else g, key_of(SEED64, step_noise_stream(gi, s)))


@functools.lru_cache(maxsize=None)
def step_streams(plant, K, seed, start, period):
    """ctrl_pid_model.step_streams on the disturbed model: the same 8 action streams through one model per (weight set, stream).
    Returns the actions [K][8] and per step {field: [G][8]...}."""
    from test_control_loop import STREAMS
    rng = np.random.default_rng(seed)
    dev = rng.integers(0, 2, (K, STREAMS)).astype(np.int32)
    dur = rng.integers(0, 20, (K, STREAMS)).astype(np.int32)
    models = [[step_model(plant, start, period, gi, s) for s in range(STREAMS)] for gi in range(G)]
    steps = []
    for k in range(K):
        fb = [[m.step(int(dev[k, s]), int(dur[k, s])) for s, m in enumerate(row)] for row in models]
        sn = [[snapshot_of(m) for m in row] for row in models]
        want = {"obs": np.array([[f[0] for f in r] for r in fb], np.int64),
                "rew": np.array([[np.float32(f[1]) for f in r] for r in fb], np.float32),
                "ang": np.array([[f[3]["Sensor angle"] for f in r] for r in fb], np.float64)}
        for f in ("now", "x", "u", "angle_deg", "rx_power", "gains", "last_error", "disturbance"):
            want[f] = np.array([[q[f] for q in r] for r in sn], np.float64)
        want["qlen"] = np.array([[q["qlen"][:2] for q in r] for r in sn], np.int64)
        want["received"] = np.array([[q["received"][1:] for q in r] for r in sn], np.int64)
        for f in ("n_tx", "commands", "substeps"):
            want[f] = np.array([[q[f] for q in r] for r in sn], np.int64)
        for f in ("noise_key", "noise_count"):
            want[f] = np.array([[q[f] for q in r] for r in sn], np.uint64)
        pm._frozen(*want.values())
        steps.append(want)
    pm._frozen(dev, dur)
    return dev, dur, steps


def fused_noise_stream(p, g, b):
    """The fused cases' noise stream number of (schedule or policy, weight set, b): one per model."""
    return (p * G + g) * 2 + b


def fused_keys():
    """uint64[512]: the key of every env of ``pm.fused_layout``."""
    p, g, b, _ = pm.fused_layout()
    return np.array([key_of(SEED64, fused_noise_stream(int(p[e]), int(g[e]), int(b[e]))) for e in range(N_FUSED)], np.uint64)


def episodic(p, gi, b, cls=EpisodicDistLoop, restart_n=False, g=None):
    """The wrapper of fused model (p, gi, b): action stream ``pm.fused_stream``'s X0S / U0S, gains and weights of set gi."""
    t = pm._g()
    s = pm.fused_stream(p, gi, b)
    return cls(x0=t.X0S[s], u0=t.U0S[s], g=G_SETS[gi] if g is None else g, key=key_of(SEED64, fused_noise_stream(p, gi, b)),
               restart_n=restart_n, start=t.START, period=t.PERIOD, gains=pm.GAIN_SETS[gi])


def run_episodes(p, gi, b, max_steps, restart_n=False):
    """Stream ``pm.fused_stream(p, gi, b)`` of ``pm.episode_actions`` through model (p, gi, b): the rows and the wrapper."""
    dev, dur = pm.episode_actions()
    s = pm.fused_stream(p, gi, b)
    env = episodic(p, gi, b, restart_n=restart_n)
    rows = [env.step(dev[k, s], dur[k, s], max_steps, FAIL_DEG) for k in range(STEPS)]
    return rows, env


@functools.lru_cache(maxsize=None)
def episode_streams(max_steps):
    """The staged-action case's reference, for every (p, g, b) of ``pm.fused_layout``.  Returns the outputs and ``ended``
    [K][P][G][2] and the final state {field: [P][G][2]...}."""
    shape = (STEPS, P, G, 2)
    obs, rew = np.empty(shape, np.int64), np.empty(shape, np.float32)
    ang, ended = np.empty(shape, np.float64), np.empty(shape, np.uint8)
    states = []
    for p in range(P):
        for i in range(G):
            for b in range(2):
                rows, env = run_episodes(p, i, b, max_steps)
                for k, (o, r, a, e) in enumerate(rows):
                    obs[k, p, i, b], rew[k, p, i, b], ang[k, p, i, b], ended[k, p, i, b] = o, np.float32(r), a, e
                states.append(env.state())
    final = {f: v.reshape((P, G, 2) + v.shape[1:]) for f, v in _rows(states).items()}
    pm._frozen(obs, rew, ang, ended, *final.values())
    return obs, rew, ang, ended, final


def run_schedule(p, gi, b, max_steps, restart_n=False, g=None):
    """ctrl_pid_model.run_schedule on model (p, gi, b).  Returns the tally, the angles, ``ended`` per step and the wrapper."""
    from ctrl_episodes_model import MAX_DURATION
    sch = pm._g().schedules_of(P, pm.ROLLOUT_L)[p]
    env = episodic(p, gi, b, restart_n=restart_n, g=g)
    n_ended = n_failed = 0
    cost_ended = 0.0
    ang, ended = np.empty(STEPS), np.empty(STEPS, np.uint8)
    for k in range(STEPS):
        d, u = sch[env.age % pm.ROLLOUT_L]
        _, _, ang[k], e = env.step(min(int(d), 1), min(int(u), MAX_DURATION - 1), max_steps, FAIL_DEG)
        ended[k] = e
        if e:
            n_ended += 1
            n_failed += e >> 1
            cost_ended = cost_ended + env.last_cost
    return [float(n_ended), float(n_failed), float(STEPS), cost_ended], ang, ended, env


@functools.lru_cache(maxsize=None)
def schedule_streams(max_steps):
    """The schedule case's reference.  Returns the schedules, the tally [P][G][2][4], the final state {field: [P][G][2]...},
    and the angles and ``ended`` [K][P][G][2]."""
    sch = pm._g().schedules_of(P, pm.ROLLOUT_L)
    tally = np.empty((P, G, 2, 4), np.float64)
    ang, ended = np.empty((STEPS, P, G, 2), np.float64), np.empty((STEPS, P, G, 2), np.uint8)
    states = []
    for p in range(P):
        for i in range(G):
            for b in range(2):
                tally[p, i, b], ang[:, p, i, b], ended[:, p, i, b], env = run_schedule(p, i, b, max_steps)
                states.append(env.state())
    final = {f: v.reshape((P, G, 2) + v.shape[1:]) for f, v in _rows(states).items()}
    pm._frozen(tally, ang, ended, *final.values())
    return sch, tally, final, ang, ended


@functools.lru_cache(maxsize=None)
def feedback_streams(max_steps, disturbed=True):
    """The feedback case's reference (``pm.feedback_policies``, key |o|).  Returns the tally [P][G][2][8], the rows
    {field: [K][P][G][2]} and the final state {field: [P][G][2]...}.  ``disturbed=False``: the same models with all weights 0,
    for the qualification."""
    import ctrl_feedback_model as fm
    sched, edg = pm.feedback_policies()
    tally = np.empty((P, G, 2, fm.COLS), np.float64)
    rows, states = None, []
    for p in range(P):
        for i in range(G):
            for b in range(2):
                env = episodic(p, i, b, cls=FeedbackDistLoop, g=None if disturbed else (0.0, 0.0, 0.0, 0.0))
                tally[p, i, b], r, _ = fm.run_feedback(env, sched[p], edg[p], True, STEPS, max_steps, FAIL_DEG)
                if rows is None:
                    rows = {f: np.empty((STEPS, P, G, 2), v.dtype) for f, v in r.items()}
                for f, v in r.items():
                    rows[f][:, p, i, b] = v
                states.append(env.state())
    final = {f: v.reshape((P, G, 2) + v.shape[1:]) for f, v in _rows(states).items()}
    pm._frozen(tally, *rows.values(), *final.values())
    return tally, rows, final
