"""Test infrastructure, not a test: the control loop's variants as tiers, and the one copy of the machinery that turns a tier's
model into the references the GPU tests run on.

A variant is a prefix of the blocks (gains, disturbance, loss), as ``GwCtrlBlocks`` says for the kernels.  A ``Block`` says
what the rule modules leave open -- tests/ctrl_pid_model.py, tests/ctrl_dist_model.py and tests/ctrl_loss_model.py state the
rules, the parameter sets and the seeds, and nothing else:

  * ``make(model, cfg, old)``: how its part of a model is made.  The gains block constructs the ``PidControlLoopModel``, the
    disturbance block calls ``disturb`` on it, the loss block ``attach``.  ``old`` is the model a reset replaces (None: a first
    model), and what a block reads from it is what its reset carries over: nothing for the gains, the plant's ``n``, the loss
    record's ``n``, ``lost`` and ``carry(old)``.
  * ``fields``: what it adds to a snapshot, with the dtype ``get_state`` returns, and ``read(model)``: their values.
  * ``wrong``: its wrong-reset knobs.  The CPU qualification sets one to show that the fixtures would catch that mistake.

``cfg`` describes one env: {"model": the constructor's arguments, "g", "key", "thr", "loss_key", "mode"} and any knob.
``step_cfg`` builds it for the step cases' model (set ``gi``, action stream ``s``), ``fused_cfg`` for the fused cases' model
``(p, gi, b)`` of ``pm.fused_layout``; set ``gi`` means gain set, weight set and loss set ``gi`` together.

Every generator takes the tier first and returns a named tuple that always holds the models or wrappers.  They are cached:
a reference takes 5 - 15 s to generate, is computed once, and its arrays are read-only."""
import collections
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctrl_dist_model as cd
import ctrl_feedback_model as fm
import ctrl_loss_model as lm
import ctrl_pid_model as pm
from ctrl_episodes_model import MAX_DURATION, EpisodicControlLoop
from ctrl_fixtures import LAYOUTS, PERIOD, START, STREAMS, U0S, X0S, dense_kw, rows_of, schedules_of

Block = collections.namedtuple("Block", "name fields read make wrong")
Tier = collections.namedtuple("Tier", "name blocks by_stream")

STEPS, MAX_STEPS, SHORT_MAX_STEPS, FAIL_DEG = pm.STEPS, pm.MAX_STEPS, pm.SHORT_MAX_STEPS, pm.FAIL_DEG
P, G, N_FUSED = pm.P, pm.G, pm.N_FUSED


def _make_gains(_, cfg, old):
    kw = dict(cfg["model"])
    if cfg.get("keep_last") and old is not None:
        kw["keep_last_err"] = old.last_err
    return pm.PidControlLoopModel(**kw)


def _make_disturbance(model, cfg, old):
    return cd.disturb(model, cfg["g"], cfg["key"], 0 if old is None or cfg.get("restart_n") else old.plant.n)


def _make_loss(model, cfg, old):
    if old is None:
        return lm.attach(model, cfg["thr"], cfg["loss_key"], 0, (0, 0, 0, 0), cfg.get("mode"))
    lm.attach(model, cfg["thr"], cfg["loss_key"], 0 if cfg.get("restart_loss_n") else old.loss.n, old.loss.lost, cfg.get("mode"))
    model.loss.carry(old.loss)
    return model


GAINS = Block("gains", (("gains", np.float64), ("last_error", np.float64)),
              lambda m: {"gains": list(m.gains), "last_error": m.last_err}, _make_gains, ("keep_last",))
DISTURBANCE = Block("disturbance", (("disturbance", np.float64), ("noise_key", np.uint64), ("noise_count", np.uint64)),
                    lambda m: {"disturbance": list(m.plant.g), "noise_key": m.plant.key, "noise_count": m.plant.n},
                    _make_disturbance, ("restart_n",))
LOSS_BLOCK = Block("loss", (("loss", np.uint32), ("loss_key", np.uint64), ("loss_count", np.uint64), ("lost", np.uint32)),
                   lambda m: {"loss": list(m.loss.thr), "loss_key": m.loss.key, "loss_count": m.loss.n, "lost": list(m.loss.lost)},
                   _make_loss, ("restart_loss_n", "mode"))

# ``by_stream``: the gains tier's staged-action reference is laid out [G][8] by (gain set, action stream), as it was generated
# before the tiers shared this code, and every array is kept as it was; from the disturbance up a model has a key of its own and
# the 64 models are laid out [P][G][2], as in every other fused case.
PID = Tier("pid", (GAINS,), True)
DIST = Tier("dist", (GAINS, DISTURBANCE), False)
LOSS = Tier("loss", (GAINS, DISTURBANCE, LOSS_BLOCK), False)


def new_fields(tier):
    """((field, dtype), ...) of everything the tier adds to the default control loop's state."""
    return tuple(fd for b in tier.blocks for fd in b.fields)


def make(tier, cfg, old=None):
    """A model of the tier; with ``old``, the fresh model a reset puts in its place."""
    known = {"model", "g", "key", "thr", "loss_key", "mode"} | {k for b in tier.blocks for k in b.wrong}
    assert set(cfg) <= known, sorted(set(cfg) - known)
    model = None
    for b in tier.blocks:
        model = b.make(model, cfg, old)
    return model


def read(tier, model):
    out = {}
    for b in tier.blocks:
        out.update(b.read(model))
    return out


def snapshot_of(tier, model):
    s = model.snapshot()
    s.update(read(tier, model))
    return s


def _rows(tier, states):
    """ctrl_fixtures.rows_of with the tier's own fields in their dtypes."""
    own = new_fields(tier)
    names = [f for f, _ in own]
    out = rows_of([{f: v for f, v in st.items() if f not in names} for st in states])
    for f, dtype in own:
        out[f] = np.array([st[f] for st in states], dtype)
    return out


def _frozen(*arrays):
    for v in arrays:
        v.setflags(write=False)


class _TierReset:
    """``reset()`` and ``state()`` of both wrappers: a reset env is ``make(tier, cfg, old model)``."""
    model = None

    def __init__(self, tier, cfg):
        self.tier, self.cfg = tier, cfg
        self.reset()

    def reset(self):
        self.model = make(self.tier, self.cfg, self.model)
        self.age, self.cost = 0, 0.0

    def state(self):
        s = EpisodicControlLoop.state(self)
        s.update(read(self.tier, self.model))
        return s


class EpisodicTierLoop(_TierReset, EpisodicControlLoop):
    """``EpisodicControlLoop`` on a tier's model: ``EpisodicTierLoop(tier, cfg)``."""


class FeedbackTierLoop(_TierReset, fm.FeedbackControlLoop):
    """``FeedbackControlLoop`` on a tier's model."""


# ---- the step cases: one model per (set, action stream) -----------------------------------------------------------------------------------
def step_cfg(tier, plant, start, period, gi, s, gains=None, mode=None, layout=None):
    """The step cases' model of (set gi, action stream s): the pair's own noise stream number for both keys, each under its own
    seed.  ``layout``: one of ctrl_fixtures.LAYOUTS on the default plant."""
    kw = dense_kw(plant, lists=True)
    if layout is not None:
        kw["positions"], kw["rrm_pos"] = LAYOUTS[layout]
    stream = cd.step_noise_stream(gi, s)
    cfg = {"model": dict(start=start, period=period, gains=pm.GAIN_SETS[gi] if gains is None else gains, **kw)}
    if DISTURBANCE in tier.blocks:
        cfg["g"], cfg["key"] = cd.G_SETS[gi], cd.key_of(cd.SEED64, stream)
    if LOSS_BLOCK in tier.blocks:
        cfg["thr"], cfg["loss_key"], cfg["mode"] = lm.THR_SETS[gi], cd.key_of(lm.SEED64, stream), mode
    return cfg


Steps = collections.namedtuple("Steps", "dev dur steps models")


@functools.lru_cache(maxsize=None)
def step_streams(tier, plant, K, seed, start, period, gains=None, layout=None, mode=None):
    """test_control_loop.model_streams on the tier's model: the same 8 action streams through one model per (set, stream).
    Returns the actions [K][8], per step {field: [G][8]...} and the models [G][8].  ``gains``: these gain sets instead of
    ``pm.GAIN_SETS`` (the first dimension is theirs)."""
    rng = np.random.default_rng(seed)
    dev = rng.integers(0, 2, (K, STREAMS)).astype(np.int32)
    dur = rng.integers(0, 20, (K, STREAMS)).astype(np.int32)
    sets = pm.GAIN_SETS if gains is None else gains
    models = [[make(tier, step_cfg(tier, plant, start, period, gi, s, gains=sets[gi], layout=layout, mode=mode)) for s in range(STREAMS)]
              for gi in range(len(sets))]
    own = new_fields(tier)
    steps = []
    for k in range(K):
        fb = [[m.step(int(dev[k, s]), int(dur[k, s])) for s, m in enumerate(row)] for row in models]
        sn = [[snapshot_of(tier, m) for m in row] for row in models]
        want = {"obs": np.array([[f[0] for f in r] for r in fb], np.int64),
                "rew": np.array([[np.float32(f[1]) for f in r] for r in fb], np.float32),
                "ang": np.array([[f[3]["Sensor angle"] for f in r] for r in fb], np.float64)}
        for f in ("now", "x", "u", "angle_deg", "rx_power"):
            want[f] = np.array([[q[f] for q in r] for r in sn], np.float64)
        want["qlen"] = np.array([[q["qlen"][:2] for q in r] for r in sn], np.int64)
        want["received"] = np.array([[q["received"][1:] for q in r] for r in sn], np.int64)
        for f in ("n_tx", "commands", "substeps"):
            want[f] = np.array([[q[f] for q in r] for r in sn], np.int64)
        for f, dtype in own:
            want[f] = np.array([[q[f] for q in r] for r in sn], dtype)
        _frozen(*want.values())
        steps.append(want)
    _frozen(dev, dur)
    return Steps(dev, dur, steps, models)


# ---- the fused cases: one model per (schedule or policy p, set gi, b) of pm.fused_layout ------------------------------------------------
def fused_keys(seed64):
    """uint64[512]: the key of every env of ``pm.fused_layout`` under one seed (``cd.SEED64``: the noise's, ``lm.SEED64``: the
    loss's)."""
    p, g, b, _ = pm.fused_layout()
    return np.array([cd.key_of(seed64, cd.fused_noise_stream(int(p[e]), int(g[e]), int(b[e]))) for e in range(N_FUSED)], np.uint64)


def fused_cfg(tier, p, gi, b, gains=None, g=None, thr=None, mode=None, **wrong):
    """The fused cases' model (p, gi, b): action stream ``pm.fused_stream``'s X0S / U0S, the sets gi, and the model's own noise
    stream number for both keys.  ``wrong``: the tier's wrong-reset knobs."""
    s = pm.fused_stream(p, gi, b)
    stream = cd.fused_noise_stream(p, gi, b)
    cfg = {"model": dict(x0=tuple(float(v) for v in X0S[s]), u0=float(U0S[s]), start=START, period=PERIOD,
                         gains=pm.GAIN_SETS[gi] if gains is None else gains)}
    if DISTURBANCE in tier.blocks:
        cfg["g"], cfg["key"] = cd.G_SETS[gi] if g is None else g, cd.key_of(cd.SEED64, stream)
    if LOSS_BLOCK in tier.blocks:
        cfg["thr"], cfg["loss_key"], cfg["mode"] = lm.THR_SETS[gi] if thr is None else thr, cd.key_of(lm.SEED64, stream), mode
    cfg.update(wrong)
    return cfg


def fused_models(by_stream=False):
    """[(p, gi, b)...] of the 64 fused models in the order of a reference's arrays, and those arrays' leading shape:
    [P][G][2], or for ``by_stream`` [G][8] with (p, b) the pair that puts set gi on action stream s."""
    if not by_stream:
        return [(p, gi, b) for p in range(P) for gi in range(G) for b in range(2)], (P, G, 2)
    where = {(gi, pm.fused_stream(p, gi, b)): (p, gi, b) for p in range(P) for gi in range(G) for b in range(2)}
    return [where[gi, s] for gi in range(G) for s in range(STREAMS)], (G, STREAMS)


def run_episodes(tier, p, gi, b, max_steps, **kw):
    """Stream ``pm.fused_stream(p, gi, b)`` of ``pm.episode_actions`` through model (p, gi, b): the rows (obs, reward, angle,
    ended) and the wrapper."""
    dev, dur = pm.episode_actions()
    s = pm.fused_stream(p, gi, b)
    env = EpisodicTierLoop(tier, fused_cfg(tier, p, gi, b, **kw))
    rows = [env.step(dev[k, s], dur[k, s], max_steps, FAIL_DEG) for k in range(STEPS)]
    return rows, env


Episodes = collections.namedtuple("Episodes", "dev dur obs rew ang ended final envs")


@functools.lru_cache(maxsize=None)
def episode_streams(tier, max_steps, mode=None, restart_loss_n=False, thr=None):
    """The staged-action case's reference, for every model of ``fused_models(tier.by_stream)`` and in its layout.  Returns the
    actions [K][8], the outputs and ``ended`` [K]..., the final state {field: ...} and the wrappers.  ``thr``: one threshold
    vector for every model."""
    order, lead = fused_models(tier.by_stream)
    dev, dur = pm.episode_actions()
    kw = {k: v for k, v in (("mode", mode), ("restart_loss_n", restart_loss_n), ("thr", thr)) if v}
    obs, rew = np.empty((STEPS, len(order)), np.int64), np.empty((STEPS, len(order)), np.float32)
    ang, ended = np.empty((STEPS, len(order)), np.float64), np.empty((STEPS, len(order)), np.uint8)
    states, envs = [], []
    for i, (p, gi, b) in enumerate(order):
        rows, env = run_episodes(tier, p, gi, b, max_steps, **kw)
        for k, (o, r, a, e) in enumerate(rows):
            obs[k, i], rew[k, i], ang[k, i], ended[k, i] = o, np.float32(r), a, e
        states.append(env.state())
        envs.append(env)
    obs, rew, ang, ended = (v.reshape((STEPS,) + lead) for v in (obs, rew, ang, ended))
    final = {f: v.reshape(lead + v.shape[1:]) for f, v in _rows(tier, states).items()}
    _frozen(dev, dur, obs, rew, ang, ended, *final.values())
    return Episodes(dev, dur, obs, rew, ang, ended, final, envs)


def run_schedule(tier, p, gi, b, max_steps, **kw):
    """ctrl_episodes_model.run_schedule for schedule p of ``schedules_of(P, pm.ROLLOUT_L)`` on model (p, gi, b), keeping every
    angle.  Returns the tally, the angles, ``ended`` per step and the wrapper."""
    sch = schedules_of(P, pm.ROLLOUT_L)[p]
    env = EpisodicTierLoop(tier, fused_cfg(tier, p, gi, b, **kw))
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


Schedules = collections.namedtuple("Schedules", "sch tally final ang ended envs")


@functools.lru_cache(maxsize=None)
def schedule_streams(tier, max_steps, mode=None, restart_loss_n=False, thr=None):
    """The schedule case's reference.  Returns the schedules, the tally [P][G][2][4], the final state {field: [P][G][2]...}, the
    angles and ``ended`` [K][P][G][2], and the wrappers."""
    kw = {k: v for k, v in (("mode", mode), ("restart_loss_n", restart_loss_n), ("thr", thr)) if v}
    sch = schedules_of(P, pm.ROLLOUT_L)
    tally = np.empty((P, G, 2, 4), np.float64)
    ang, ended = np.empty((STEPS, P, G, 2), np.float64), np.empty((STEPS, P, G, 2), np.uint8)
    states, envs = [], []
    for p, i, b in fused_models()[0]:
        tally[p, i, b], ang[:, p, i, b], ended[:, p, i, b], env = run_schedule(tier, p, i, b, max_steps, **kw)
        states.append(env.state())
        envs.append(env)
    final = {f: v.reshape((P, G, 2) + v.shape[1:]) for f, v in _rows(tier, states).items()}
    _frozen(tally, ang, ended, *final.values())
    return Schedules(sch, tally, final, ang, ended, envs)


Feedback = collections.namedtuple("Feedback", "tally rows final envs")


@functools.lru_cache(maxsize=None)
def feedback_streams(tier, max_steps, mode=None, restart_loss_n=False, thr=None, g=None):
    """The feedback case's reference (``pm.feedback_policies``, key |o|).  Returns the tally [P][G][2][8], the rows
    {field: [K][P][G][2]}, the final state {field: [P][G][2]...} and the wrappers.  ``g``: one weight vector for every model
    (all 0: the calm twin of the disturbance's qualification)."""
    kw = {k: v for k, v in (("mode", mode), ("restart_loss_n", restart_loss_n), ("thr", thr), ("g", g)) if v}
    sched, edg = pm.feedback_policies()
    tally = np.empty((P, G, 2, fm.COLS), np.float64)
    rows, states, envs = None, [], []
    for p, i, b in fused_models()[0]:
        env = FeedbackTierLoop(tier, fused_cfg(tier, p, i, b, **kw))
        tally[p, i, b], r, _ = fm.run_feedback(env, sched[p], edg[p], True, STEPS, max_steps, FAIL_DEG)
        if rows is None:
            rows = {f: np.empty((STEPS, P, G, 2), v.dtype) for f, v in r.items()}
        for f, v in r.items():
            rows[f][:, p, i, b] = v
        states.append(env.state())
        envs.append(env)
    final = {f: v.reshape((P, G, 2) + v.shape[1:]) for f, v in _rows(tier, states).items()}
    _frozen(tally, *rows.values(), *final.values())
    return Feedback(tally, rows, final, envs)
