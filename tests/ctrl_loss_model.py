"""Test infrastructure, not a test: the control-loop model with the packet erasures of gw_ctrl_set_loss (include/gymwipe_amd.h)
-- tests/ctrl_dist_model.py's disturbed PID model whose band takes one counter-based draw per transmission -- and the two
episode wrappers whose ``reset()`` hands the old model's loss record to the fresh one.

``attach(model, thr, key, n, lost)`` hooks a built model from outside, nothing in oracle/des_model.py is edited:

  * ``model.world.band.transmit`` is wrapped as an instance attribute.  Every transmission goes through it exactly once, when it
    goes on the air and before any PHY has decided about it.  The link comes from the packet's MAC header: ``src == RRM`` makes
    it link 0 (``dst`` the sensor) or 1 (the controller); otherwise it is 2 + the sender's index (sensor 2, controller 3).  In
    pure Python integers:

        z  = key ^ (n * 0xA0761D6478BD642F)                       (mod 2^64)
        z += 0x9E3779B97F4A7C15
        z  = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
        z  = (z ^ (z >> 27)) * 0x94D049BB133111EB
        z ^= z >> 31
        r  = z >> 32
        erased = r < thr[link];  lost[link] += erased (mod 2^32);  n += 1

    and the packet is marked.
  * every radio's ``phy.mac_out.trigger`` is wrapped, an instance attribute as well (``Phy._receive`` looks it up when it has
    decoded a packet): an erased packet is not handed up.  The MAC of an erased announcement's addressee never opens its window;
    an erased data packet has left its queue and been on the air, and reaches nobody.

A reset env is a fresh model that goes on drawing where the old one stopped: ``thr``, ``key``, ``n`` and ``lost`` survive.
``mode`` selects one of the wrong rules the CPU qualification compares against: ``"phy_only"`` (the draw is taken only when the
addressee's PHY decoded the packet), ``"one_thr"`` (threshold 0 for all links), ``"no_pop"`` (an erased data packet goes back to
the head of its queue); ``restart_n`` is the wrong reset.

The fixtures tests/test_ctrl_loss.py runs on are defined here and qualified on the model alone in tests/test_ctrl_loss_cpu.py."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctrl_dist_model as cd
import ctrl_pid_model as pm
from ctrl_episodes_model import EpisodicControlLoop
from ctrl_feedback_model import FeedbackControlLoop
from oracle import des_model as dm

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
LOSS_FIELDS = ("loss", "loss_key", "loss_count", "lost")


def draw(key, n):
    """The rule's ``r`` for one key and count, Python integers throughout."""
    z = (key ^ ((n * 0xA0761D6478BD642F) & M64)) & M64
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z >> 32


class LossRecord:
    """An env's record {thr, key, n, lost}, and what the qualification asks about it: per link the receptions the addressee's PHY
    decoded and the rule erased, and those delivered; the draws that fell on transmissions the addressee's PHY rejected."""

    def __init__(self, thr, key, n=0, lost=(0, 0, 0, 0), mode=None):
        self.thr, self.key, self.n, self.lost = [int(v) for v in thr], int(key), int(n), [int(v) for v in lost]
        self.mode = mode
        self.erased_decoded, self.delivered = [0, 0, 0, 0], [0, 0, 0, 0]
        self.sent = []                                       # every packet that took a draw

    def take(self, link):
        r = draw(self.key, self.n)
        erased = r < self.thr[0 if self.mode == "one_thr" else link]
        if erased:
            self.lost[link] = (self.lost[link] + 1) & M32
        self.n = (self.n + 1) & M64
        return erased

    @property
    def rejected_draws(self):
        return sum(1 for p in self.sent if not p.loss_decoded)

    def carry(self, old):
        """Bookkeeping across a reset: the qualification counts over all episodes of an env."""
        self.erased_decoded, self.delivered, self.sent = old.erased_decoded, old.delivered, old.sent


def attach(model, thr, key, n=0, lost=(0, 0, 0, 0), mode=None):
    """Hook the rule into a built model; returns the model.  ``model.loss`` is its LossRecord."""
    rec = model.loss = LossRecord(thr, key, n, lost, mode)
    band = model.world.band
    sensor, controller, _ = model.devs
    index_of = {d.mac_addr: i for i, d in enumerate(model.devs)}

    def link_of(packet):
        h = packet.header
        if h.src == dm.RRM_ADDR:
            return 0 if h.dst == sensor.mac_addr else 1
        return 2 + index_of[h.src]

    inner_transmit = band.transmit

    def transmit(sender, power, packet, mcs_h, mcs_p):
        packet.loss_link = link_of(packet)
        packet.loss_decoded = False
        packet.loss_erased = False
        if rec.mode != "phy_only":
            packet.loss_erased = rec.take(packet.loss_link)
            rec.sent.append(packet)
            if packet.loss_erased and rec.mode == "no_pop" and packet.loss_link >= 2:
                sender.mac.queue.appendleft(packet)
        return inner_transmit(sender, power, packet, mcs_h, mcs_p)
    band.transmit = transmit

    def hook(radio, addr):
        inner = radio.phy.mac_out.trigger

        def trigger(packet):
            if packet.header.dst == addr:                    # the addressee's PHY has decoded it
                packet.loss_decoded = True
                if rec.mode == "phy_only":
                    packet.loss_erased = rec.take(packet.loss_link)
                    rec.sent.append(packet)
                if packet.loss_erased:
                    rec.erased_decoded[packet.loss_link] += 1
                else:
                    rec.delivered[packet.loss_link] += 1
            if not packet.loss_erased:
                inner(packet)
        radio.phy.mac_out.trigger = trigger
    for d in model.devs:
        hook(d, d.mac_addr)
    hook(model.rrm, dm.RRM_ADDR)
    return model


def snapshot_of(model):
    s = cd.snapshot_of(model)
    s["loss"], s["loss_key"], s["loss_count"], s["lost"] = list(model.loss.thr), model.loss.key, model.loss.n, list(model.loss.lost)
    return s


class _LossReset(cd._DistReset):
    """``reset()`` of both wrappers: ctrl_dist_model's fresh disturbed model, with the rule attached on the env's own thresholds
    and key from the counts the old model had reached.  ``restart_loss_n``: the wrong reset -- every episode replays the
    sequence from 0."""

    def __init__(self, x0=(0.0, 0.0, 0.05, 0.0), u0=0.1, thr=(0, 0, 0, 0), loss_key=0, mode=None, restart_loss_n=False, **kw):
        self.thr, self.loss_key, self.mode, self.restart_loss_n = tuple(int(v) for v in thr), int(loss_key), mode, restart_loss_n
        super().__init__(x0=x0, u0=u0, **kw)

    def reset(self):
        old = None if self.model is None else self.model.loss
        cd._DistReset.reset(self)
        if old is None:
            attach(self.model, self.thr, self.loss_key, 0, (0, 0, 0, 0), self.mode)
        else:
            attach(self.model, self.thr, self.loss_key, 0 if self.restart_loss_n else old.n, old.lost, self.mode)
            self.model.loss.carry(old)

    def state(self):
        s = cd._DistReset.state(self)
        r = self.model.loss
        s["loss"], s["loss_key"], s["loss_count"], s["lost"] = list(r.thr), r.key, r.n, list(r.lost)
        return s


class EpisodicLossLoop(_LossReset, EpisodicControlLoop):
    """``EpisodicControlLoop`` on the lossy, disturbed PID model."""


class FeedbackLossLoop(_LossReset, FeedbackControlLoop):
    """``FeedbackControlLoop`` on the lossy, disturbed PID model."""


# ---- fixtures of tests/test_ctrl_loss.py ----------------------------------------------------------------------------------------------------
# 8 loss sets as probabilities per link (announcement to the sensor, to the controller, sensor's data, controller's data): none
# first (its envs must walk the disturbance model's trajectory), the announcements only, the data links only, mixtures, and last
# both announcements at thr = 0xFFFFFFFF, where no step is ever granted.  Set i runs under cd.G_SETS[i] and pm.GAIN_SETS[i]: the
# loss instantiations are disturbance and PID instantiations, and all three rules run together.
P_SETS = ((0.0, 0.0, 0.0, 0.0), (0.3, 0.3, 0.0, 0.0), (0.0, 0.0, 0.3, 0.3), (0.25, 0.1, 0.4, 0.2), (0.1, 0.25, 0.2, 0.4),
          (0.5, 0.5, 0.5, 0.5), (0.05, 0.6, 0.7, 0.05), (1.0, 1.0, 0.5, 0.5))
G = len(P_SETS)
assert G == pm.G == cd.G
ALL_LOST = 7                                                 # the set with 0xFFFFFFFF on both announcement links
SEED = 0x5EED0F10557DA7A5EED                                 # wider than 64 bits: the helper takes its low 64
SEED64 = SEED & M64
STEPS, MAX_STEPS, SHORT_MAX_STEPS, FAIL_DEG = pm.STEPS, pm.MAX_STEPS, pm.SHORT_MAX_STEPS, pm.FAIL_DEG
P, N_FUSED, PER_SET = pm.P, pm.N_FUSED, pm.PER_SET
FAILING_LAYOUT = "same_distance"                             # tests/test_control_loop_edges.LAYOUTS: the commands do not decode


def threshold(p):
    """``actions.ctrl_loss_threshold`` restated for one probability in [0, 1]."""
    return min(int(p * 4294967296.0), M32)


THR_SETS = tuple(tuple(threshold(p) for p in row) for row in P_SETS)
assert THR_SETS[0] == (0, 0, 0, 0) and THR_SETS[ALL_LOST][:2] == (M32, M32)


def thr_array():
    return np.array(THR_SETS, np.uint32)


def _rows(states):
    """ctrl_dist_model._rows with the four fields of the loss."""
    out = cd._rows([{f: v for f, v in st.items() if f not in LOSS_FIELDS} for st in states])
    out["loss"] = np.array([st["loss"] for st in states], np.uint32)
    out["loss_key"] = np.array([st["loss_key"] for st in states], np.uint64)
    out["loss_count"] = np.array([st["loss_count"] for st in states], np.uint64)
    out["lost"] = np.array([st["lost"] for st in states], np.uint32)
    return out


def step_model(plant, start, period, gi, s, thr=None, mode=None, layout=None):
    """ctrl_dist_model.step_model with the rule attached: the loss's stream number is the noise's, its seed its own."""
    if layout is None:
        m = cd.step_model(plant, start, period, gi, s)
    else:
        from test_control_loop_edges import LAYOUTS
        pos, rrm = LAYOUTS[layout]
        m = pm.PidControlLoopModel(positions=pos, rrm_pos=rrm, start=start, period=period, gains=pm.GAIN_SETS[gi])
        cd.disturb(m, cd.G_SETS[gi], cd.key_of(cd.SEED64, cd.step_noise_stream(gi, s)))
    return attach(m, THR_SETS[gi] if thr is None else thr, cd.key_of(SEED64, cd.step_noise_stream(gi, s)), mode=mode)


@functools.lru_cache(maxsize=None)
def step_streams(plant, K, seed, start, period, layout=None, mode=None):
    """ctrl_dist_model.step_streams on the lossy model: the same 8 action streams through one model per (set, stream).  Returns
    the actions [K][8], per step {field: [G][8]...} and the models."""
    from test_control_loop import STREAMS
    rng = np.random.default_rng(seed)
    dev = rng.integers(0, 2, (K, STREAMS)).astype(np.int32)
    dur = rng.integers(0, 20, (K, STREAMS)).astype(np.int32)
    models = [[step_model(plant, start, period, gi, s, layout=layout, mode=mode) for s in range(STREAMS)] for gi in range(G)]
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
        for f in ("noise_key", "noise_count", "loss_key", "loss_count"):
            want[f] = np.array([[q[f] for q in r] for r in sn], np.uint64)
        for f in ("loss", "lost"):
            want[f] = np.array([[q[f] for q in r] for r in sn], np.uint32)
        pm._frozen(*want.values())
        steps.append(want)
    pm._frozen(dev, dur)
    return dev, dur, steps, models


def fused_keys():
    """uint64[512]: the loss key of every env of ``pm.fused_layout``."""
    p, g, b, _ = pm.fused_layout()
    return np.array([cd.key_of(SEED64, cd.fused_noise_stream(int(p[e]), int(g[e]), int(b[e]))) for e in range(N_FUSED)], np.uint64)


def episodic(p, gi, b, cls=EpisodicLossLoop, thr=None, mode=None, restart_loss_n=False):
    """The wrapper of fused model (p, gi, b): ctrl_dist_model.episodic's, with thresholds of set gi and the model's own loss key."""
    t = pm._g()
    s = pm.fused_stream(p, gi, b)
    stream = cd.fused_noise_stream(p, gi, b)
    return cls(x0=t.X0S[s], u0=t.U0S[s], g=cd.G_SETS[gi], key=cd.key_of(cd.SEED64, stream), thr=THR_SETS[gi] if thr is None else thr,
               loss_key=cd.key_of(SEED64, stream), mode=mode, restart_loss_n=restart_loss_n, start=t.START, period=t.PERIOD,
               gains=pm.GAIN_SETS[gi])


def run_episodes(p, gi, b, max_steps, **kw):
    dev, dur = pm.episode_actions()
    s = pm.fused_stream(p, gi, b)
    env = episodic(p, gi, b, **kw)
    rows = [env.step(dev[k, s], dur[k, s], max_steps, FAIL_DEG) for k in range(STEPS)]
    return rows, env


def _every_model():
    for p in range(P):
        for i in range(G):
            for b in range(2):
                yield p, i, b


@functools.lru_cache(maxsize=None)
def episode_streams(max_steps, mode=None, restart_loss_n=False, thr=None):
    """The staged-action case's reference, for every (p, g, b) of ``pm.fused_layout``.  Returns the outputs and ``ended``
    [K][P][G][2], the final state {field: [P][G][2]...} and the wrappers.  ``thr``: one threshold vector for every model."""
    shape = (STEPS, P, G, 2)
    obs, rew = np.empty(shape, np.int64), np.empty(shape, np.float32)
    ang, ended = np.empty(shape, np.float64), np.empty(shape, np.uint8)
    states, envs = [], []
    for p, i, b in _every_model():
        rows, env = run_episodes(p, i, b, max_steps, mode=mode, restart_loss_n=restart_loss_n, thr=thr)
        for k, (o, r, a, e) in enumerate(rows):
            obs[k, p, i, b], rew[k, p, i, b], ang[k, p, i, b], ended[k, p, i, b] = o, np.float32(r), a, e
        states.append(env.state())
        envs.append(env)
    final = {f: v.reshape((P, G, 2) + v.shape[1:]) for f, v in _rows(states).items()}
    pm._frozen(obs, rew, ang, ended, *final.values())
    return obs, rew, ang, ended, final, envs


def run_schedule(p, gi, b, max_steps, **kw):
    """ctrl_dist_model.run_schedule on the lossy model (p, gi, b)."""
    from ctrl_episodes_model import MAX_DURATION
    sch = pm._g().schedules_of(P, pm.ROLLOUT_L)[p]
    env = episodic(p, gi, b, **kw)
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
def schedule_streams(max_steps, mode=None, restart_loss_n=False, thr=None):
    """The schedule case's reference.  Returns the schedules, the tally [P][G][2][4], the final state {field: [P][G][2]...}, the
    angles and ``ended`` [K][P][G][2], and the wrappers."""
    sch = pm._g().schedules_of(P, pm.ROLLOUT_L)
    tally = np.empty((P, G, 2, 4), np.float64)
    ang, ended = np.empty((STEPS, P, G, 2), np.float64), np.empty((STEPS, P, G, 2), np.uint8)
    states, envs = [], []
    for p, i, b in _every_model():
        tally[p, i, b], ang[:, p, i, b], ended[:, p, i, b], env = run_schedule(p, i, b, max_steps, mode=mode,
                                                                                 restart_loss_n=restart_loss_n, thr=thr)
        states.append(env.state())
        envs.append(env)
    final = {f: v.reshape((P, G, 2) + v.shape[1:]) for f, v in _rows(states).items()}
    pm._frozen(tally, ang, ended, *final.values())
    return sch, tally, final, ang, ended, envs


@functools.lru_cache(maxsize=None)
def feedback_streams(max_steps, mode=None, restart_loss_n=False, thr=None):
    """The feedback case's reference (``pm.feedback_policies``, key |o|).  Returns the tally [P][G][2][8], the rows
    {field: [K][P][G][2]}, the final state {field: [P][G][2]...} and the wrappers."""
    import ctrl_feedback_model as fm
    sched, edg = pm.feedback_policies()
    tally = np.empty((P, G, 2, fm.COLS), np.float64)
    rows, states, envs = None, [], []
    for p, i, b in _every_model():
        env = episodic(p, i, b, cls=FeedbackLossLoop, mode=mode, restart_loss_n=restart_loss_n, thr=thr)
        tally[p, i, b], r, _ = fm.run_feedback(env, sched[p], edg[p], True, STEPS, max_steps, FAIL_DEG)
        if rows is None:
            rows = {f: np.empty((STEPS, P, G, 2), v.dtype) for f, v in r.items()}
        for f, v in r.items():
            rows[f][:, p, i, b] = v
        states.append(env.state())
        envs.append(env)
    final = {f: v.reshape((P, G, 2) + v.shape[1:]) for f, v in _rows(states).items()}
    pm._frozen(tally, *rows.values(), *final.values())
    return tally, rows, final, envs
