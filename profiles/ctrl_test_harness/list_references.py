"""One line per array of every reference the control-loop tests generate: name, dtype, shape, SHA-256 of its bytes.

    python profiles/ctrl_test_harness/list_references.py > listing.txt

Every stream generator of tests/ctrl_tiers.py is called with every argument combination the tests under tests/ use, and the
single-model calls of the CPU qualification with each wrong-reset knob once.  The per-step dictionaries of ``step_streams`` are
stacked along the steps, one line per field.  README.md says what the listing is for; only the section "call syntax" differs
from the script that produced the same listing at the parent commit."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctrl_dist_model as cd
import ctrl_loss_model as lm
import ctrl_pid_model as pm
import ctrl_tiers as ct

TIER = {"pid": ct.PID, "dist": ct.DIST, "loss": ct.LOSS}

LINES = []


def emit(name, a):
    a = np.ascontiguousarray(a)
    LINES.append("%s %s %s %s" % (name, a.dtype, "x".join(map(str, a.shape)) or "scalar", hashlib.sha256(a.tobytes()).hexdigest()))


def emit_dict(name, d):
    for f in sorted(d):
        emit("%s/%s" % (name, f), d[f])


def emit_steps(name, steps):
    for f in sorted(steps[0]):
        emit("%s/steps/%s" % (name, f), np.stack([w[f] for w in steps]))


def emit_state(name, st):
    for f in sorted(st):
        emit("%s/%s" % (name, f), np.array(st[f]))


GRID = [(1, 20, 10), (2, 0, 3), (3, 50, 1)]
EDGE = (24, 20, 5, 3)                                    # test_control_loop_edges: K, SEED, START, PERIOD
ZERO = (0, 0, 0, 0)


# ---- call syntax ---------------------------------------------------------------------------------------------------------------------------

def steps_of(tier, plant, K, seed, start, period, **kw):
    r = ct.step_streams(TIER[tier], plant, K, seed, start, period, **{k: v for k, v in kw.items() if v is not None})
    return r.dev, r.dur, r.steps


def episodes_of(tier, max_steps, **kw):
    r = ct.episode_streams(TIER[tier], max_steps, **kw)
    return {"dev": r.dev, "dur": r.dur, "obs": r.obs, "rew": r.rew, "ang": r.ang, "ended": r.ended}, r.final


def schedules_of(tier, max_steps, **kw):
    r = ct.schedule_streams(TIER[tier], max_steps, **kw)
    return {"sch": r.sch, "tally": r.tally, "ang": r.ang, "ended": r.ended}, r.final


def feedback_of(tier, max_steps, **kw):
    r = ct.feedback_streams(TIER[tier], max_steps, **kw)
    return r.tally, r.rows, r.final


def one_schedule(tier, p, gi, b, max_steps, **kw):
    r = ct.run_schedule(TIER[tier], p, gi, b, max_steps, **kw)
    return {"tally": np.array(r[0]), "ang": r[1], "ended": r[2]}, r[3].state()


def one_episodes(tier, p, gi, b, max_steps, **kw):
    rows, env = ct.run_episodes(TIER[tier], p, gi, b, max_steps, **kw)
    return {"rows": np.array([[float(v) for v in r] for r in rows])}, env.state()


def keys_of(tier):
    return ct.fused_keys({"dist": cd.SEED64, "loss": lm.SEED64}[tier])


# ---- the calls ---------------------------------------------------------------------------------------
def main():
    for tier in ("pid", "dist", "loss"):
        for plant in (None, "dense"):
            for seed, start, period in GRID:
                name = "%s.step_streams(%s,70,%d,%d,%d)" % (tier, plant, seed, start, period)
                dev, dur, steps = steps_of(tier, plant, 70, seed, start, period)
                emit(name + "/dev", dev), emit(name + "/dur", dur), emit_steps(name, steps)
    for plant in (None, "dense"):
        name = "pid.step_streams(%s,70,1,20,10,gains=default)" % plant
        dev, dur, steps = steps_of("pid", plant, 70, 1, 20, 10, gains=(pm.DEFAULT_GAINS,))
        emit(name + "/dev", dev), emit(name + "/dur", dur), emit_steps(name, steps)
    K, seed, start, period = EDGE
    for mode in (None, "phy_only"):
        name = "loss.step_streams(None,%d,%d,%d,%d,layout=%s,mode=%s)" % (K, seed, start, period, lm.FAILING_LAYOUT, mode)
        dev, dur, steps = steps_of("loss", None, K, seed, start, period, layout=lm.FAILING_LAYOUT, mode=mode)
        emit(name + "/dev", dev), emit(name + "/dur", dur), emit_steps(name, steps)

    for tier, sizes in (("pid", (pm.MAX_STEPS, pm.SHORT_MAX_STEPS)), ("dist", (pm.SHORT_MAX_STEPS,)), ("loss", (pm.SHORT_MAX_STEPS,))):
        for ms in sizes:
            name = "%s.episode_streams(%d)" % (tier, ms)
            out, final = episodes_of(tier, ms)
            emit_dict(name, out), emit_dict(name + "/final", final)
    sched_cases = [("pid", pm.MAX_STEPS, {}), ("pid", pm.SHORT_MAX_STEPS, {}), ("dist", pm.MAX_STEPS, {}), ("loss", pm.MAX_STEPS, {}),
                   ("loss", pm.MAX_STEPS, {"thr": ZERO}), ("loss", pm.MAX_STEPS, {"mode": "one_thr"}), ("loss", pm.MAX_STEPS, {"mode": "no_pop"}),
                   ("loss", pm.MAX_STEPS, {"restart_loss_n": True})]
    for tier, ms, kw in sched_cases:
        name = "%s.schedule_streams(%d%s)" % (tier, ms, "".join(",%s=%s" % kv for kv in sorted(kw.items())))
        out, final = schedules_of(tier, ms, **kw)
        emit_dict(name, out), emit_dict(name + "/final", final)
    fb_cases = [("pid", pm.MAX_STEPS, {}), ("pid", pm.SHORT_MAX_STEPS, {}), ("dist", pm.MAX_STEPS, {}),
                ("dist", pm.MAX_STEPS, {"g": (0.0, 0.0, 0.0, 0.0)}), ("loss", pm.MAX_STEPS, {})]
    for tier, ms, kw in fb_cases:
        name = "%s.feedback_streams(%d%s)" % (tier, ms, "".join(",%s=%s" % kv for kv in sorted(kw.items())))
        tally, rows, final = feedback_of(tier, ms, **kw)
        emit(name + "/tally", tally), emit_dict(name + "/rows", rows), emit_dict(name + "/final", final)

    # the single-model calls of the CPU qualification, one model each
    one_cases = [("pid", 1, 3, 1, pm.MAX_STEPS, {"keep_last": True}), ("pid", 2, 2, 0, pm.MAX_STEPS, {"gains": (0.02, 0.0, 0.05)}),
                 ("dist", 1, 3, 1, pm.MAX_STEPS, {"restart_n": True}), ("dist", 2, 5, 0, pm.MAX_STEPS, {"g": (0.001, 0.0, 0.0005, 0.01)}),
                 ("loss", 1, 3, 1, pm.MAX_STEPS, {"restart_loss_n": True}), ("loss", 2, 5, 0, pm.MAX_STEPS, {"mode": "no_pop"})]
    for tier, p, gi, b, ms, kw in one_cases:
        name = "%s.run_schedule(%d,%d,%d,%d%s)" % (tier, p, gi, b, ms, "".join(",%s=%s" % kv for kv in sorted(kw.items())))
        out, st = one_schedule(tier, p, gi, b, ms, **dict(kw))
        emit_dict(name, out), emit_state(name + "/state", st)
    for tier, p, gi, b, ms, kw in (("pid", 1, 3, 1, pm.SHORT_MAX_STEPS, {"keep_last": True}), ("dist", 1, 3, 1, pm.SHORT_MAX_STEPS, {"restart_n": True}),
                                   ("loss", 1, 3, 1, pm.SHORT_MAX_STEPS, {"restart_loss_n": True})):
        name = "%s.run_episodes(%d,%d,%d,%d%s)" % (tier, p, gi, b, ms, "".join(",%s=%s" % kv for kv in sorted(kw.items())))
        out, st = one_episodes(tier, p, gi, b, ms, **dict(kw))
        emit_dict(name, out), emit_state(name + "/state", st)
    for tier in ("dist", "loss"):
        emit("%s.fused_keys()" % tier, keys_of(tier))
    sched, edges = pm.feedback_policies()
    emit("feedback_policies()/sched", sched), emit("feedback_policies()/edges", edges)
    dev, dur = pm.episode_actions()
    emit("episode_actions()/dev", dev), emit("episode_actions()/dur", dur)
    print("\n".join(LINES))


main()
