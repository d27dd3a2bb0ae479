"""The closed control loop where its existing tests never go (tests/test_control_loop.py and tests/test_ctrl_rollout.py use the
default layout and a 1 ms counter interval, on which every reception succeeds, no two events share a time and a step holds
at most 21 counter ticks):
  * layouts on which a reception FAILS -- an announcement refused, a data packet lost at either destination -- so that the
    `granted == false` and `ok == false` branches of ctrl_step_body.h and both `s_ber[(listener, talker, state)]` lookups
    decide something;
  * counter intervals that put a tick EXACTLY on the end of a data transmission or on the end of the step;
  * the smallest counter interval gw_ctrl_create admits, which fills the staging columns of a step's appends furthest.
The specification is oracle/des_model.py::ControlLoopModel, bit for bit, after every step, for ctrl_step_kernel and for
ctrl_rollout_kernel on a twin handle (and ctrl_rollout_sched_kernel on one layout).  Env e follows stream
(5 e + e // 64) % 8 (tests/test_control_loop.py); N = 70 is one full block and a ragged wave.  The data the cases run on is
defined here; tests/test_control_loop_edges_cpu.py pins on the model alone that it does what each case is named for."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ctrl_episodes_model import FIELDS, EpisodicControlLoop, run_schedule
from ctrl_fixtures import ALL_FIELDS, LAYOUTS, STREAMS, T, U0S, X0S, assert_same, stream_of
from test_ctrl_rollout import assert_states_equal, state_of

from oracle import des_model as dm

N, K = 70, 24
START, PERIOD, SEED = 5, 3, 20
TIE_ACTS = [(0, 19), (1, 7), (0, 3), (1, 19), (0, 0), (1, 12)]
TIE_CASES = ("t_e1", "t_e1/2", "t_end/8")
GATE_INTERVAL = 0.00097                                    # the issue's figure: just above the smallest interval admitted
FLAG_TIE = 4
SCHED_P, SCHED_L, SCHED_N, SCHED_MAX, SCHED_FAIL = 2, 3, 128, 7, 90.0       # max_steps does not divide K
SCHEDULES = [[(0, 19), (1, 5), (0, 7)], [(1, 12), (0, 3), (1, 250)]]         # 4- and 5-digit slot counts for both devices


def running_sum(interval, n):
    """The time of counter tick n (tick 0 falls at 0): n additions, as the event heap and the kernels keep it."""
    w = 0.0
    for _ in range(n):
        w = w + interval
    return w


@functools.lru_cache(maxsize=None)
def tie_times():
    """From the model: the end t_e1 of the first data transmission of a fresh env's step {device 0, duration 19} (when its
    completion event fires, as tests/test_oracle_pinning.py::tie_intervals derives it) and the end t_end of that step.
    Neither depends on the counter interval as long as the queue holds a packet when the window opens."""
    m = dm.ControlLoopModel(start=0, period=1)
    m.step(0, 19)
    tx = m.world.band.log[1]
    assert tx.sender is m.devs[0]
    return tx.start + (tx.stop - tx.start), m.sim.now


def tie_interval(case):
    t_e1, t_end = tie_times()
    return {"t_e1": t_e1, "t_e1/2": t_e1 / 2, "t_end/8": t_end / 8}[case]


def layout_actions():
    """The convention of test_control_loop.model_streams: seed 20, devices drawn first, then durations."""
    rng = np.random.default_rng(SEED)
    dev = rng.integers(0, 2, (K, STREAMS)).astype(np.int32)
    dur = rng.integers(0, 20, (K, STREAMS)).astype(np.int32)
    return dev, dur


def tie_actions():
    """Stream s takes TIE_ACTS rotated by s: streams 0 and 6 open with {0, 19} from a fresh env, where the tie is."""
    acts = np.array([[TIE_ACTS[(k + s) % len(TIE_ACTS)] for s in range(STREAMS)] for k in range(len(TIE_ACTS))], np.int32)
    return np.ascontiguousarray(acts[:, :, 0]), np.ascontiguousarray(acts[:, :, 1])


def gate_actions():
    """The longest window on two steps of three (which two differs by stream), random devices, random durations between."""
    rng = np.random.default_rng(SEED)
    dev = rng.integers(0, 2, (K, STREAMS)).astype(np.int32)
    dur = rng.integers(0, 20, (K, STREAMS)).astype(np.int32)
    k, s = np.mgrid[0:K, 0:STREAMS]
    dur[(k + s) % 3 != 2] = 19
    return dev, dur


def case_of(name):
    """-> (the model's keyword arguments, VecControlLoopEnv's, the actions int32[steps][8] x 2)."""
    if name in LAYOUTS:
        pos, rrm = LAYOUTS[name]
        return (dict(positions=pos, rrm_pos=rrm, start=START, period=PERIOD),
                dict(positions=pos + (rrm,), ctrl_start_tick=START, ctrl_period_ticks=PERIOD), layout_actions())
    interval, acts = (GATE_INTERVAL, gate_actions()) if name == "gate" else (tie_interval(name), tie_actions())
    return (dict(start=0, period=1, counter_interval=interval),
            dict(ctrl_start_tick=0, ctrl_period_ticks=1, counter_interval=interval), acts)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case's 8 streams through one ControlLoopModel each: the actions and, per step, the model's feedback and state as
    arrays over the streams -- the fields tests/test_control_loop.py compares and ``wake``, the time of the next counter tick.
    Also per step and stream {ticks, commands, transmissions, deliveries to controller / actuator} of that step alone.
    Computed once per case, shared and never modified."""
    model_kw, _, (dev, dur) = case_of(name)
    models = [dm.ControlLoopModel(**model_kw) for _ in range(STREAMS)]
    steps, counts = [], np.zeros((len(dev), STREAMS, 5), np.int64)
    for k in range(len(dev)):
        before = [(m.tick, m.n_cmd, len(m.world.band.log), m.got[1], m.got[2]) for m in models]
        fb = [m.step(int(dev[k, s]), int(dur[k, s])) for s, m in enumerate(models)]
        counts[k] = np.array([(m.tick, m.n_cmd, len(m.world.band.log), m.got[1], m.got[2]) for m in models]) - np.array(before)
        sn = [m.snapshot() for m in models]
        assert all(q["qlen"][2] == 0 for q in sn)
        want = {"obs": np.array([f[0] for f in fb], np.int64), "rew": np.array([np.float32(f[1]) for f in fb], np.float32),
                "ang": np.array([f[3]["Sensor angle"] for f in fb], np.float64),
                "wake": np.array([m.wake for m in models], np.float64),
                "qlen": np.array([q["qlen"][:2] for q in sn], np.int64),
                "received": np.array([q["received"][1:] for q in sn], np.int64)}
        for f in ("now", "x", "u", "angle_deg", "rx_power"):
            want[f] = np.array([q[f] for q in sn], np.float64)
        for f in ("n_tx", "commands", "substeps"):
            want[f] = np.array([q[f] for q in sn], np.int64)
        for v in want.values():
            v.setflags(write=False)
        steps.append(want)
    counts.setflags(write=False)
    return dev, dur, steps, counts, models


@functools.lru_cache(maxsize=None)
def schedule_reference():
    """SCHEDULES[p] on stream s of the rrm_edge layout, every (p, s), from X0S[s] / U0S[s]: the tally [P][8][4], the states
    after the last step (listed [p][s]) and the actions taken."""
    from gymwipe_amd import actions
    model_kw = case_of("rrm_edge")[0]
    sch = actions.make_ctrl_schedules(SCHEDULES, SCHED_L)
    tally, states, taken = np.empty((SCHED_P, STREAMS, 4), np.float64), [], []
    for p in range(SCHED_P):
        for s in range(STREAMS):
            env = EpisodicControlLoop(x0=X0S[s], u0=U0S[s], **model_kw)
            tally[p, s], _, t = run_schedule(env, sch[p], K, SCHED_MAX, SCHED_FAIL)
            states.append(env.state())
            taken.append(t)
    final = {f: np.array([st[f] for st in states]) for f in states[0]}
    for f, a in final.items():
        final[f] = a.astype(np.float64) if f in ("now", "x", "u", "angle_deg", "rx_power", "cost") else a.astype(np.int64)
    for v in (tally,) + tuple(final.values()):
        v.setflags(write=False)
    return sch, tally, final, np.array(taken).reshape(SCHED_P, STREAMS, K, 2)


def _run_case(name):
    """ctrl_step_kernel step by step against the model, every field after every step; then ctrl_rollout_kernel, one launch of
    the same actions on a twin handle: its rows are the steps' and it ends in the identical state."""
    from gymwipe_amd import VecControlLoopEnv
    _, env_kw, _ = case_of(name)
    dev, dur, steps, _, _ = reference(name)
    so = stream_of(N)
    d, u = T(dev[:, so]), T(dur[:, so])
    one = VecControlLoopEnv(N, **env_kw)
    for k, want in enumerate(steps):
        obs, rew, done, info = one.step({"device": d[k], "duration": u[k]})
        got = {"obs": obs.cpu().numpy(), "rew": rew.cpu().numpy(), "ang": info["Sensor angle"].cpu().numpy()}
        got.update(state_of(one, FIELDS + ("wake",)))
        for f, w in want.items():
            assert_same(got[f], w[so], (name, f, k))
        assert not (one.get_state("flags") & 3).any() and not done.any(), k
    st = state_of(one)
    twin = VecControlLoopEnv(N, **env_kw)
    obs, rew, done, info = twin.rollout(d, u)
    assert not done.any()
    for f, g in (("obs", obs), ("rew", rew), ("ang", info["Sensor angle"])):
        g = g.cpu().numpy()
        for k, want in enumerate(steps):
            assert_same(g[k], want[f][so], (name, "rollout", f, k))
    assert_states_equal(state_of(twin), st, (name, "rollout"))
    one.close(), twin.close()
    return st, so


@pytest.mark.gpu
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_control_loop_kernels_where_receptions_fail(layout):
    _run_case(layout)


@pytest.mark.gpu
@pytest.mark.parametrize("case", TIE_CASES)
def test_control_loop_kernels_at_an_exact_time_tie(case):
    """A counter tick exactly on the end of a data transmission (the tick is the older event: it runs first, the delivery
    after it) or exactly on the end of the step (the tick belongs to the step); GW_FLAG_TIE says that it happened."""
    st, so = _run_case(case)
    opens_fresh = np.isin(so, (0, 6))                                    # {0, 19} as a fresh env's first step
    assert (st["flags"][opens_fresh] & FLAG_TIE).all() and opens_fresh.any()


@pytest.mark.gpu
def test_control_loop_kernels_at_the_smallest_counter_interval():
    """22 ticks and 22 commands in one step: rows 0 - 21 of both staging columns, every lane beside its neighbours."""
    _run_case("gate")


@pytest.mark.gpu
def test_rollout_schedules_where_announcements_are_refused():
    from gymwipe_amd import VecControlLoopEnv
    sch, w_tally, final, taken = schedule_reference()
    n, M = SCHED_N, SCHED_N // SCHED_P
    so, p_of = stream_of(n), np.arange(n) // M
    env_kw = case_of("rrm_edge")[1]

    def make():
        env = VecControlLoopEnv(n, **env_kw)
        env.set_initial_state(T(X0S[so]), T(U0S[so]))
        env.reset_envs()
        return env
    env = make()
    tally, sums = env.rollout_schedules(T(sch), (SCHED_MAX, SCHED_FAIL), K)
    assert_same(tally.cpu().numpy(), w_tally[p_of, so], "tally")
    assert (sums.cpu().numpy()[:, 2] == K * M).all()
    st = state_of(env)
    rows = p_of * STREAMS + so
    for f in FIELDS + ("age", "cost"):
        assert_same(st[f], final[f][rows], f)
    assert not (st["flags"] & 3).any()
    twin = make()                                                        # the same from the schedules expanded to [K][N] actions
    acts = taken[p_of, so]                                               # [n][K][2]
    twin.rollout(T(acts[:, :, 0].T), T(acts[:, :, 1].T), episodes=(SCHED_MAX, SCHED_FAIL))
    assert_states_equal(state_of(twin), st, "expanded")
    env.close(), twin.close()
