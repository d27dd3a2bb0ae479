"""Per-env PID gains of the control loop on the GPU (gw_ctrl_set_gains): the PID instantiations of the step kernel and of the
fused rollout kernels against the event-driven model of tests/ctrl_pid_model.py, bit for bit, over every state field and the
controller's own two (``gains``, ``last_error``).  A reset env is a freshly constructed model with the same gains.  The
fixtures are defined in tests/ctrl_pid_model.py and qualified on the model alone in tests/test_ctrl_gains_cpu.py (every gain
matters, a kept last error would show, both ending causes occur).  Every test calls ``set_gains``: none passes without it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctrl_pid_model as pm
import test_ctrl_rollout as g
from test_control_loop import DENSE_CTRL, stream_of
from test_ctrl_rollout import ALL_FIELDS, FIELDS, T, assert_same

PID_FIELDS = ALL_FIELDS + ("gains", "last_error")
MODEL_FIELDS = FIELDS + ("gains", "last_error")
GAINS = pm.gains_array()


def state_of(env, fields=PID_FIELDS):
    return {f: env.get_state(f) for f in fields}


def assert_states_equal(a, b, what, fields=PID_FIELDS):
    for f in fields:
        assert_same(a[f], b[f], (what, f))


def step_layout(N):
    """The step cases' envs: stream ``stream_of(e)``, gain set ``(e // 8) % 8`` -- the first 64 envs are the 64 pairs."""
    return (np.arange(N) // 8) % pm.G, stream_of(N)


def step_env(N, start, period, plant=None, gains=None):
    from gymwipe_amd import VecControlLoopEnv
    kw = {} if plant is None else {"A": DENSE_CTRL["A"], "B": DENSE_CTRL["B"], "x0": DENSE_CTRL["x0"], "u0": DENSE_CTRL["u0"]}
    return VecControlLoopEnv(N, ctrl_start_tick=start, ctrl_period_ticks=period, gains=gains, **kw)


def fused_env(switch=True):
    """512 envs on the fused cases' layout: every env starts from its stream's X0S / U0S under its gain set."""
    from gymwipe_amd import VecControlLoopEnv, actions
    _, _, _, so = pm.fused_layout()
    env = VecControlLoopEnv(pm.N_FUSED, ctrl_start_tick=g.START, ctrl_period_ticks=g.PERIOD)
    env.set_initial_state(T(g.X0S[so]), T(g.U0S[so]))
    env.reset_envs()
    if switch:
        env.set_gains(actions.make_ctrl_gains(pm.GAIN_SETS, pm.N_FUSED, pm.PER_SET))
    return env


# ---- 1. step -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("plant", [None, "dense"])
@pytest.mark.parametrize("seed,start,period", [(1, 20, 10), (2, 0, 3), (3, 50, 1)])
def test_step_with_per_env_gains_matches_the_model(seed, start, period, plant):
    N, K = 70, 70                                        # one full block and a partial one
    gi, so = step_layout(N)
    dev, dur, steps = pm.step_streams(plant, K, seed, start, period)
    env = step_env(N, start, period, plant, gains=T(GAINS[gi]))
    assert_same(env.get_state("gains"), GAINS[gi], "gains at construction")
    for k in range(K):
        obs, rew, done, info = env.step({"device": T(dev[k][so]), "duration": T(dur[k][so])})
        want = steps[k]
        got = {"obs": obs.cpu().numpy(), "rew": rew.cpu().numpy(), "ang": info["Sensor angle"].cpu().numpy()}
        got.update(state_of(env, MODEL_FIELDS))
        for f, w in want.items():
            assert_same(got[f], w[gi, so], (f, k))
        assert not done.any()
    assert not (env.get_state("flags") & 3).any()
    assert (env.get_state("commands") > 0).all() and (env.get_state("last_error") != 0).all()
    env.close()


# ---- 2. gains (1, 0, 0) are the unswitched handle --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_default_gains_set_explicitly_equal_a_handle_that_never_set_any():
    one, two = fused_env(switch=False), fused_env(switch=False)
    one.set_gains((1.0, 0.0, 0.0))                       # one set is broadcast; `two` stays on the kernels without gains
    _, _, _, so = pm.fused_layout()
    dev, dur = pm.episode_actions()
    d, u = T(dev[:, so]), T(dur[:, so])
    fields = tuple(f for f in PID_FIELDS if f != "last_error")

    def same_state(what):
        a, b = state_of(one), state_of(two)
        assert_states_equal(a, b, what, fields)
        assert (b["last_error"] == 0).all(), what        # never read, never written
        return a["last_error"]

    for k in range(12):
        a, b = one.step({"device": d[k], "duration": u[k]}), two.step({"device": d[k], "duration": u[k]})
        for x, y in ((a[0], b[0]), (a[1], b[1]), (a[3]["Sensor angle"], b[3]["Sensor angle"])):
            assert_same(x.cpu().numpy(), y.cpu().numpy(), ("step", k))
    moved = same_state("step")
    assert (moved != 0).sum() > 100
    a, b = one.rollout(d[12:], u[12:], episodes=(pm.SHORT_MAX_STEPS, pm.FAIL_DEG)), two.rollout(d[12:], u[12:], episodes=(pm.SHORT_MAX_STEPS, pm.FAIL_DEG))
    for x, y in ((a[0], b[0]), (a[1], b[1]), (a[2], b[2]), (a[3]["Sensor angle"], b[3]["Sensor angle"])):
        assert_same(x.cpu().numpy(), y.cpu().numpy(), "rollout")
    assert a[2].any()
    same_state("rollout")
    sch = T(g.schedules_of(pm.P, pm.ROLLOUT_L))
    a, b = one.rollout_schedules(sch, (pm.MAX_STEPS, pm.FAIL_DEG), 40), two.rollout_schedules(sch, (pm.MAX_STEPS, pm.FAIL_DEG), 40)
    assert_same(a[0].cpu().numpy(), b[0].cpu().numpy(), "schedules")
    same_state("schedules")
    sched, edges = pm.feedback_policies()
    a = one.rollout_feedback(T(sched), T(edges), (pm.MAX_STEPS, pm.FAIL_DEG), 40, record=True)
    b = two.rollout_feedback(T(sched), T(edges), (pm.MAX_STEPS, pm.FAIL_DEG), 40, record=True)
    assert_same(a[0].cpu().numpy(), b[0].cpu().numpy(), "feedback")
    for f in a[2]:
        assert_same(a[2][f].cpu().numpy(), b[2][f].cpu().numpy(), ("feedback", f))
    a, b = one.rollout_feedback(T(sched), T(edges), (pm.MAX_STEPS, pm.FAIL_DEG), 20), two.rollout_feedback(T(sched), T(edges), (pm.MAX_STEPS, pm.FAIL_DEG), 20)
    assert_same(a[0].cpu().numpy(), b[0].cpu().numpy(), "feedback without rows")
    moved = same_state("feedback")
    assert (moved != 0).sum() > 100
    one.close(), two.close()


# ---- 3. the fused rollouts with per-env gains -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("max_steps", [pm.MAX_STEPS, pm.SHORT_MAX_STEPS])
def test_rollout_with_per_env_gains_matches_the_wrapper(max_steps):
    K = pm.STEPS
    _, gi, _, so = pm.fused_layout()
    dev, dur, w_obs, w_rew, w_ang, w_ended, final = pm.episode_streams(max_steps)
    d, u = T(dev[:, so]), T(dur[:, so])
    env = fused_env()
    obs, rew, ended, info = env.rollout(d, u, episodes=(max_steps, pm.FAIL_DEG))
    assert_same(ended.cpu().numpy(), w_ended[:, gi, so], "ended")
    assert_same(obs.cpu().numpy(), w_obs[:, gi, so], "obs") and assert_same(rew.cpu().numpy(), w_rew[:, gi, so], "reward")
    assert_same(info["Sensor angle"].cpu().numpy(), w_ang[:, gi, so], "angle")
    st = state_of(env)
    for f in MODEL_FIELDS + ("age", "cost"):
        assert_same(st[f], final[f][gi, so], f)
    assert not (st["flags"] & 3).any()
    halves = fused_env()                                 # two calls of K / 2: last_error is handle state, as age and cost are
    a = halves.rollout(d[:K // 2], u[:K // 2], episodes=(max_steps, pm.FAIL_DEG))
    b = halves.rollout(d[K // 2:], u[K // 2:], episodes=(max_steps, pm.FAIL_DEG))
    assert_same(np.concatenate([a[3]["Sensor angle"].cpu().numpy(), b[3]["Sensor angle"].cpu().numpy()]), w_ang[:, gi, so], "halves")
    assert_states_equal(state_of(halves), st, "halves")
    env.close(), halves.close()


@pytest.mark.gpu
@pytest.mark.parametrize("max_steps", [pm.MAX_STEPS, pm.SHORT_MAX_STEPS])
def test_rollout_schedules_with_per_env_gains_matches_the_wrapper(max_steps):
    K = pm.STEPS
    pi, gi, bi, _ = pm.fused_layout()
    sch, w_tally, final, _, _ = pm.schedule_streams(max_steps)
    env = fused_env()
    tally, sums = env.rollout_schedules(T(sch), (max_steps, pm.FAIL_DEG), K)
    tally = tally.cpu().numpy()
    assert_same(tally, w_tally[pi, gi, bi], "tally")
    assert sums.shape == (pm.P, 4)
    st = state_of(env)
    for f in MODEL_FIELDS + ("age", "cost"):
        assert_same(st[f], final[f][pi, gi, bi], f)
    halves = fused_env()
    a, _ = halves.rollout_schedules(T(sch), (max_steps, pm.FAIL_DEG), K // 2)
    b, _ = halves.rollout_schedules(T(sch), (max_steps, pm.FAIL_DEG), K // 2)
    assert_same((a + b).cpu().numpy()[:, :3], tally[:, :3], "halves' counts")
    assert_states_equal(state_of(halves), st, "halves")
    env.close(), halves.close()


@pytest.mark.gpu
@pytest.mark.parametrize("max_steps", [pm.MAX_STEPS, pm.SHORT_MAX_STEPS])
def test_rollout_feedback_with_per_env_gains_matches_the_wrapper(max_steps):
    K = pm.STEPS
    pi, gi, bi, _ = pm.fused_layout()
    sched, edges = pm.feedback_policies()
    w_tally, w_rows, final = pm.feedback_streams(max_steps)
    env = fused_env()
    tally, sums, rows = env.rollout_feedback(T(sched), T(edges), (max_steps, pm.FAIL_DEG), K, abs_key=True, record=True)
    assert_same(tally.cpu().numpy(), w_tally[pi, gi, bi], "tally")
    for f in ("device", "duration", "obs", "reward", "angle", "ended"):
        assert_same(rows[f].cpu().numpy(), w_rows[f][:, pi, gi, bi], ("rows", f))
    st = state_of(env)
    for f in MODEL_FIELDS + ("age", "cost"):
        assert_same(st[f], final[f][pi, gi, bi], f)
    halves = fused_env()                                 # without rows: the other kernel
    a, _ = halves.rollout_feedback(T(sched), T(edges), (max_steps, pm.FAIL_DEG), K // 2)
    b, _ = halves.rollout_feedback(T(sched), T(edges), (max_steps, pm.FAIL_DEG), K // 2)
    assert_same((a + b).cpu().numpy()[:, (0, 1, 2, 4, 7)], w_tally[pi, gi, bi][:, (0, 1, 2, 4, 7)], "halves' counts")
    assert_states_equal(state_of(halves), st, "halves")
    env.close(), halves.close()


# ---- 4. set_gains with a mask, mid-run -------------------------------------------------------------------------------------------------
MASKED = (5, 6, 7, 40, 63, 64, 69)                     # inside the full block, its last lane, the partial block's first and last
NEW_GAINS = (0.07, 0.015, 0.12)


def _masked_models(K0, K, start, period, reset=False):
    """The masked envs' models after K0 steps under their old gains and K - K0 more under NEW_GAINS (``reset``: as fresh
    models under their old gains instead).  Returns {field: [len(MASKED)]...}."""
    gi, so = step_layout(70)
    dev, dur, _ = pm.step_streams(None, K, 1, start, period)
    states = []
    for e in MASKED:
        m = pm.PidControlLoopModel(start=start, period=period, gains=pm.GAIN_SETS[gi[e]])
        for k in range(K):
            if k == K0:
                if reset:
                    m = pm.PidControlLoopModel(start=start, period=period, gains=pm.GAIN_SETS[gi[e]])
                else:
                    m.gains = NEW_GAINS
            m.step(int(dev[k, so[e]]), int(dur[k, so[e]]))
        states.append(m.snapshot())
    out = {f: np.array([s[f] for s in states], np.float64) for f in ("now", "x", "u", "angle_deg", "rx_power", "gains", "last_error")}
    out["qlen"] = np.array([s["qlen"][:2] for s in states], np.int64)
    out["received"] = np.array([s["received"][1:] for s in states], np.int64)
    for f in ("n_tx", "commands", "substeps"):
        out[f] = np.array([s[f] for s in states], np.int64)
    return out


@pytest.mark.gpu
def test_set_gains_with_a_mask_mid_run_touches_the_masked_gains_and_nothing_else():
    N, K0, K, start, period = 70, 35, 70, 20, 10
    gi, so = step_layout(N)
    dev, dur, steps = pm.step_streams(None, K, 1, start, period)
    env = step_env(N, start, period, gains=T(GAINS[gi]))
    for k in range(K0):
        env.step({"device": T(dev[k][so]), "duration": T(dur[k][so])})
    before = state_of(env)
    assert (before["last_error"] != 0).any()
    mask = np.zeros(N, np.uint8)
    mask[list(MASKED)] = 1
    m = mask.astype(bool)
    env.set_gains(NEW_GAINS, mask=T(mask))
    after = state_of(env)
    for f in PID_FIELDS:
        if f != "gains":
            assert_same(after[f], before[f], ("running state", f))
    assert_same(after["gains"][~m], before["gains"][~m], "other envs' gains")
    assert_same(after["gains"][m], np.tile(NEW_GAINS, (m.sum(), 1)), "masked gains")
    for k in range(K0, K):
        env.step({"device": T(dev[k][so]), "duration": T(dur[k][so])})
    st = state_of(env, MODEL_FIELDS)
    want = _masked_models(K0, K, start, period)
    for f in MODEL_FIELDS:
        assert_same(st[f][~m], steps[-1][f][gi, so][~m], ("other envs", f))       # as if nothing had happened
        assert_same(st[f][m], want[f], ("masked envs", f))                         # their own past, the new gains from K0 on
    assert (st["x"][m] != steps[-1]["x"][gi, so][m]).any()
    env.close()


# ---- 5. reset ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_reset_clears_the_last_error_of_the_masked_envs_and_keeps_their_gains():
    N, K0, K, start, period = 70, 35, 70, 20, 10
    gi, so = step_layout(N)
    dev, dur, steps = pm.step_streams(None, K, 1, start, period)
    env = step_env(N, start, period)
    env.set_gains(T(GAINS[gi]))
    for k in range(K0):
        env.step({"device": T(dev[k][so]), "duration": T(dur[k][so])})
    before = state_of(env)
    assert (before["last_error"][list(MASKED)] != 0).all()
    mask = np.zeros(N, np.uint8)
    mask[list(MASKED)] = 1
    m = mask.astype(bool)
    env.reset_envs(T(mask))
    after = state_of(env)
    for f in PID_FIELDS:
        assert_same(after[f][~m], before[f][~m], ("untouched", f))
    assert (after["last_error"][m] == 0).all() and (after["now"][m] == 0).all()
    assert_same(after["gains"], before["gains"], "the gains survive a reset")
    for k in range(K0, K):
        env.step({"device": T(dev[k][so]), "duration": T(dur[k][so])})
    st = state_of(env, MODEL_FIELDS)
    want = _masked_models(K0, K, start, period, reset=True)
    for f in MODEL_FIELDS:
        assert_same(st[f][~m], steps[-1][f][gi, so][~m], ("other envs", f))
        assert_same(st[f][m], want[f], ("reset envs: fresh models with their gains", f))
    env.close()


# ---- 6. refusals and surface ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_set_gains_refusals_come_before_any_launch_and_the_env_has_the_new_verbs():
    import torch
    import gymwipe_amd
    from gymwipe_amd import _native as nat
    N = 128
    env = gymwipe_amd.make("VecControlLoop-v0", num_envs=N)
    assert callable(env.set_gains)
    for f, shape in (("gains", (N, 3)), ("last_error", (N,))):
        assert env.get_state(f).shape == shape and env.get_state(f).dtype == np.float64
    assert (env.get_state("gains") == [1.0, 0.0, 0.0]).all() and (env.get_state("last_error") == 0).all()
    L = nat.lib()
    some = torch.zeros((N, 3), dtype=torch.float64, device="cuda")
    before = state_of(env)
    assert L.gw_ctrl_set_gains(None, some.data_ptr(), None, None) == nat.EINVAL
    assert L.gw_ctrl_set_gains(env._h, None, None, None) == nat.EINVAL
    with pytest.raises(nat.NativeError) as err:
        nat.check(L.gw_ctrl_set_gains(env._h, None, None, None))
    assert err.value.code == nat.EINVAL and "gains_dev" in str(err.value)
    for bad in ([1.0, 0.0], np.zeros((N - 1, 3)), np.zeros((N, 4))):
        with pytest.raises(ValueError):
            env.set_gains(bad)
    assert_states_equal(state_of(env), before, "refused")
    env.set_gains(np.tile([0.5, 0.25, 0.125], (N, 1)), mask=torch.arange(N) < 64)         # a host array, a mask on the host
    env.set_gains(torch.full((N, 3), 2.0, dtype=torch.float64, device="cuda"), mask=np.arange(N) >= 96)
    want = np.where((np.arange(N) < 64)[:, None], [0.5, 0.25, 0.125], np.where((np.arange(N) >= 96)[:, None], 2.0, [1.0, 0.0, 0.0]))
    assert_same(env.get_state("gains"), want, "gains")
    buf = np.empty(N * 2)                                 # a wrong size is refused, as for every field
    assert L.gw_ctrl_get_state(env._h, b"gains", buf.ctypes.data, buf.nbytes) == nat.EFIELD
    env.close()
    env = gymwipe_amd.make("VecControlLoop-v0", num_envs=N, gains=(0.1, 0.0, 0.2))
    assert (env.get_state("gains") == [0.1, 0.0, 0.2]).all()
    env.close()
