"""Test infrastructure, not a test: what tests/test_ctrl_gains.py, tests/test_ctrl_disturbance.py and tests/test_ctrl_loss.py do
alike, once, parametrised by the tier of tests/ctrl_tiers.py -- the handles on the fixtures' layouts, the comparison of a
handle's state with a reference, and the bodies of the test shapes the three files share.  A body runs the handle against the
tier's reference, asserts what holds for every tier and returns what it measured; the assertions that belong to one tier alone
stand in that tier's test.  Nothing here touches the GPU at import."""
import collections
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctrl_dist_model as cd
import ctrl_loss_model as lm
import ctrl_pid_model as pm
import ctrl_tiers as ct
from ctrl_fixtures import ALL_FIELDS, FIELDS, LAYOUTS, PERIOD, START, U0S, X0S, T, assert_same, dense_kw, schedules_of, stream_of

GAINS, WEIGHTS, THR, PROBS = pm.gains_array(), cd.g_array(), lm.thr_array(), np.array(lm.P_SETS, np.float64)
N70, K70, K0 = 70, 70, 35                                # the step cases: one full block and a partial one; the mid-run point


def new_names(tier):
    return tuple(f for f, _ in ct.new_fields(tier))


def state_fields(tier):
    return ALL_FIELDS + new_names(tier)


def model_fields(tier):
    return FIELDS + new_names(tier)


def state_of(tier, env, fields=None):
    return {f: env.get_state(f) for f in (state_fields(tier) if fields is None else fields)}


def assert_states_equal(tier, a, b, what, fields=None):
    for f in state_fields(tier) if fields is None else fields:
        assert_same(a[f], b[f], (what, f))


def check_final(tier, st, final, index, what):
    for f in model_fields(tier) + ("age", "cost"):
        assert_same(st[f], final[f][index], (what, f))
    assert not (st["flags"] & 3).any(), what


# ---- handles on the fixtures' layouts -------------------------------------------------------------------------------------------------------
def step_layout(tier, N):
    """The step cases' envs: action stream ``stream_of(e)``, gain, weight and loss set ``(e // 8) % 8`` -- the first 64 envs are
    the 64 pairs -- and the pair's own noise key and loss key (None below the tier that has one).  Returns (gi, so, nkey, lkey)."""
    from gymwipe_amd import actions
    gi, so = (np.arange(N) // 8) % ct.G, stream_of(N)
    nkey = lkey = None
    if ct.DISTURBANCE in tier.blocks:
        nkey = actions.make_ctrl_disturbance(np.zeros(4), N, seed=cd.SEED, streams=gi * 8 + so)[1]
    if ct.LOSS_BLOCK in tier.blocks:
        lkey = actions.make_ctrl_loss(np.zeros(4), N, seed=lm.SEED, streams=gi * 8 + so)[1]
    return gi, so, nkey, lkey


def step_env(tier, N, start, period, plant=None, layout=None, gains=True):
    """N envs on the step cases' layout, every block of the tier set.  ``gains=False``: the gains are left to the caller."""
    from gymwipe_amd import VecControlLoopEnv
    gi, _, nkey, lkey = step_layout(tier, N)
    kw = dense_kw(plant)
    if layout is not None:
        pos, rrm = LAYOUTS[layout]
        kw["positions"] = pos + (rrm,)
    env = VecControlLoopEnv(N, ctrl_start_tick=start, ctrl_period_ticks=period, gains=T(GAINS[gi]) if gains else None, **kw)
    if nkey is not None:
        env.set_disturbance(T(WEIGHTS[gi]), nkey)
    if lkey is not None:
        env.set_loss(PROBS[gi], lkey)
    return env


def fused_env(tier=None):
    """512 envs on the fused cases' layout: every env starts from its stream's X0S / U0S under its gain set, its weights, its loss
    set and its model's keys -- as far as the tier goes; None: a handle no block was set on."""
    from gymwipe_amd import VecControlLoopEnv, actions
    _, gi, _, so = pm.fused_layout()
    env = VecControlLoopEnv(pm.N_FUSED, ctrl_start_tick=START, ctrl_period_ticks=PERIOD)
    env.set_initial_state(T(X0S[so]), T(U0S[so]))
    env.reset_envs()
    blocks = () if tier is None else tier.blocks
    if ct.GAINS in blocks:
        env.set_gains(actions.make_ctrl_gains(pm.GAIN_SETS, pm.N_FUSED, pm.PER_SET))
    if ct.DISTURBANCE in blocks:
        env.set_disturbance(actions.make_ctrl_disturbance(cd.G_SETS, pm.N_FUSED, envs_per_set=pm.PER_SET)[0], ct.fused_keys(cd.SEED64))
    if ct.LOSS_BLOCK in blocks:
        thr, _ = actions.make_ctrl_loss(lm.P_SETS, pm.N_FUSED, envs_per_set=pm.PER_SET)
        assert_same(thr, THR[gi], "the helper's thresholds are the model's")
        env.set_loss(PROBS[gi], ct.fused_keys(lm.SEED64))
    return env


def fused_index(tier, episodes=False):
    """The index of every fused env into a reference's arrays: (p, gi, b), or (gi, stream) for the staged-action reference of
    a tier laid out by stream."""
    pi, gi, bi, so = pm.fused_layout()
    return (gi, so) if episodes and tier.by_stream else (pi, gi, bi)


def masked(N, envs):
    mask = np.zeros(N, np.uint8)
    mask[list(envs)] = 1
    return mask, mask.astype(bool)


# ---- step against the model ---------------------------------------------------------------------------------------------------------------
def run_steps(tier, env, ref, gi, so, k0, k1, every=True):
    """Steps k0 .. k1 - 1 of a step reference through ``env.step``; ``every``: compared with the model after every step, in
    every output and model field.  Returns what the handle gave per step, [{field: ...}]."""
    seen = []
    for k in range(k0, k1):
        obs, rew, done, info = env.step({"device": T(ref.dev[k][so]), "duration": T(ref.dur[k][so])})
        if not every:
            continue
        got = {"obs": obs.cpu().numpy(), "rew": rew.cpu().numpy(), "ang": info["Sensor angle"].cpu().numpy()}
        got.update(state_of(tier, env, model_fields(tier)))
        for f, w in ref.steps[k].items():
            assert_same(got[f], w[gi, so], (f, k))
        assert not done.any()
        seen.append(got)
    return seen


StepRun = collections.namedtuple("StepRun", "gi so nkey lkey first seen final")


def step_matches_the_model(tier, K, seed, start, period, plant=None, layout=None):
    """70 envs, K steps, every step against the model.  Returns the layout, the tier's fields as the handle was set up, what it
    gave per step and its state after the last."""
    gi, so, nkey, lkey = step_layout(tier, N70)
    ref = ct.step_streams(tier, plant, K, seed, start, period, layout=layout)
    env = step_env(tier, N70, start, period, plant, layout)
    first = state_of(tier, env, new_names(tier))
    seen = run_steps(tier, env, ref, gi, so, 0, K)
    final = state_of(tier, env)
    env.close()
    return StepRun(gi, so, nkey, lkey, first, seen, final)


def rollout_at_seventy_envs(tier):
    """The step reference through one fused launch of 70 envs: a partial block in the rollout kernel."""
    seed, start, period = 1, 20, 10
    gi, so, _, _ = step_layout(tier, N70)
    ref = ct.step_streams(tier, None, K70, seed, start, period)
    env = step_env(tier, N70, start, period)
    obs, rew, done, info = env.rollout(T(ref.dev[:, so]), T(ref.dur[:, so]))
    assert_same(obs.cpu().numpy(), np.array([w["obs"][gi, so] for w in ref.steps]), "obs")
    assert_same(rew.cpu().numpy(), np.array([w["rew"][gi, so] for w in ref.steps]), "reward")
    assert_same(info["Sensor angle"].cpu().numpy(), np.array([w["ang"][gi, so] for w in ref.steps]), "angle")
    assert not done.any()
    st = state_of(tier, env, model_fields(tier))
    for f in model_fields(tier):
        assert_same(st[f], ref.steps[-1][f][gi, so], f)
    env.close()
    return st


# ---- the fused rollouts, and K / 2 + K / 2 = K ------------------------------------------------------------------------------------------------
Fused = collections.namedtuple("Fused", "st mid")         # the state after K steps, and the halves' after K / 2


def rollout_matches_the_wrapper(tier, max_steps):
    K = ct.STEPS
    ix, so = fused_index(tier, episodes=True), pm.fused_layout()[3]
    ref = ct.episode_streams(tier, max_steps)
    d, u = T(ref.dev[:, so]), T(ref.dur[:, so])
    env = fused_env(tier)
    obs, rew, ended, info = env.rollout(d, u, episodes=(max_steps, ct.FAIL_DEG))
    assert_same(ended.cpu().numpy(), ref.ended[(slice(None),) + ix], "ended")
    assert_same(obs.cpu().numpy(), ref.obs[(slice(None),) + ix], "obs") and assert_same(rew.cpu().numpy(), ref.rew[(slice(None),) + ix], "reward")
    assert_same(info["Sensor angle"].cpu().numpy(), ref.ang[(slice(None),) + ix], "angle")
    st = state_of(tier, env)
    check_final(tier, st, ref.final, ix, "rollout")
    halves = fused_env(tier)                             # two calls of K / 2: the tier's records are handle state, as age and cost are
    a = halves.rollout(d[:K // 2], u[:K // 2], episodes=(max_steps, ct.FAIL_DEG))
    mid = state_of(tier, halves)
    b = halves.rollout(d[K // 2:], u[K // 2:], episodes=(max_steps, ct.FAIL_DEG))
    assert_same(np.concatenate([a[3]["Sensor angle"].cpu().numpy(), b[3]["Sensor angle"].cpu().numpy()]), ref.ang[(slice(None),) + ix], "halves")
    assert_states_equal(tier, state_of(tier, halves), st, "halves")
    env.close(), halves.close()
    return Fused(st, mid)


def rollout_schedules_matches_the_wrapper(tier, max_steps):
    K = ct.STEPS
    ix = fused_index(tier)
    ref = ct.schedule_streams(tier, max_steps)
    env = fused_env(tier)
    tally, sums = env.rollout_schedules(T(ref.sch), (max_steps, ct.FAIL_DEG), K)
    tally = tally.cpu().numpy()
    assert_same(tally, ref.tally[ix], "tally")
    assert sums.shape == (pm.P, 4)
    st = state_of(tier, env)
    check_final(tier, st, ref.final, ix, "schedules")
    halves = fused_env(tier)
    a, _ = halves.rollout_schedules(T(ref.sch), (max_steps, ct.FAIL_DEG), K // 2)
    mid = state_of(tier, halves)
    b, _ = halves.rollout_schedules(T(ref.sch), (max_steps, ct.FAIL_DEG), K // 2)
    assert_same((a + b).cpu().numpy()[:, :3], tally[:, :3], "halves' counts")
    assert_states_equal(tier, state_of(tier, halves), st, "halves")
    env.close(), halves.close()
    return Fused(st, mid)


def rollout_feedback_matches_the_wrapper(tier, max_steps):
    K = ct.STEPS
    ix = fused_index(tier)
    sched, edges = pm.feedback_policies()
    ref = ct.feedback_streams(tier, max_steps)
    env = fused_env(tier)
    tally, sums, rows = env.rollout_feedback(T(sched), T(edges), (max_steps, ct.FAIL_DEG), K, abs_key=True, record=True)
    tally = tally.cpu().numpy()
    assert_same(tally, ref.tally[ix], "tally")
    for f in ("device", "duration", "obs", "reward", "angle", "ended"):
        assert_same(rows[f].cpu().numpy(), ref.rows[f][(slice(None),) + ix], ("rows", f))
    st = state_of(tier, env)
    check_final(tier, st, ref.final, ix, "feedback")
    halves = fused_env(tier)                             # without rows: the other kernel, in two calls of K / 2
    a, _ = halves.rollout_feedback(T(sched), T(edges), (max_steps, ct.FAIL_DEG), K // 2)
    mid = state_of(tier, halves)
    b, _ = halves.rollout_feedback(T(sched), T(edges), (max_steps, ct.FAIL_DEG), K // 2)
    assert_same((a + b).cpu().numpy()[:, (0, 1, 2, 4, 7)], ref.tally[ix][:, (0, 1, 2, 4, 7)], "halves' counts")
    assert_states_equal(tier, state_of(tier, halves), st, "halves")
    env.close(), halves.close()
    return Fused(st, mid)


# ---- "zero X equals the tier below": one call on two handles, the outputs compared -----------------------------------------------------------
def fused_actions():
    """The staged-action case's actions laid out on the fused envs, as tensors [K][512]."""
    so = pm.fused_layout()[3]
    dev, dur = pm.episode_actions()
    return T(dev[:, so]), T(dur[:, so])


def twin_steps(one, two, d, u, k0, k1):
    for k in range(k0, k1):
        a, b = one.step({"device": d[k], "duration": u[k]}), two.step({"device": d[k], "duration": u[k]})
        for x, y in ((a[0], b[0]), (a[1], b[1]), (a[3]["Sensor angle"], b[3]["Sensor angle"])):
            assert_same(x.cpu().numpy(), y.cpu().numpy(), ("step", k))


def twin_rollout(one, two, d, u, what="rollout"):
    """Returns ``one``'s ``ended``."""
    ep = (pm.SHORT_MAX_STEPS, pm.FAIL_DEG)
    a, b = one.rollout(d, u, episodes=ep), two.rollout(d, u, episodes=ep)
    for x, y in ((a[0], b[0]), (a[1], b[1]), (a[2], b[2]), (a[3]["Sensor angle"], b[3]["Sensor angle"])):
        assert_same(x.cpu().numpy(), y.cpu().numpy(), what)
    return a[2]


def twin_schedules(one, two):
    sch = T(schedules_of(pm.P, pm.ROLLOUT_L))
    a, b = one.rollout_schedules(sch, (pm.MAX_STEPS, pm.FAIL_DEG), 40), two.rollout_schedules(sch, (pm.MAX_STEPS, pm.FAIL_DEG), 40)
    assert_same(a[0].cpu().numpy(), b[0].cpu().numpy(), "schedules")


def twin_feedback(one, two, record):
    sched, edges = pm.feedback_policies()
    if record:
        a = one.rollout_feedback(T(sched), T(edges), (pm.MAX_STEPS, pm.FAIL_DEG), 40, record=True)
        b = two.rollout_feedback(T(sched), T(edges), (pm.MAX_STEPS, pm.FAIL_DEG), 40, record=True)
        assert_same(a[0].cpu().numpy(), b[0].cpu().numpy(), "feedback")
        for f in a[2]:
            assert_same(a[2][f].cpu().numpy(), b[2][f].cpu().numpy(), ("feedback", f))
    else:
        a, b = one.rollout_feedback(T(sched), T(edges), (pm.MAX_STEPS, pm.FAIL_DEG), 20), two.rollout_feedback(T(sched), T(edges), (pm.MAX_STEPS, pm.FAIL_DEG), 20)
        assert_same(a[0].cpu().numpy(), b[0].cpu().numpy(), "feedback without rows")


# ---- equal keys, equal trajectories -------------------------------------------------------------------------------------------------------
A, B, C = 3, 200, 70                                     # lanes 3, 8 and 6 of blocks 0, 3 and 1


def equal_records_walk_equal_trajectories(tier, differ):
    """256 envs of their own actions, initial states, gains and keys; B is A's copy in everything, C as well but for what
    ``differ(weights, nkey, lkey)`` changes at index C.  Returns the angles [K][N] and the final state."""
    from gymwipe_amd import VecControlLoopEnv, actions
    N, K = 256, 40
    rng = np.random.default_rng(11)
    dev = rng.integers(0, 2, (K, N)).astype(np.int32)
    dur = rng.integers(0, 20, (K, N)).astype(np.int32)
    x0 = rng.uniform(-0.3, 0.3, (N, 4))
    gains = np.tile([0.1, 0.0, 0.05], (N, 1)) * rng.uniform(0.5, 1.5, (N, 1))
    weights, nkey = actions.make_ctrl_disturbance((0.001, 0.0, 0.0005, 0.01), N, seed=77)
    p = np.tile([0.3, 0.2, 0.4, 0.25], (N, 1))
    _, lkey = actions.make_ctrl_loss(np.zeros(4), N, seed=78)
    for e in (B, C):
        dev[:, e], dur[:, e], x0[e], gains[e], nkey[e], lkey[e] = dev[:, A], dur[:, A], x0[A], gains[A], nkey[A], lkey[A]
    differ(weights, nkey, lkey)
    env = VecControlLoopEnv(N, ctrl_start_tick=START, ctrl_period_ticks=PERIOD, gains=T(gains))
    env.set_initial_state(T(x0))
    env.reset_envs()
    env.set_disturbance(T(weights), nkey)
    if ct.LOSS_BLOCK in tier.blocks:
        env.set_loss(p, lkey)
    obs, rew, ended, info = env.rollout(T(dev), T(dur), episodes=(pm.SHORT_MAX_STEPS, pm.FAIL_DEG))
    ang = info["Sensor angle"].cpu().numpy()
    assert_same(ang[:, B], ang[:, A], "angles of the pair")
    assert ended[:, A].any()
    st = state_of(tier, env)
    for f in state_fields(tier):
        assert_same(st[f][B], st[f][A], ("the pair", f))
    others = [e for e in range(N) if e not in (A, B, C)]
    assert len({st["x"][e].tobytes() for e in others}) == len(others)
    env.close()
    return ang, st


# ---- a masked set mid-run; what a reset leaves ------------------------------------------------------------------------------------------------
def masked_models(tier, envs, change=None):
    """The models of ``envs`` of the 70-env step case after K0 steps and K70 - K0 more: with ``change(model, e)`` applied
    between (the new record, as the setter leaves it), or, without one, reset there -- the fresh model ``ct.make`` builds from
    the old one.  Returns {field: [len(envs)]...} in get_state's dtypes."""
    start, period = 20, 10
    gi, so, _, _ = step_layout(tier, N70)
    ref = ct.step_streams(tier, None, K70, 1, start, period)
    states = []
    for e in envs:
        cfg = ct.step_cfg(tier, None, start, period, gi[e], so[e])
        m = ct.make(tier, cfg)
        for k in range(K70):
            if k == K0:
                if change is None:
                    m = ct.make(tier, cfg, old=m)
                else:
                    change(m, e)
            m.step(int(ref.dev[k, so[e]]), int(ref.dur[k, so[e]]))
        states.append(ct.snapshot_of(tier, m))
    out = {f: np.array([s[f] for s in states], np.float64) for f in ("now", "x", "u", "angle_deg", "rx_power")}
    out["qlen"] = np.array([s["qlen"][:2] for s in states], np.int64)
    out["received"] = np.array([s["received"][1:] for s in states], np.int64)
    for f in ("n_tx", "commands", "substeps"):
        out[f] = np.array([s[f] for s in states], np.int64)
    for f, dtype in ct.new_fields(tier):
        out[f] = np.array([s[f] for s in states], dtype)
    return out


MidRun = collections.namedtuple("MidRun", "m before after st last")   # the mask, the states around the call, the final one, the reference's


def _mid_run(tier, envs, env, act, change):
    """K0 steps, ``act(env, mask)``, the rest: the envs outside the mask end where the reference does, those inside where
    ``masked_models`` does."""
    start, period = 20, 10
    gi, so, _, _ = step_layout(tier, N70)
    ref = ct.step_streams(tier, None, K70, 1, start, period)
    env = step_env(tier, N70, start, period) if env is None else env
    run_steps(tier, env, ref, gi, so, 0, K0, every=False)
    before = state_of(tier, env)
    mask, m = masked(N70, envs)
    act(env, T(mask))
    after = state_of(tier, env)
    run_steps(tier, env, ref, gi, so, K0, K70, every=False)
    st = state_of(tier, env, model_fields(tier))
    want = masked_models(tier, envs, change)
    last = {f: ref.steps[-1][f][gi, so] for f in model_fields(tier)}
    for f in model_fields(tier):
        assert_same(st[f][~m], last[f][~m], ("other envs", f))                    # as if nothing had happened
        assert_same(st[f][m], want[f], ("masked envs", f))                         # their own past; the new record, or a fresh model
    env.close()
    return MidRun(m, before, after, st, last)


def masked_set_mid_run(tier, envs, setter, change, own):
    """``setter(env, mask)`` after K0 steps touches the fields ``own`` of the masked envs and nothing else; ``change(model, e)``
    is what it does to env e's model."""
    r = _mid_run(tier, envs, None, setter, change)
    for f in state_fields(tier):
        if f not in own:
            assert_same(r.after[f], r.before[f], ("running state", f))
        else:
            assert_same(r.after[f][~r.m], r.before[f][~r.m], ("other envs", f))
    return r


def reset_mid_run(tier, envs, env=None):
    """``reset_envs(mask)`` after K0 steps leaves the other envs alone, and the masked ones go on as fresh models that carry
    what the tier's reset carries."""
    r = _mid_run(tier, envs, env, lambda env, mask: env.reset_envs(mask), None)
    for f in state_fields(tier):
        assert_same(r.after[f][~r.m], r.before[f][~r.m], ("untouched", f))
    return r


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def refusals_come_before_any_launch(tier, verb, fields, pointers, words, bad):
    """A fresh 128-env handle has ``verb`` and the block's ``fields`` ((name, shape, dtype)...); the native call refuses a null
    handle and each null pointer of ``pointers`` (device tensors, in argument order; ``words``: what each refusal's message
    names), the method refuses every argument tuple of ``bad``, and none of it touches the state.  Returns the env and the
    library."""
    import pytest
    import gymwipe_amd
    from gymwipe_amd import _native as nat
    env = gymwipe_amd.make("VecControlLoop-v0", num_envs=128)
    assert callable(getattr(env, verb))
    for f, shape, dt in fields:
        assert env.get_state(f).shape == shape and env.get_state(f).dtype == dt
    L = nat.lib()
    native = getattr(L, "gw_ctrl_" + verb)
    ptrs = [t.data_ptr() for t in pointers]
    before = state_of(tier, env)
    assert native(None, *ptrs, None, None) == nat.EINVAL
    for i, word in enumerate(words):
        args = (env._h,) + tuple(None if j == i else p for j, p in enumerate(ptrs)) + (None, None)
        assert native(*args) == nat.EINVAL
        with pytest.raises(nat.NativeError) as err:
            nat.check(native(*args))
        assert err.value.code == nat.EINVAL and word in str(err.value)
    for args in bad:
        with pytest.raises(ValueError):
            getattr(env, verb)(*args)
    assert_states_equal(tier, state_of(tier, env), before, "refused")
    return env, L
