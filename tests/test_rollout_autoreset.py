"""
gw_rollout_autoreset on the GPU: gw_rollout's pre-staged actions with episodes -- an env whose step returned done, or whose
episode reached its step limit, is reset inside the launch (ct_rollout_sync_ep<DT, MODE>) -- its one-step form
env.step_autoreset(), and the per-step form of every other handle.

Every expected value comes from the oracle alone: CtOracle.step on the staged rows, then actions.episodes_numpy, then
CtOracle.reset(mask) for the envs whose episode ended (oracle_autoreset_steps(): tests/test_rollout_episodes.py's loop with the
draw replaced by the rows).  All comparisons are exact, the state included (STATE_FIELDS + STAT_FIELDS).  autoreset_reference()
raises, instead of letting a test pass, when fewer than MIN_EPISODES episodes end by a cause the case is meant to exercise.
tests/test_rollout_autoreset_cpu.py checks on the CPU that INSTANTIATIONS is exactly the library's set.
"""
import functools

import numpy as np
import pytest

from test_kernel_variants import MODE_SWITCHES, SFX_DTS, launches
from test_rollout_episodes import MAX_STEPS, MIN_EPISODES, new_oracle
from test_rollout_policy import CENTER, K_INST, K_LONG, N, PARITY_DS, SEED, delta, gpu_prep, make_env, policy_table
from util import action_stream, assert_state_equal, STATE_FIELDS, STAT_FIELDS

INSTANTIATIONS = {"ct_rollout_sync_ep<%d, %d>" % (dt, mode): (dt, mode) for dt in SFX_DTS + (0,) for mode in (2, 1, 0)}
NAMES = ("obs", "reward", "done", "ended")
DTYPES = (np.int32, np.float32, np.uint8, np.uint8)
FLAG_BADACT = 8


def oracle_autoreset_steps(orc, dev, dur, state, max_steps, on_done, center=CENTER):
    """The oracle on staged rows with episodes: the four [K][n] outputs, the observation each env acts on next and the episode
    tally; ``state`` ({age, ret}, int32[n][2]) is updated in place."""
    from gymwipe_amd.actions import EP_COLS, episodes_numpy
    K, n = dev.shape
    out = [np.empty((K, n), t) for t in DTYPES]
    tally = np.zeros(EP_COLS, np.int64)
    acts_on = None
    for k in range(K):
        obs, r, dn = orc.step(dev[k], dur[k])
        ended, t = episodes_numpy(state, r, dn, max_steps, on_done)
        tally += t
        if ended.any():
            orc.reset((ended != 0).astype(np.uint8))
        for a, v in zip(out, (obs, r, dn, ended)):
            a[k] = v
        acts_on = np.where(ended != 0, center, obs).astype(np.int32)
    return tuple(out), acts_on, tally


def staged_actions(D, steps, both=False):
    """The parity inputs: seeded uniform rows; `both`: the duration set to 0 in about half of them (with counter_bound = 2 a
    step then delivers nothing and done does not fire, so some episodes reach the step limit)."""
    dev, dur = action_stream(31 + D, steps, N, D)
    if both:
        dur = np.where(np.random.default_rng(131 + D).random((steps, N)) < 0.5, 0, dur).astype(np.int32)
    return dev, dur


def ended_by(tally):
    return {1: int(tally[1]), 2: int(tally[0] - tally[1])}


@functools.lru_cache(maxsize=None)
def autoreset_reference(D, steps=K_LONG, max_steps=MAX_STEPS, on_done=True, both=False, causes=(2,)):
    """The oracle's trajectory over the staged rows after a reset, computed once and read only.  `causes`: the ways an episode
    ends that the case is meant to exercise (1 done, 2 step limit)."""
    bound = 2 if both else None
    dev, dur = staged_actions(D, steps, both)
    orc = new_oracle(D, bound=bound)
    center = CENTER if bound is None else bound
    orc.reset()
    state = np.zeros((N, 2), np.int32)
    out, obs_next, tally = oracle_autoreset_steps(orc, dev, dur, state, max_steps, on_done, center)
    by = ended_by(tally)
    for cause in causes:
        if by[cause] < MIN_EPISODES:
            raise RuntimeError("autoreset_reference(%d, %d): %d episodes ended by cause %d, fewer than %d"
                               % (D, steps, by[cause], cause, MIN_EPISODES))
    assert tally[0] == (out[3] != 0).sum() and tally[1] == (out[3] == 1).sum()
    for a in out + (obs_next, state, tally, dev, dur):
        a.setflags(write=False)
    return {"dev": dev, "dur": dur, "out": out, "obs_next": obs_next, "state": state, "tally": tally, "orc": orc, "center": center}


def assert_outputs(got, want, where, cols=slice(None)):
    assert len(got) == len(want) == 4
    for name, g, w in zip(NAMES, got, want):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w[:, cols].shape, (name, where)
        same = g.view(np.uint8) == np.ascontiguousarray(w[:, cols]).view(np.uint8)
        assert same.all(), "%s differs %s, first at (step, env) %s" % (name, where, np.argwhere(g != w[:, cols])[:3].tolist())


def assert_episodes(env, ref, where, tally=True):
    assert (env._last[0].cpu().numpy() == ref["obs_next"]).all(), "obs_next differs " + where
    assert (env.episode_state.cpu().numpy() == ref["state"]).all(), "{age, ret} differs " + where
    if tally:
        assert env.episode_tally.cpu().numpy().tolist() == ref["tally"].tolist(), "tally differs " + where


def ep_launches(env):
    return {k: v for k, v in launches(env).items() if k.startswith("ct_rollout_")}


def staged(ref, rows=slice(None)):
    import torch
    return torch.tensor(ref["dev"][rows]).cuda(), torch.tensor(ref["dur"][rows]).cuda()    # (copies: the reference is read-only)


def step_outputs(n=N):
    import torch
    from gymwipe_amd import StepOutputs
    return StepOutputs(torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda"),
                       torch.empty(n, dtype=torch.uint8, device="cuda"), ended=torch.empty(n, dtype=torch.uint8, device="cuda"))


# ---- 1. one call ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("D", PARITY_DS)
def test_one_call_matches_the_oracle(D):
    ref = autoreset_reference(D)
    env = make_env(D)
    env.reset()
    got = env.rollout_autoreset(*staged(ref), max_steps=MAX_STEPS)
    assert_outputs(got, ref["out"], "in one call of %d steps" % K_LONG)
    assert_episodes(env, ref, "after the call")
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after the call")
    dt = D if D in SFX_DTS else 0
    assert ep_launches(env) == {"ct_rollout_sync_ep<%d, 2>" % dt: 3}, launches(env)
    stats = env.episode_stats()
    n, by_done, length, ret, sq = (int(x) for x in ref["tally"])
    assert stats["episodes"] == n and stats["by_done"] == by_done and stats["mean_length"] == length / n
    assert stats["mean_return"] == ret / n
    assert abs(stats["return_stderr"] - (max(sq / n - (ret / n) ** 2, 0.0) / n) ** 0.5) <= 1e-12
    env.check()


# ---- 2. both causes -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("on_done", [True, False])
def test_done_and_the_step_limit_both_end_episodes(on_done):
    """counter_bound = 2 at D = 2: a delivered payload reaches the bound, so done fires with the first delivery; a row of
    duration 0 delivers nothing.  on_done=False on the same rows: done never ends an episode."""
    ref = autoreset_reference(2, on_done=on_done, both=True, causes=(1, 2) if on_done else (2,))
    if not on_done:
        assert set(np.unique(ref["out"][3]).tolist()) == {0, 2} and int(ref["out"][2].sum()) >= MIN_EPISODES
    env = make_env(2, counter_bound=2)
    env.reset()
    got = env.rollout_autoreset(*staged(ref), max_steps=MAX_STEPS, on_done=on_done)
    assert_outputs(got, ref["out"], "with both causes (on_done=%s)" % on_done)
    assert_episodes(env, ref, "with both causes (on_done=%s)" % on_done)
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="with both causes (on_done=%s)" % on_done)


# ---- 3. limits off --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_without_limits_it_is_rollout():
    """max_steps = 0, on_done = False on one handle, rollout() on its twin: output for output, and no byte of the two
    snapshots differs that did not differ before the calls (the header's own device addresses)."""
    import torch
    D = 4
    dev, dur = (torch.from_numpy(a).cuda() for a in staged_actions(D, K_LONG))
    env, twin = make_env(D), make_env(D)
    gpu_prep(env, D)
    gpu_prep(twin, D)
    own = env.snapshot() != twin.snapshot()
    assert own.sum() < 4096, own.sum()
    got = env.rollout_autoreset(dev, dur, max_steps=0, on_done=False)
    want = twin.rollout(dev, dur)
    for name, g, w in zip(NAMES, got, want):
        assert (g == w).all(), name
    assert int(got[3].sum()) == 0 and float(got[1].abs().sum()) > 0
    differ = env.snapshot() != twin.snapshot()
    assert not (differ & ~own).any(), np.flatnonzero(differ & ~own)[:8]
    state = env.episode_state.cpu().numpy()
    assert (state[:, 0] == K_LONG).all() and (state[:, 1] == got[1].cpu().numpy().astype(np.int64).sum(axis=0)).all()
    assert (env._last[0] == got[0][-1]).all() and int(env.episode_tally.abs().sum()) == 0


# ---- 4. calls continue one another ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pieces", [(37, 64, 49), (1,) * K_LONG], ids=["37+64+49", "150 steps"])
def test_split_calls_equal_one_call(pieces):
    """{age, ret}, the tally and obs_next are carried in place from call to call; a piece of 1 goes through step_autoreset.
    (The one call of 150 is case 1: all three sequences are compared with the same oracle trajectory.)"""
    import torch
    D = 4
    ref = autoreset_reference(D)
    env = make_env(D)
    env.reset()
    tally0 = np.array([3, 1, 1 << 40, -(1 << 33), 7], np.int64)
    env.episode_tally.copy_(torch.from_numpy(tally0))
    dev, dur = staged(ref)
    rows, s = [], 0
    for n in pieces:
        before = (env.episode_state.data_ptr(), env._last[0].data_ptr() if s else None)
        if n == 1:
            out = step_outputs()
            o, r, d, e, nxt = env.step_autoreset({"device": dev[s], "duration": dur[s]}, max_steps=MAX_STEPS, out=out)
            assert o is out.obs and e is out.ended and nxt is env._last[0]
            rows.append(tuple(t.unsqueeze(0) for t in (o, r, d, e)))
        else:
            rows.append(env.rollout_autoreset(dev[s:s + n], dur[s:s + n], max_steps=MAX_STEPS))
        assert env.episode_state.data_ptr() == before[0] and (before[1] is None or env._last[0].data_ptr() == before[1])
        s += n
    got = tuple(torch.cat([r[i] for r in rows]) for i in range(4))
    assert_outputs(got, ref["out"], "over calls of %s steps" % (pieces[:3],))
    assert_episodes(env, ref, "after the split calls", tally=False)
    assert (env.episode_tally.cpu().numpy() == tally0 + ref["tally"]).all()
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after the split calls")


@pytest.mark.gpu
def test_a_callers_reset_between_two_calls_starts_new_episodes():
    import torch
    D, K1, K2 = 4, 23, 41
    dev, dur = staged_actions(D, K1 + K2)
    mask = (np.random.default_rng(5).random(N) < 0.5).astype(np.uint8)
    orc = new_oracle(D)
    orc.reset()
    state = np.zeros((N, 2), np.int32)
    want1, _, tally1 = oracle_autoreset_steps(orc, dev[:K1], dur[:K1], state, MAX_STEPS, True)
    assert (state[mask != 0, 0] != 0).any()                            # (the reset below zeroes ages that were not zero)
    orc.reset(mask)
    state[mask != 0] = 0
    want2, acts_on, tally2 = oracle_autoreset_steps(orc, dev[K1:], dur[K1:], state, MAX_STEPS, True)
    if tally1[0] + tally2[0] < MIN_EPISODES:
        raise RuntimeError("%d episodes ended, fewer than %d" % (tally1[0] + tally2[0], MIN_EPISODES))
    env = make_env(D)
    env.reset()
    t_dev, t_dur = torch.from_numpy(dev).cuda(), torch.from_numpy(dur).cuda()
    assert_outputs(env.rollout_autoreset(t_dev[:K1], t_dur[:K1], max_steps=MAX_STEPS), want1, "before the caller's reset")
    env.reset(torch.from_numpy(mask).cuda())
    assert_outputs(env.rollout_autoreset(t_dev[K1:], t_dur[K1:], max_steps=MAX_STEPS), want2, "after the caller's reset")
    assert_episodes(env, {"obs_next": acts_on, "state": state, "tally": tally1 + tally2}, "after the caller's reset")
    assert_state_equal(env, orc, STATE_FIELDS + STAT_FIELDS, where="after the caller's reset")


# ---- 5. replay of the closed loop ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_recorded_closed_loop_replays_through_the_staged_form():
    import torch
    D = 4
    _, cdf = policy_table(D)
    env, twin = make_env(D), make_env(D)
    gpu_prep(env, D)
    gpu_prep(twin, D)
    dev, dur, obs, rew, done, ended = env.rollout_episodes(cdf, K_LONG, SEED, max_steps=MAX_STEPS)
    assert int((ended != 0).sum()) >= MIN_EPISODES
    got = twin.rollout_autoreset(dev, dur, max_steps=MAX_STEPS)
    for name, g, w in zip(NAMES, got, (obs, rew, done, ended)):
        assert torch.equal(g, w), name
    assert torch.equal(twin._last[0], env._last[0]) and torch.equal(twin.episode_state, env.episode_state)
    assert torch.equal(twin.episode_tally, env.episode_tally)
    for f in STATE_FIELDS + STAT_FIELDS:
        assert (twin.get_state(f).view(np.uint8) == env.get_state(f).view(np.uint8)).all(), f


# ---- 6. one case per instantiation ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(INSTANTIATIONS))
def test_instantiation_matches_the_oracle(name, monkeypatch):
    dt, mode = INSTANTIATIONS[name]
    D = dt if dt else 11
    for k, v in dict(MODE_SWITCHES[mode], GW_ROLLOUT_STRICT="1").items():
        monkeypatch.setenv(k, v)
    ref = autoreset_reference(D, K_INST)                                # (shared by the three modes of a sender count)
    env = make_env(D)
    env.reset()
    before = launches(env)
    got = env.rollout_autoreset(*staged(ref), max_steps=MAX_STEPS)
    assert_outputs(got, ref["out"], "under %s" % name)
    assert_episodes(env, ref, "after %s" % name)
    assert_state_equal(env, ref["orc"], STATE_FIELDS + STAT_FIELDS, where="after %s" % name)
    assert delta(launches(env), before) == {name: 1}, launches(env)     # the target, and no step or reset kernel


# ---- 7. invalid actions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_rejected_action_is_a_step_of_the_episode():
    """Step 9 of three envs is outside the action space: the env is untouched, the row repeats what the env acted on with
    reward 0, and -- being the fifth step of the second episode -- it ends that episode by the step limit.  The oracle refuses
    such rows, so the three envs come from a second oracle of three envs that skips the step but not its bookkeeping."""
    import torch
    from gymwipe_amd.actions import EP_COLS, episodes_numpy
    D, K, BAD_STEP = 4, K_INST, 9
    bad = [0, N // 2, N - 1]
    others = np.setdiff1d(np.arange(N), bad)
    dev, dur = staged_actions(D, K)
    big, small = new_oracle(D), new_oracle(D, n=3)
    big.reset()
    state_big = np.zeros((N, 2), np.int32)
    want, acts_big, _ = oracle_autoreset_steps(big, dev, dur, state_big, MAX_STEPS, True)      # (its three columns: ignored)
    small.reset()
    state = np.zeros((3, 2), np.int32)
    rows = [np.empty((K, 3), t) for t in DTYPES]
    tally = np.zeros(EP_COLS, np.int64)
    acts_on, dn_cur, ended_on_bad = np.full(3, CENTER, np.int32), np.zeros(3, np.uint8), None
    for k in range(K):
        if k == BAD_STEP:
            obs, r, dn = acts_on.copy(), np.zeros(3, np.float32), dn_cur.copy()
        else:
            obs, r, dn = small.step(np.ascontiguousarray(dev[k, bad]), np.ascontiguousarray(dur[k, bad]))
        ended, t = episodes_numpy(state, r, dn, MAX_STEPS, True)
        tally += t
        if ended.any():
            small.reset((ended != 0).astype(np.uint8))
        if k == BAD_STEP:
            ended_on_bad = ended.copy()
        for a, v in zip(rows, (obs, r, dn, ended)):
            a[k] = v
        acts_on = np.where(ended != 0, CENTER, obs).astype(np.int32)
        dn_cur = np.where(ended != 0, 0, dn).astype(np.uint8)
    if not (ended_on_bad == 2).any():
        raise RuntimeError("no env reached the step limit on the rejected step")
    g_dev, g_dur = dev.copy(), dur.copy()
    g_dev[BAD_STEP, bad[0]] = D
    g_dur[BAD_STEP, bad[1]] = 99
    g_dev[BAD_STEP, bad[2]] = -1
    env = make_env(D)
    env.reset()
    got = [t.cpu().numpy() for t in env.rollout_autoreset(torch.from_numpy(g_dev).cuda(), torch.from_numpy(g_dur).cuda(),
                                                           max_steps=MAX_STEPS)]
    for name, g, w, w3 in zip(NAMES, got, want, rows):
        assert (g[:, others] == w[:, others]).all(), name
        assert (g[:, bad] == w3).all(), (name, np.argwhere(g[:, bad] != w3)[:3].tolist())
    flags = env.get_state("flags")
    assert np.flatnonzero(flags & FLAG_BADACT).tolist() == bad and env.stats()["bad_actions"] == 3
    assert (env._last[0].cpu().numpy()[others] == acts_big[others]).all() and (env._last[0].cpu().numpy()[bad] == acts_on).all()
    st = env.episode_state.cpu().numpy()
    assert (st[others] == state_big[others]).all() and (st[bad] == state).all()
    for f in STATE_FIELDS + STAT_FIELDS:
        a = env.get_state(f)
        if f == "flags":
            a = a & ~np.asarray(FLAG_BADACT, a.dtype)
        assert (a[others].view(np.uint8) == big.get(f)[others].view(np.uint8)).all(), f
        assert (a[bad].view(np.uint8) == small.get(f).view(np.uint8)).all(), f


# ---- 8. other handles -------------------------------------------------------------------------------------------------------------
K_OTHER = 24


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["explicit_queue", "per_env_geometry", "rollout_cap_0"])
def test_handles_without_a_fused_form_reset_per_step(kind, monkeypatch):
    """(GW_ROLLOUT_CAP is read when the handle is created, so the third handle is a default one without a fused rollout.)"""
    import torch
    from gymwipe_amd import _native as nat
    D = {"explicit_queue": 3, "per_env_geometry": 4, "rollout_cap_0": 4}[kind]
    kw = {"explicit_queue": {"explicit_queue": True}, "per_env_geometry": {"per_env_geometry": True}, "rollout_cap_0": {}}[kind]
    if kind == "rollout_cap_0":
        monkeypatch.setenv("GW_ROLLOUT_CAP", "0")
    env, orc = make_env(D, **kw), new_oracle(D)
    monkeypatch.delenv("GW_ROLLOUT_CAP", raising=False)
    dev, dur = staged_actions(D, 2 * K_OTHER)
    t_dev, t_dur = torch.from_numpy(dev).cuda(), torch.from_numpy(dur).cuda()
    env.reset()
    orc.reset()
    state, tally = np.zeros((N, 2), np.int32), 0
    before = launches(env)
    for call in range(2):
        rows = slice(call * K_OTHER, (call + 1) * K_OTHER)
        got = env.rollout_autoreset(t_dev[rows], t_dur[rows], max_steps=MAX_STEPS)
        want, acts_on, t = oracle_autoreset_steps(orc, dev[rows], dur[rows], state, MAX_STEPS, True)
        tally = tally + t
        assert_outputs(got, want, "in call %d (%s)" % (call, kind))
    if tally[0] < MIN_EPISODES:
        raise RuntimeError("%d episodes ended, fewer than %d" % (tally[0], MIN_EPISODES))
    assert_episodes(env, {"obs_next": acts_on, "state": state, "tally": tally}, "after two calls (%s)" % kind)
    if kind == "per_env_geometry":                                      # (received power as tests/test_rollout_policy.py bounds it)
        fields = tuple(f for f in STATE_FIELDS + STAT_FIELDS if f != "rx_power")
        a, b = env.get_state("rx_power"), orc.get("rx_power")
        assert np.max(np.abs(a - b) / b) < 1e-5
    else:
        fields = STATE_FIELDS + STAT_FIELDS
    assert_state_equal(env, orc, fields, where="after two calls (%s)" % kind)
    ran = delta(launches(env), before)
    assert not [k for k in launches(env) if k.startswith("ct_rollout")], ran
    assert sum(v for k, v in ran.items() if k.startswith("ct_step")) == 2 * K_OTHER and len(ran) == 1, ran
    monkeypatch.setenv("GW_ROLLOUT_STRICT", "1")
    for call in (lambda: env.rollout_autoreset(t_dev[:4], t_dur[:4], max_steps=MAX_STEPS),
                 lambda: env.step_autoreset({"device": t_dev[0], "duration": t_dur[0]}, max_steps=MAX_STEPS)):
        with pytest.raises(nat.NativeError) as exc:
            call()
        assert exc.value.code == nat.EUNSUPPORTED
    assert delta(launches(env), before) == ran                          # refused before anything was launched


# ---- 9. hipGraph ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graph_capture_of_reset_and_eight_autoreset_steps():
    """A linear capture on a side stream (as tests/test_fast_step.py captures step()): one replay equals eager stepping on a
    twin, and with max_steps = 3 the eight steps end two episodes per env."""
    import torch
    D, G = 4, 8
    dev, dur = (torch.from_numpy(a).cuda() for a in staged_actions(D, G))
    acts = [{"device": dev[j].clone(), "duration": dur[j].clone()} for j in range(G)]
    g, e = make_env(D), make_env(D)
    outs_g, outs_e = [step_outputs() for _ in range(G)], [step_outputs() for _ in range(G)]
    for env, outs in ((g, outs_g), (e, outs_e)):                        # eager: fills the identity cache, allocates the tensors
        env.reset()
        for j in range(G):
            env.step_autoreset(acts[j], max_steps=3, out=outs[j])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        g.reset()
        for j in range(G):
            g.step_autoreset(acts[j], max_steps=3, out=outs_g[j])
    for o in outs_g:
        o.ended.fill_(9)
    graph.replay()
    e.reset()
    for j in range(G):
        e.step_autoreset(acts[j], max_steps=3, out=outs_e[j])
    torch.cuda.synchronize()
    for j in range(G):
        for x, y in zip(outs_g[j]._as_tuple + (outs_g[j].ended,), outs_e[j]._as_tuple + (outs_e[j].ended,)):
            assert torch.equal(x, y), j
        assert int(outs_g[j].ended.sum()) == (2 * N if j % 3 == 2 else 0)
    assert torch.equal(g.episode_state, e.episode_state) and torch.equal(g._last[0], e._last[0])
    assert (g.episode_state[:, 0] == G % 3).all()
    for f in STATE_FIELDS + STAT_FIELDS:
        assert (g.get_state(f).view(np.uint8) == e.get_state(f).view(np.uint8)).all(), f
    assert launches(g) == {"ct_rollout_sync_ep<4, 2>": G, "ct_rollout_sync_ep<4, 1>": G}, launches(g)


# ---- 10. shim and ctypes ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_shim_and_ctypes_reach_the_same_entry_point(monkeypatch):
    import torch
    from gymwipe_amd import _native as nat
    if nat.fast() is None:
        pytest.skip("the CPython shim is not built")
    D, K = 4, 20
    dev, dur = (torch.from_numpy(a).cuda() for a in staged_actions(D, K))
    a, b = make_env(D), make_env(D)
    assert a._fast is nat.fast() and hasattr(a._fast, "rollout_autoreset")
    monkeypatch.setattr(b, "_fast", None)                               # this handle's calls go through ctypes
    monkeypatch.setattr(b, "_fast_native", False)
    for env in (a, b):
        env.reset()
    for k in range(K):
        act = {"device": dev[k], "duration": dur[k]}
        ra, rb = a.step_autoreset(act, max_steps=MAX_STEPS), b.step_autoreset(act, max_steps=MAX_STEPS)
        for x, y in zip(ra, rb):
            assert torch.equal(x, y), k
        assert int(ra[3].sum()) == (2 * N if k % MAX_STEPS == MAX_STEPS - 1 else 0)
    assert torch.equal(a.episode_state, b.episode_state) and torch.equal(a.episode_tally, b.episode_tally)
    assert launches(a) == launches(b) == {"ct_rollout_sync_ep<4, 2>": K}


# ---- 11. the agent ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_dqn_fit_with_episode_steps_acts_on_the_resets_observation():
    import torch
    from gymwipe_amd.agents import DqnCounterTrafficAgent
    n, steps, E = 256, 48, 8
    env = make_env(4, n=n)
    agent = DqnCounterTrafficAgent(env, seed=5)
    agent.fit(steps, episode_steps=E)
    assert agent.m_len == steps * n and agent.steps == steps
    m_obs, m_next = agent.m_obs[:steps * n].view(steps, n), agent.m_next[:steps * n].view(steps, n)
    # the default configuration never returns done, so every env's episodes end at steps 7, 15, ... by the step limit
    assert int(agent.m_done.sum()) == 0
    over = torch.zeros(steps - 1, dtype=torch.bool, device=m_obs.device)
    over[E - 1::E] = True
    assert torch.equal(m_obs[0], torch.full_like(m_obs[0], agent.center))
    assert torch.equal(m_obs[1:][over], torch.full_like(m_obs[1:][over], agent.center))   # acted on the reset's observation
    assert torch.equal(m_obs[1:][~over], m_next[:-1][~over])
    assert bool((m_next[:-1][over] != agent.center).any())              # m_next kept the terminal observations
    stats = env.episode_stats()
    assert stats["episodes"] == n * (steps // E) > 0 and stats["by_done"] == 0 and stats["mean_length"] == E
    assert launches(env) == {"ct_rollout_sync_ep<4, 2>": steps}, launches(env)
