"""
The 16 fused rollout families, and the per-step forms of three of them, where packets are lost and grants are refused
(util.lossy_layout(): one sender only some of whose packets reach the RRM, two that never decode an announcement), and the fast
forms' limit on simulated time crossed inside one launch.

Every expected value comes from the oracle alone, through the sibling files' compositions: tests/test_rollout_lossy_cpu.py
builds each reference once and refuses to hand out one that does not exercise what it is for (partly delivered steps, refused
grants, episodes, and a popped-for-delivered substitute that would change a compared output).  All comparisons are bit for bit:
every output row, obs_next, {age, ret}, the tallies and tables, the controllers' nodes, the state (STATE_FIELDS + STAT_FIELDS).
Every fused case asserts from the launch record that exactly its target instantiation ran (two launches: 64 + 6 steps) with no
step, reset or bookkeeping kernel beside it, under GW_ROLLOUT_STRICT.  N = 192 is three blocks, P x M = 3 x 64.
"""
import numpy as np
import pytest

from test_kernel_variants import MODE_SWITCHES, SFX_DTS, launches
from test_rollout_backlog import gpu_prologue, make_env as make_backlog_env
from test_rollout_lossy_cpu import (FAMILIES, FLAGS_FATAL, LIMIT_STEPS, M, MAX_STEPS, MODERATE, N, NEAR_LIMIT, SEED, STEPS, env_kw,
                                    limit_reference, prep_cols, reference)
from test_rollout_policy import delta, gpu_prep, make_env
from util import assert_state_equal, STATE_FIELDS, STAT_FIELDS

KIND_OF = {family: kind for kind, families in FAMILIES.items() for family in families}
BACKLOG_ROWS = ("obs", "reward", "done", "ended", "delivered", "device", "duration", "seen_len")
POLICY_ROWS = ("device", "duration", "obs", "reward", "done", "ended", "delivered", "node")
STAGED_ROWS = ("obs", "reward", "done", "ended", "delivered")

CASES = ([(family, 4, 2) for family in sorted(KIND_OF)]
         + [(family, 9, 2) for family in ("ct_rollout_sync_kernel", "ct_rollout_policy_eps", "ct_rollout_backlog", "ct_rollout_fsc")]
         + [(family, 4, mode) for mode in (1, 0) for family in ("ct_rollout_sync_kernel", "ct_rollout_policy_eps")])


def fused_name(family, D, mode=2):
    return "%s<%d, %d>" % (family, D if D in SFX_DTS else 0, mode)


def prepared_env(kind, D, layout="lossy", **kw):
    """A handle in the state the reference of run kind ``kind`` starts from."""
    if kind in ("backlog", "backlog_pop"):
        env = make_backlog_env(D, MODERATE, n=N, **dict(env_kw(layout, D), **kw))
        gpu_prologue(env)
    else:
        env = make_env(D, n=N, **dict(env_kw(layout, D), **kw))
        if kind in ("sync", "auto", "auto_scored"):
            env.reset()
        else:
            gpu_prep(env, D, prep_cols(0, N))
    return env


def assert_rows(got, cmp, names, where):
    assert len(got) == len(names)
    for name, g in zip(names, got):
        g, w = g.cpu().numpy(), cmp[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (name, where, g.dtype, w.dtype)
        assert (g.view(np.uint8) == w.view(np.uint8)).all(), \
            "%s differs %s, first at (step, env) %s" % (name, where, np.argwhere(g != w)[:3].tolist())


def assert_table(got, want, where):
    g = got.cpu().numpy()
    assert g.dtype == want.dtype and g.shape == want.shape, where
    assert (g == want).all(), "the table differs %s, first at (class, action, column) %s" % (where, np.argwhere(g != want)[:3].tolist())


def assert_episodes(env, cmp, where, call_wide=None):
    assert (env._last[0].cpu().numpy() == cmp["obs_next"]).all(), "obs_next differs " + where
    assert (env.episode_state.cpu().numpy() == cmp["state"]).all(), "{age, ret} differs " + where
    call_wide = cmp["tally"] if call_wide is None else call_wide
    assert env.episode_tally.cpu().numpy().tolist() == np.asarray(call_wide).tolist(), "the call-wide tally differs " + where


def assert_states(env, ref, where):
    """The handle's state against the oracle's -- against each slice's own oracle where the reference has several."""
    orcs = ref["orcs"]
    if len(orcs) == 1:
        assert_state_equal(env, orcs[0], STATE_FIELDS + STAT_FIELDS, where=where)
        return
    for f in STATE_FIELDS + STAT_FIELDS:
        got = env.get_state(f)
        for p, orc in enumerate(orcs):
            assert (got[p * M:(p + 1) * M].view(np.uint8) == orc.get(f).view(np.uint8)).all(), (f, p, where)


def staged(ref):
    import torch
    return torch.tensor(ref["dev"]).cuda(), torch.tensor(ref["dur"]).cuda()      # (copies: the reference is read-only)


def call_family(family, env, ref, steps, where):
    """The call that runs ``family`` on a fused handle, its results compared with the reference's."""
    import torch
    from gymwipe_amd.actions import make_controller_population
    cmp = ref["cmp"]
    ep = dict(max_steps=MAX_STEPS)
    if family == "ct_rollout_sync_kernel":
        assert_rows(env.rollout(*staged(ref)), cmp, ("obs", "reward", "done"), where)
    elif family == "ct_rollout_policy":
        assert_rows(env.rollout_policy(ref["cdf"], steps, SEED), cmp, POLICY_ROWS[:5], where)
    elif family in ("ct_rollout_pstats", "ct_rollout_pstats_d"):
        ret = torch.zeros(N, dtype=torch.int32, device=env.device)
        packets = family.endswith("_d")
        got = env.rollout_policy_stats(ref["cdf"], steps, SEED, returns=ret, packets=packets)
        assert_table(got, cmp["table8" if packets else "table7"], where)
        assert (ret.cpu().numpy() == cmp["returns"]).all(), "returns differ " + where
        assert (env._last[0].cpu().numpy() == cmp["obs_next"]).all(), "obs_next differs " + where
    elif family == "ct_rollout_policy_ep":
        assert_rows(env.rollout_episodes(ref["cdf"], steps, SEED, **ep), cmp, POLICY_ROWS[:6], where)
        assert_episodes(env, cmp, where)
    elif family in ("ct_rollout_pstats_ep", "ct_rollout_pstats_epd"):
        packets = family.endswith("_epd")
        got = env.rollout_episodes_stats(ref["cdf"], steps, SEED, packets=packets, **ep)
        assert_table(got, cmp["table8" if packets else "table7"], where)
        assert_episodes(env, cmp, where)
    elif family == "ct_rollout_policy_eps":
        assert_rows(env.rollout_episodes(ref["cdf"], steps, SEED, score=ref["score"], **ep), cmp, POLICY_ROWS[:7], where)
        assert_episodes(env, cmp, where)
    elif family in ("ct_rollout_pop_ep", "ct_rollout_pop_eps"):
        got = env.rollout_population(ref["cdfs"], steps, SEED, score=ref.get("score"), **ep)
        assert got.cpu().numpy().tolist() == cmp["tally"].tolist(), "the per-policy tally differs " + where
        assert_episodes(env, cmp, where, call_wide=cmp["tally"].sum(axis=0))
    elif family == "ct_rollout_sync_ep":
        assert_rows(env.rollout_autoreset(*staged(ref), **ep), cmp, STAGED_ROWS[:4], where)
        assert_episodes(env, cmp, where)
    elif family == "ct_rollout_sync_eps":
        assert_rows(env.rollout_autoreset(*staged(ref), score=ref["score"], **ep), cmp, STAGED_ROWS, where)
        assert_episodes(env, cmp, where)
    elif family == "ct_rollout_backlog":
        assert_rows(env.rollout_backlog(steps, ref["policy"], score=ref["score"], **ep), cmp, BACKLOG_ROWS, where)
        assert_episodes(env, cmp, where)
    elif family == "ct_rollout_backlog_pop":
        got = env.rollout_backlog_population(ref["population"], steps, score=ref["score"], **ep)
        assert got.cpu().numpy().tolist() == cmp["tally"].tolist(), "the per-policy tally differs " + where
        assert_episodes(env, cmp, where, call_wide=cmp["total"])
    elif family == "ct_rollout_fsc":
        assert_rows(env.rollout_controller(ref["controller"], steps, SEED, score=ref["score"], **ep), cmp, POLICY_ROWS, where)
        assert_episodes(env, cmp, where)
        assert (env.controller_node.cpu().numpy() == cmp["node_dev"]).all(), "node_dev differs " + where
    elif family == "ct_rollout_fsc_pop":
        got = env.rollout_controller_population(make_controller_population(ref["controllers"]), steps, SEED, score=ref["score"], **ep)
        assert got.cpu().numpy().tolist() == cmp["tally"].tolist(), "the per-controller tally differs " + where
        assert_episodes(env, cmp, where, call_wide=cmp["tally"].sum(axis=0))
        assert (env.controller_node.cpu().numpy() == cmp["node_dev"]).all(), "node_dev differs " + where
    else:
        raise KeyError(family)


# ---- 1. the fused families ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("family,D,mode", CASES, ids=["%s-D%d-MODE%d" % c for c in CASES])
def test_fused_family_matches_the_oracle_on_the_lossy_layout(family, D, mode, monkeypatch):
    kind = KIND_OF[family]
    ref = reference(kind, D)
    for k, v in dict(MODE_SWITCHES[mode], GW_ROLLOUT_STRICT="1").items():
        monkeypatch.setenv(k, v)
    name = fused_name(family, D, mode)
    env = prepared_env(kind, D)
    before = launches(env)
    call_family(family, env, ref, STEPS, "under %s" % name)
    assert_states(env, ref, "after %s" % name)
    assert delta(launches(env), before) == {name: 2}, launches(env)     # 64 + 6 steps of the target and nothing else
    assert not ref["flags"] & FLAGS_FATAL
    env.check()


# ---- 2. the per-step forms ------------------------------------------------------------------------------------------------------------
# GW_ROLLOUT_POLICY_UNFUSED governs the calls that draw or choose their actions; gw_rollout_autoreset has no such switch, so its
# per-step form is reached on the capacity-0 handle only.
PER_STEP = [("episodes", "unfused_switch"), ("episodes", "rollout_cap_0"), ("autoreset", "rollout_cap_0"),
            ("backlog", "unfused_switch"), ("backlog", "rollout_cap_0")]


@pytest.mark.gpu
@pytest.mark.parametrize("call,route", PER_STEP, ids=["%s-%s" % c for c in PER_STEP])
def test_per_step_form_matches_the_oracle_on_the_lossy_layout(call, route, monkeypatch):
    """policy_sample_kernel, episodes_step_kernel<true>, gw_delivered and the per-step backlog difference the delivered half of
    the counter word: the same references, no fused launch, and gw_delivered's row against the oracle's counter."""
    import torch
    from gymwipe_amd import _native as nat
    D = 4
    family = {"episodes": "ct_rollout_policy_eps", "autoreset": "ct_rollout_sync_eps", "backlog": "ct_rollout_backlog"}[call]
    kind = KIND_OF[family]
    ref = reference(kind, D)
    if route == "rollout_cap_0":
        monkeypatch.setenv("GW_ROLLOUT_CAP", "0")                       # (read when the handle is created)
    env = prepared_env(kind, D)
    monkeypatch.delenv("GW_ROLLOUT_CAP", raising=False)
    if route == "unfused_switch":
        monkeypatch.setenv("GW_ROLLOUT_POLICY_UNFUSED", "1")
    before = launches(env)
    call_family(family, env, ref, STEPS, "per step (%s, %s)" % (call, route))
    assert_states(env, ref, "per step (%s, %s)" % (call, route))
    ran = delta(launches(env), before)
    assert not [k for k in launches(env) if k.startswith("ct_rollout")], ran
    assert sum(v for k, v in ran.items() if k.startswith("ct_step")) == STEPS and len(ran) == 1, ran
    row = torch.empty(N, dtype=torch.int32, device=env.device)          # as VecCounterTrafficEnv._feed_custom calls it
    with torch.cuda.device(env.device):
        nat.check(env._L.gw_delivered(env._h, row.data_ptr(), env._stream()))
    want = ref["orcs"][0].get("n_delivered").astype(np.int64)
    assert (row.cpu().numpy().astype(np.int64) == want).all(), "gw_delivered differs from the oracle's n_delivered"
    assert (want != ref["orcs"][0].get("n_popped").astype(np.int64)).any()
    env.check()


# ---- 3. the limit crossed inside a launch -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("family", ["ct_rollout_sync_kernel", "ct_rollout_policy_eps"])
def test_clocks_cross_the_fast_forms_limit_inside_one_launch(family, monkeypatch):
    """Started at NEAR_LIMIT with every clock below 10^6 s: the host's bound on the clocks selects MODE 1 by itself, and lanes
    straddle the limit while the launch runs (limit_reference() gates both on the oracle's clocks)."""
    kind = KIND_OF[family]
    ref = limit_reference(kind)
    monkeypatch.setenv("GW_ROLLOUT_STRICT", "1")
    env = prepared_env(kind, 4, layout="default", start_time=NEAR_LIMIT)
    assert (env.get_state("now") == ref["now0"]).all() and (ref["now0"] < 1.0e6).all()
    before = launches(env)
    call_family(family, env, ref, LIMIT_STEPS, "across the limit")
    assert_states(env, ref, "across the limit")
    assert delta(launches(env), before) == {fused_name(family, 4, 1): 1}, launches(env)
    assert not ref["flags"] & FLAGS_FATAL
    env.check()
