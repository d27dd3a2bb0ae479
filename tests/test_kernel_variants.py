"""
One parity case per kernel instantiation of the step / rollout families (134 of them, listed by the library's symbol table).

The host picks an instantiation before every launch -- from the sender count, the queue mode, the exact fast forms gw_create
validated, the host's bound on simulated time, the batch size, per-env stats, live PHY and the A/B switches -- and the
other GPU tests only ever reach some of them.  RECIPES maps every instantiation, spelled as c++filt prints its symbol, to the
configuration that makes the launcher pick it; each case drives GPU and oracle through one shared driver and then asks the
handle's launch record (gw_selftest_launches) whether the target ran and nothing outside the recipe's declared set did.
tests/test_host_logic.py checks on the CPU that RECIPES covers exactly the library's instantiations.
"""
import ctypes as C

import numpy as np
import pytest

from util import (action_stream, assert_state_equal, STATE_FIELDS, STAT_FIELDS, PLANT_MODELS, PLANT_KMAX, PlantEmulation,
                  plant_err, plant_error_bound, plant_reference_ld)

# sender counts with an instantiation of their own, per family (ct_step_sfx.hip, ct_rollout_sfx.hip, ct_step.hip,
# ct_step_dyn.hip); any other D takes DT = 0
SFX_DTS = (2, 3, 4, 5, 6, 7, 8, 16, 32)
EVENT_LOOP_DTS = (2, 3, 4, 6, 8, 16, 32)
LIVE_DTS = (2, 3, 4, 6, 8, 16, 32)
GENERIC_DTS = (2, 3, 4, 8, 16)
GENERIC_LIVE_DTS = (4, 16)

# Layouts whose rx-power residue never closes into a finite noise-state set, at each sender count that has a live-PHY
# instantiation of its own: open_layout(D, seed) draws them (random radii + random extra attenuation per pair; found by a
# search with gw_selftest_fastmath, re-checked on the CPU by tests/test_host_logic.py).  DT = 0 uses tests/test_live_phy.py's
# OPEN_LAYOUTS (D = 9 and 13).
OPEN_LAYOUT_SEEDS = {4: 785, 6: 354, 8: 775, 16: 0, 32: 1}
# Instantiations that no configuration we found reaches.  ct_step_live_kernel<D, false> needs an open noise-state set at
# that D: none turned up at D = 2 or 3 among ~2 000 random geometries each, with or without up to 30 dB of extra
# attenuation per pair (D = 4 needed 785 draws with it, and none turned up without it among 1 500).
UNREACHABLE = {
    "ct_step_live_kernel<2, false>": "no open noise-state layout found at D = 2",
    "ct_step_live_kernel<3, false>": "no open noise-state layout found at D = 3",
}


def open_layout(D, seed, extra_db=30.0):
    """Radios on a random disc layout around an RRM near the origin, every pair with uniform(0, extra_db) dB of extra
    attenuation: (positions, rrm_position, extra_attenuation)."""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0, 2 * np.pi, D)
    rad = rng.uniform(0.5, 6.0, D)
    pos = [(float(r * np.cos(a)), float(r * np.sin(a))) for r, a in zip(rad, ang)]
    rrm = (float(rng.uniform(-1, 1)), float(rng.uniform(-1, 1)))
    extra = {}
    for a in range(D + 1):
        for b in range(a + 1, D + 1):
            extra[(a, b)] = float(rng.uniform(0, extra_db))
    return pos, rrm, extra


def _dt(D, dts):
    return D if D in dts else 0


def _d_for(dt, generic_d):
    return dt if dt else generic_d


# MODE 2: every exact fast form, no per-lane limit tests; 1: the same with the tests (GW_NO_CLASSES: t_limit = 0, every lane
# takes the exact fallback); 0: the plain forms
MODE_SWITCHES = {2: {}, 1: {"GW_NO_CLASSES": "1"}, 0: {"GW_NO_FASTMATH": "1"}}
# the host's bound on simulated time crosses 10^6 s after a few steps (one step takes at most ~21 ms), the clocks themselves
# a few steps later: MODE 2 first, then MODE 1 while lanes straddle the limit
NEAR_LIMIT = 999999.9


def _recipe(kind, D, target, declared, env=None, N=1000, **kw):
    return {"kind": kind, "D": D, "N": N, "env": dict(env or {}), "kw": kw, "target": target,
            "declared": frozenset(set(declared) | {target})}


def _build_recipes():
    R = {}
    # ---- default (suffix-queue) step ----
    for i, dt in enumerate(SFX_DTS + (0,)):
        D = _d_for(dt, 11)
        for mode in (2, 1, 0):
            name = "ct_step_sfx_kernel<%d, %d>" % (dt, mode)
            env, kw, declared = dict(MODE_SWITCHES[mode]), {}, set()
            if mode == 0 and i % 2:
                env = {"GW_NO_IDEM": "1"}       # the D-dependent full transition tables instead of the combined LDS ones
            if mode == 1 and dt in (4, 16, 0):
                env, kw = {}, {"start_time": NEAR_LIMIT}
                declared = {"ct_step_sfx_kernel<%d, 2>" % dt}
            R[name] = _recipe("step", D, name, declared, env, N=37 if (dt, mode) == (5, 2) else 1000, **kw)
            if kw:
                R[name]["first"] = "ct_step_sfx_kernel<%d, 2>" % dt
    # ---- fused rollout, step-synchronous form (GW_ROLLOUT_STRICT: no silent fall-back to step launches), then 3 plain steps
    for dt in SFX_DTS + (0,):
        D = _d_for(dt, 11)
        for mode in (2, 1, 0):
            name = "ct_rollout_sync_kernel<%d, %d>" % (dt, mode)
            R[name] = _recipe("rollout", D, name, {"ct_step_sfx_kernel<%d, %d>" % (dt, mode)},
                              dict(MODE_SWITCHES[mode], GW_ROLLOUT_STRICT="1"))
    # under GW_NO_IDEM the rollouts keep MODE 2 (their fast test leaves idem_states out) while the steps take MODE 0
    R["ct_rollout_sync_kernel<4, 2>"] = _recipe("rollout", 4, "ct_rollout_sync_kernel<4, 2>", {"ct_step_sfx_kernel<4, 0>"},
                                                {"GW_NO_IDEM": "1", "GW_ROLLOUT_STRICT": "1"})
    # ---- fused rollout, event-loop form (GW_ROLLOUT_EVENT_LOOP at gw_create); D = 5 has no instantiation of its own here
    for dt in EVENT_LOOP_DTS + (0,):
        D = _d_for(dt, 5)
        for mode in (2, 1, 0):
            name = "ct_rollout_sfx_kernel<%d, %d>" % (dt, mode)
            R[name] = _recipe("rollout", D, name, {"ct_step_sfx_kernel<%d, %d>" % (_dt(D, SFX_DTS), mode)},
                              dict(MODE_SWITCHES[mode], GW_ROLLOUT_STRICT="1", GW_ROLLOUT_EVENT_LOOP="1"))
    # ---- pendulum env's one-launch step: 32 envs per wave up to 32 768 envs, 64 beyond
    for mode in (2, 1, 0):
        for half, N in ((True, 100), (False, 33000)):
            name = "pend_step_kernel<%d, %s>" % (mode, "true" if half else "false")
            R[name] = _recipe("pendulum", 2, name, set(), MODE_SWITCHES[mode], N=N)
    # ---- generic kernel (explicit queues): walker + helper waves at block 64; one wave with GW_NO_SPLIT, or for DT = 0
    for dt in GENERIC_DTS + (0,):
        D = _d_for(dt, 5)
        for pes in (True, False):
            for split in ((True, False) if dt else (False,)):
                name = "ct_step_kernel<%d, %s, false, %s>" % (dt, str(pes).lower(), str(split).lower())
                R[name] = _recipe("step", D, name, set(), {} if split or not dt else {"GW_NO_SPLIT": "1"},
                                  N=37 if (dt, pes, split) == (2, True, True) else 1000, explicit_queue=True, per_env_stats=pes)
    # ---- generic kernel, live PHY (explicit queues + per-env geometry)
    for dt in GENERIC_LIVE_DTS + (0,):
        D = _d_for(dt, 5)
        for pes in (True, False):
            name = "ct_step_kernel<%d, %s, true, false>" % (dt, str(pes).lower())
            R[name] = _recipe("step", D, name, set(), explicit_queue=True, per_env_stats=pes, per_env_geometry=True)
    # ---- live-PHY default-queue kernel: per-env geometry (rows per env), or a layout without a finite noise-state set
    for dt in LIVE_DTS + (0,):
        D = _d_for(dt, 5)
        name = "ct_step_live_kernel<%d, true>" % dt
        R[name] = _recipe("step", D, name, set(), per_env_geometry=True)
        name = "ct_step_live_kernel<%d, false>" % dt
        if name in UNREACHABLE:
            continue
        if dt:
            pos, rrm, extra = open_layout(D, OPEN_LAYOUT_SEEDS[dt])
        else:
            from test_live_phy import OPEN_LAYOUTS, open_state_set_layout
            D, pos, rrm = open_state_set_layout(OPEN_LAYOUTS[0])
            extra = None
        R[name] = _recipe("step", D, name, set(), N=512, positions=pos, rrm_position=rrm, extra_attenuation=extra)
    return R


RECIPES = _build_recipes()


# ---- the shared driver ----------------------------------------------------------------------------------------------------
def launches(env):
    """The launch record of a handle (env None: of the whole process) as {instantiation: launches}."""
    from gymwipe_amd import _native as nat
    L = nat.lib()
    h = env._h if env is not None else None
    need = L.gw_selftest_launches(h, None, 0)
    assert need >= 0
    buf = C.create_string_buffer(int(need) + 1)
    assert L.gw_selftest_launches(h, buf, len(buf)) == need
    out = {}
    for line in buf.value.decode().splitlines():
        name, n = line.rsplit(" ", 1)
        out[name] = int(n)
    return out


def _mk(recipe):
    from gymwipe_amd import VecCounterTrafficEnv
    from oracle.ct_oracle import CtOracle, default_config
    D, N, kw = recipe["D"], recipe["N"], dict(recipe["kw"])
    kw.setdefault("per_env_stats", True)
    env = VecCounterTrafficEnv(N, num_devices=D, **kw)
    cfg = default_config(D, positions=kw.get("positions"), rrm_pos=kw.get("rrm_position"),
                         extra_att=kw.get("extra_attenuation"), start_time=kw.get("start_time"))
    return env, CtOracle(N, D, config=cfg, nthreads=8)


def _check_state(env, orc, per_env_stats, where, flags=True):
    fields = tuple(f for f in STATE_FIELDS if flags or f != "flags") + (STAT_FIELDS if per_env_stats else ())
    assert_state_equal(env, orc, fields, where=where)


def _outputs_equal(o, r, d, oo, orr, od, where, sel=slice(None)):
    assert (o.cpu().numpy()[sel] == oo[sel]).all(), "obs differ %s" % where
    assert (r.cpu().numpy()[sel] == orr[sel]).all(), "reward differs %s" % where
    assert (d.cpu().numpy()[sel] == od[sel]).all(), "done differs %s" % where


def drive(env, orc, D, N, K, per_env_stats, rollout_k=0, seed=0):
    """Ragged N; full resets and one masked reset; one step with invalid actions in a few envs (those envs must keep their
    state and get FLAG_BADACT; a second call in which only they have valid actions then catches them up with the oracle);
    every step's outputs; the state every 16 steps and at the end; the event totals.  With rollout_k: a fused rollout of that
    many steps, then 3 plain steps.  In the default queue mode every other step goes through gw_step_fb, its byte row checked."""
    import torch
    from gymwipe_amd import _native as nat
    dev, dur = action_stream(seed, K + rollout_k + 3, N, D)
    bad_step, bad_envs = 9, sorted({0, N // 2, N - 1})
    suffix = not env.config.flags & (nat.CFG_EXPLICIT_QUEUE | nat.CFG_PER_ENV_GEOMETRY)
    rows = torch.zeros(N, dtype=torch.uint8, device="cuda")
    n_bad, flags_cleared = 0, False
    assert (env.reset().cpu().numpy() == orc.reset()).all()
    for k in range(K):
        if k in (12, 32):
            assert (env.reset().cpu().numpy() == orc.reset()).all()
        if k == 5:
            mask = (np.arange(N) % 3 == 1).astype(np.uint8)
            assert (env.reset(torch.from_numpy(mask)).cpu().numpy() == orc.reset(mask)).all()
        dk, uk = dev[k].copy(), dur[k].copy()
        fb = suffix and k % 2 == 1
        env.feedback_bytes_into(rows if fb else None)
        if k == bad_step:
            before = {f: orc.get(f)[bad_envs].copy() for f in ("now", "counter", "qlen", "queue", "rx_power")}
            dk[bad_envs[0]], uk[bad_envs[-1]] = D, 99
            if len(bad_envs) > 2:
                dk[bad_envs[1]] = -1
            o, r, d, _ = env.step({"device": torch.from_numpy(dk), "duration": torch.from_numpy(uk)})
            n_bad += len(bad_envs)
            if fb:
                assert torch.equal(rows, env.pack_feedback(o, r, d, check=True)), k
            o1, r1, d1 = o.clone(), r.clone(), d.clone()
            fl = env.get_state("flags")
            assert all(fl[e] & nat.FLAG_BADACT for e in bad_envs)
            assert not (np.delete(fl, bad_envs) & nat.FLAG_BADACT).any()
            for f, v in before.items():                        # untouched: still the oracle's state before this step
                assert (env.get_state(f)[bad_envs].view(np.uint8) == v.view(np.uint8)).all(), f
            dk[bad_envs], uk[bad_envs] = dev[k][bad_envs], dur[k][bad_envs]
            oo, orr, od = orc.step(dk, uk)
            good = np.ones(N, bool)
            good[bad_envs] = False
            _outputs_equal(o1, r1, d1, oo, orr, od, "at the bad-action step", good)
            only = np.where(good, -1, dk).astype(np.int32)     # the catch-up call: every other env is invalid, so untouched
            env.feedback_bytes_into(None)
            o, r, d, _ = env.step({"device": torch.from_numpy(only), "duration": torch.from_numpy(uk)})
            n_bad += N - len(bad_envs)
            _outputs_equal(o, r, d, oo, orr, od, "at the catch-up step", np.array(bad_envs))
            env.clear_flags()                                  # (the oracle never sets FLAG_BADACT)
            flags_cleared = True
        else:
            o, r, d, _ = env.step({"device": torch.from_numpy(dk), "duration": torch.from_numpy(uk)})
            oo, orr, od = orc.step(dk, uk)
            _outputs_equal(o, r, d, oo, orr, od, "at step %d" % k)
            if fb:
                assert torch.equal(rows, env.pack_feedback(o, r, d, check=True)), k
        if (k + 1) % 16 == 0 or k == K - 1:
            _check_state(env, orc, per_env_stats, "after step %d" % k, flags=not flags_cleared)
    env.feedback_bytes_into(None)
    if rollout_k:
        ks = slice(K, K + rollout_k)
        fo, fr, fd = env.rollout(torch.from_numpy(dev[ks]).cuda(), torch.from_numpy(dur[ks]).cuda())
        for j in range(rollout_k):
            oo, orr, od = orc.step(dev[K + j], dur[K + j])
            _outputs_equal(fo[j], fr[j], fd[j], oo, orr, od, "at rollout step %d" % j)
        _check_state(env, orc, per_env_stats, "after the rollout", flags=not flags_cleared)
        for k in range(K + rollout_k, K + rollout_k + 3):
            o, r, d, _ = env.step({"device": torch.from_numpy(dev[k]), "duration": torch.from_numpy(dur[k])})
            oo, orr, od = orc.step(dev[k], dur[k])
            _outputs_equal(o, r, d, oo, orr, od, "at step %d after the rollout" % k)
        _check_state(env, orc, per_env_stats, "after rollout + steps", flags=not flags_cleared)
    if flags_cleared:                                          # flags raised after the clear: a subset of the oracle's
        g, f = env.get_state("flags"), orc.get("flags")
        assert not (g & ~f).any()
    st = env.stats()
    assert st["bad_actions"] == n_bad
    for name, f in (("transmissions", "n_tx"), ("delivered", "n_delivered"), ("appended", "n_appended"),
                    ("popped", "n_popped"), ("dropped", "n_dropped")):
        assert st[name] == int(orc.get(f).sum()), name


def _run_pendulum(recipe, plant=None):
    """pend_step_kernel against the network's oracle (bit-exact) and the plant's oracle advanced to the oracle's clocks
    (<= 1e-5 relative), as tests/test_plant.py does.  ``plant``: (model of tests/util.py, dt) in place of the default plant,
    with a different input per env; the plant state is then also held to the long-double reference within
    util.plant_error_bound after every step, as tests/test_plant_models.py does, and the run must hold three-pass counts."""
    import torch
    from gymwipe_amd import VecInvertedPendulumEnv, VecLinearPlant
    from gymwipe_amd.actions import actions_torch
    from oracle.ct_oracle import CtOracle, default_config
    from oracle.plant_oracle import PlantOracle
    N, K = recipe["N"], 24
    emu = None
    if plant is None:
        env = VecInvertedPendulumEnv(N)
    else:
        m, dt = PLANT_MODELS[plant[0]], plant[1]
        u = np.random.default_rng(13).normal(0.0, 0.3, N)
        env = VecInvertedPendulumEnv(N, plant=VecLinearPlant(N, A=m["A"], B=m["B"], dt=dt, x0=m["x0"], u0=m["u0"]))
        env.plant.setMotorVelocity(torch.from_numpy(u))
        emu = PlantEmulation(m["A"], m["B"], dt, m["x0"], u, N)
    cfg = default_config(2, positions=[(0.0, 0.0), (0.0, -1.0)], rrm_pos=(0.0, 1.0), mult=[1, 0], dest=[1, 0])
    net = CtOracle(N, 2, config=cfg, nthreads=8)
    pc = env.plant.config
    porc = PlantOracle(N, list(pc.A), list(pc.B), pc.dt, list(pc.x0), pc.u0)
    if plant is not None:
        porc.set_input(u)
    a_dev, a_dur = actions_torch(31, 0, N, 0, K, 2, device="cuda")
    h_dev, h_dur = a_dev.cpu().numpy(), a_dur.cpu().numpy()
    nows, xs = [], []
    for k in range(K):
        env.step({"device": a_dev[k], "duration": a_dur[k]})
        net.step(h_dev[k], h_dur[k])
        porc.update(net.get("now"))
        if emu is not None:
            emu.update(net.get("now"))
            nows.append(net.get("now").copy())
            xs.append((env.plant.state(), porc.x.copy(), emu.x.copy()))
            assert (env.plant.get_state("substeps") == porc.substeps).all(), k
            assert (env.plant.get_state("t_last") == porc.t_last).all(), k
        if k % 8 == 7:
            for f in ("now", "wake", "counter", "qlen", "queue", "rx_power"):
                a, b = env.network.get_state(f), net.get(f)
                assert (a.view(np.uint8) == b.view(np.uint8)).all(), (f, k)
            x = env.plant.state()
            assert (env.plant.get_state("substeps") == porc.substeps).all()
            assert (env.plant.get_state("t_last") == porc.t_last).all()
            err = np.abs(x - porc.x) / np.maximum(np.abs(porc.x), 1e-6)
            assert err.max() < 1e-5, err.max()
    if emu is not None:
        ref = plant_reference_ld(m["A"], m["B"], dt, m["x0"], u, np.array(nows))
        assert (ref["substeps"][-1] == porc.substeps).all() and (ref["n"] > 2 * PLANT_KMAX).any()
        e_gpu, e_orc, e_emu = (max(plant_err(v[i], ref["x"][k]) for k, v in enumerate(xs)) for i in range(3))
        print("PLANT_ERR %s %s err_gpu=%.3g err_orc=%.3g err_emu=%.3g" % (recipe["target"], plant[0], e_gpu, e_orc, e_emu))
        assert e_gpu <= plant_error_bound(e_orc, e_emu) and e_gpu < 1e-9, (e_gpu, e_orc, e_emu)
    return env.network


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(RECIPES))
def test_kernel_instantiation_matches_oracle(name, monkeypatch):
    import torch
    recipe = RECIPES[name]
    for k, v in recipe["env"].items():
        monkeypatch.setenv(k, v)
    if recipe["kind"] == "pendulum":
        env = _run_pendulum(recipe)
    else:
        env, orc = _mk(recipe)
        if "first" in recipe:                                  # MODE 2 while the host's bound stays below 10^6 s
            dev, dur = action_stream(5, 1, recipe["N"], recipe["D"])
            env.reset()
            orc.reset()
            o, r, d, _ = env.step({"device": torch.from_numpy(dev[0]), "duration": torch.from_numpy(dur[0])})
            _outputs_equal(o, r, d, *orc.step(dev[0], dur[0]), "at the first step")
            assert launches(env) == {recipe["first"]: 1}, launches(env)
        drive(env, orc, recipe["D"], recipe["N"], 48 if recipe["kind"] == "step" else 20,
              recipe["kw"].get("per_env_stats", True), rollout_k=70 if recipe["kind"] == "rollout" else 0, seed=len(name))
    got = launches(env)
    assert got.get(name, 0) > 0, (name, got)
    assert set(got) <= recipe["declared"], (name, got)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(MODE_SWITCHES))
def test_pendulum_dense_plant_in_every_mode(mode, monkeypatch):
    """The plant half of pend_step_kernel is compiled once per MODE: each of the three with a dense plant at dt = 2.5e-4, where
    an env takes up to ~88 substeps in a step (three passes of the kernel's loop; the default plant never needs a second)."""
    for k, v in MODE_SWITCHES[mode].items():
        monkeypatch.setenv(k, v)
    name = "pend_step_kernel<%d, true>" % mode
    env = _run_pendulum(RECIPES[name], plant=("dense0", 2.5e-4))
    got = launches(env)
    assert got.get(name, 0) > 0 and set(got) <= RECIPES[name]["declared"], (name, got)
