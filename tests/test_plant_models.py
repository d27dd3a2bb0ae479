"""
The two kernels that advance the linear plant on v_mfma_f64_16x16x4_f64 -- plant_update_kernel (plant_mfma.hip) and the plant
half of pend_step_kernel (ct_step_sfx.hip) -- beyond the default model, beyond one tile and beyond one pass.

The plant is builder-defined, so its recurrence x <- A x + B u, taken n = llrint((now - t_last) / dt) times, is the only
specification it has.  tests/util.py restates it in long double (plant_reference_ld), and emulates in float64 numpy what the
kernels compute instead (PlantEmulation: the tables P_k, Q_k of gw_plant_create applied in chunks of at most 32).  The CPU
tier holds oracle/plant_oracle.c and the emulation to the reference and asserts what the substep schedule covers; the GPU
tier holds the kernels to  err <= 16 x max(err_orc, err_emu, 64 ulp)  with both errors taken in the same run, where
err(x) = max over envs of |x_e - ref_e|_inf / max(1, |ref_e|_inf)  (util.plant_error_bound says why 16).

Models: (a) the default pendulum, whose A has e0 as column 0 and whose B and x0 are mostly zero; (b) three dense Gaussian A
of spectral radius 0.999; (c) Q R Q^T of two rotation blocks.  Step sizes: 1e-3, 3e-4 (1/dt inexact) and 2^-10 (exact, so
that a clock difference of k + 1/2 steps is a tie for llrint to break).

Worst err(x_gpu) measured on an MI355X, per model over every N and dt of test_plant_update_kernel_models (the same run's
err_orc / err_emu in brackets); the bound was 2.3e-13 throughout, its 64-ulp floor deciding:
  default 3.72e-15 (1.47e-14 / 3.83e-15)    dense0 2.70e-15 (1.56e-15 / 2.70e-15)    dense1 3.28e-15 (2.24e-15 / 3.39e-15)
  dense2  3.82e-16 (1.07e-15 / 3.96e-16)    qrq    1.85e-15 (1.89e-15 / 1.96e-15)
pend_step_kernel with dense0 at dt = 2.5e-4: 4.18e-15 (1.13e-15 / 4.02e-15) at N = 100, 3.95e-15 (1.78e-15 / 4.01e-15) at N = 33 000; the default
plant five network steps behind: 3.45e-16 (1.57e-15 / 4.56e-16).  profiles/plant_parity/README.md has the tables and what
three deliberately wrong kernels did to these tests.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from util import (PLANT_MODELS, DENSE_MODELS, PLANT_DTS, PLANT_KMAX, PLANT_DESIGNED_ENVS, PlantEmulation, assert_dense,
                  plant_chunks, plant_err, plant_error_bound, plant_reference_ld, plant_schedule)

MODEL_DT = [(m, d) for m in PLANT_MODELS for d in PLANT_DTS]
COVER_N = 63                                  # the smallest tested N that holds the whole designed block of the schedule
assert COVER_N >= PLANT_DESIGNED_ENVS
UPDATE_NS = (1, 15, 16, 17, 63, 65)
BIG_N = 65553                                 # 4097 tiles and a ragged one: the 4096-block grid strides a second time
BIG_CASES = [("default", "1e-3"), ("dense0", "3e-4"), ("dense0", "2^-10")]
INPUT_CHANGES_AT = (3, 8)


@functools.lru_cache(maxsize=None)
def schedule_run(model, dtname, N):
    """One run of the schedule on the CPU, shared by every test that needs it and never modified: the clocks, the per-env
    inputs, the long-double reference, and the float64 oracle's and the emulation's error against it."""
    from oracle.plant_oracle import PlantOracle
    m, dt = PLANT_MODELS[model], PLANT_DTS[dtname]
    now = np.cumsum(plant_schedule(N), axis=0) * dt
    rng = np.random.default_rng(1000 + N)
    u_init = rng.normal(0.0, 0.3, N)              # a different input per env before the first update: distinct states
    changes = {t: (rng.normal(0.0, 0.3, N), rng.random(N) > 0.5) for t in INPUT_CHANGES_AT}
    ref = plant_reference_ld(m["A"], m["B"], dt, m["x0"], u_init, now, changes)
    orc = PlantOracle(N, m["A"], m["B"], dt, m["x0"], m["u0"])
    orc.set_input(u_init)
    emu = PlantEmulation(m["A"], m["B"], dt, m["x0"], u_init, N)
    err_orc = err_emu = 0.0
    for t in range(len(now)):
        orc.update(now[t])
        emu.update(now[t])
        for who in (orc, emu):
            assert (who.substeps == ref["substeps"][t]).all() and (who.t_last == ref["t_last"][t]).all(), (model, dtname, t)
        err_orc = max(err_orc, plant_err(orc.x, ref["x"][t]))
        err_emu = max(err_emu, plant_err(emu.x, ref["x"][t]))
        if t in changes:
            orc.set_input(*changes[t])
            emu.set_input(*changes[t])
    for a in (now, u_init, ref["x"], ref["n"], ref["t_last"], ref["substeps"]):
        a.setflags(write=False)
    return {"model": m, "dt": dt, "now": now, "u_init": u_init, "changes": changes, "ref": ref,
            "err_orc": err_orc, "err_emu": err_emu}


def cpu_error_bound(run):
    """What float64 may lose against the long-double reference, from first principles: one application rounds nine times, so
    it is off by at most 8 ulp-halves of |A|_inf xmax + |B|_inf umax (xmax: the largest component the reference ever held);
    later applications multiply that by at most kappa = max_k |A^k|_inf, and there are S of them.  The tabulated form obeys the
    same bound: entry k of a table carries k such roundings, and a chunk of k substeps stands for k applications."""
    m, ref = run["model"], run["ref"]
    A = np.asarray(m["A"])
    umax = max([np.abs(run["u_init"]).max()] + [np.abs(u).max() for u, _ in run["changes"].values()])
    S = int(ref["substeps"][-1].max())
    kappa, P = 1.0, np.eye(4)
    for _ in range(S):
        P = A @ P
        kappa = max(kappa, float(np.abs(P).sum(axis=1).max()))
    per_step = 8 * 2.0 ** -53 * (np.abs(A).sum(axis=1).max() * ref["xmax"] + np.abs(m["B"]).max() * umax)
    return S * kappa * per_step


# ---- CPU tier -------------------------------------------------------------------------------------------------------------
def test_long_double_is_wider_than_float64():
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is float64 here: the plant tests have no high-precision reference"


def test_models_are_what_they_claim():
    from gymwipe_amd import _native as nat
    cfg = nat.PlantConfig()
    nat.check(nat.lib().gw_plant_config_default(C.byref(cfg), 8))
    d = PLANT_MODELS["default"]
    assert (np.array(list(cfg.A)).reshape(4, 4).view(np.uint64) == d["A"].view(np.uint64)).all()
    assert list(cfg.B) == d["B"].tolist() and list(cfg.x0) == d["x0"].tolist() and cfg.u0 == d["u0"] and cfg.dt == 1e-3
    assert (d["A"][:, 0] == [1, 0, 0, 0]).all()                   # what the default hides: column 0 of every power is e0
    for name in DENSE_MODELS:
        m = PLANT_MODELS[name]
        assert_dense(m["A"])
        assert (m["x0"] != 0).all() and (m["B"] != 0).all()
        rho = np.abs(np.linalg.eigvals(m["A"])).max()
        assert abs(rho - (1.0 if name == "qrq" else 0.999)) < 1e-12, (name, rho)
    assert len({PLANT_MODELS[n]["A"].tobytes() for n in PLANT_MODELS}) == 5
    from fractions import Fraction
    exact = {k: Fraction(1.0 / v) * Fraction(v) == 1 for k, v in PLANT_DTS.items()}      # is float64(1 / dt) the true 1 / dt?
    assert exact == {"1e-3": False, "3e-4": False, "2^-10": True}


@pytest.mark.parametrize("model,dtname", MODEL_DT)
def test_oracle_matches_long_double_reference(model, dtname):
    """oracle/plant_oracle.c: substeps and t_last exactly (asserted inside schedule_run), the state within float64's reach."""
    run = schedule_run(model, dtname, COVER_N)
    bound = cpu_error_bound(run)
    print("%s dt=%s err_orc=%.3g bound=%.3g" % (model, dtname, run["err_orc"], bound))
    assert run["err_orc"] <= bound < 1e-9


@pytest.mark.parametrize("model,dtname", MODEL_DT)
def test_emulation_matches_long_double_reference(model, dtname):
    run = schedule_run(model, dtname, COVER_N)
    bound = cpu_error_bound(run)
    print("%s dt=%s err_emu=%.3g bound=%.3g" % (model, dtname, run["err_emu"], bound))
    assert run["err_emu"] <= bound < 1e-9


@pytest.mark.parametrize("model", list(PLANT_MODELS))
def test_a_wrong_table_is_far_outside_the_bound(model):
    """The check has teeth: an emulation that applies A^(k-1) for A^k, or Q_(k-1) for Q_k, misses the GPU tests' bound by
    orders of magnitude on every model."""
    run = schedule_run(model, "3e-4", COVER_N)
    m, ref = run["model"], run["ref"]
    bound = plant_error_bound(run["err_orc"], run["err_emu"])
    for which in ("P", "Q"):
        emu = PlantEmulation(m["A"], m["B"], run["dt"], m["x0"], run["u_init"], COVER_N)
        if which == "P":
            emu.P[2:] = emu.P[1:-1].copy()
            emu.P[1] = np.eye(4)
        else:
            emu.Q[2:] = emu.Q[1:-1].copy()
            emu.Q[1] = 0.0
        err = 0.0
        for t in range(len(run["now"])):
            emu.update(run["now"][t])
            err = max(err, plant_err(emu.x, ref["x"][t]))
            if t in run["changes"]:
                emu.set_input(*run["changes"][t])
        assert err > 1e-3 > 1e6 * bound, (model, which, err, bound)


@pytest.mark.parametrize("dtname", list(PLANT_DTS))
def test_schedule_covers_what_the_gpu_tests_rely_on(dtname):
    """Conditions on the reference's own substep counts, for the smallest N that holds the designed block (every larger N
    starts with the same 48 envs)."""
    run = schedule_run("dense0", dtname, COVER_N)
    ref, now = run["ref"], run["now"]
    n = ref["n"]
    assert (plant_schedule(BIG_N)[:, :PLANT_DESIGNED_ENVS] == plant_schedule(COVER_N)[:, :PLANT_DESIGNED_ENVS]).all()
    chunks = {c for v in n.ravel() for c in plant_chunks(int(v))}
    assert chunks == set(range(1, PLANT_KMAX + 1))                 # every (candidate group, select) pair
    assert {((c - 1) >> 2, (c - 1) & 3) for c in chunks} == {(g, r) for g in range(8) for r in range(4)}
    for want in (0, 32, 33, 64, 65):
        assert (n == want).any(), want
    assert (n >= 97).any()
    tiles = n[:, :48].reshape(len(n), 3, 16)
    assert (((tiles >= 97).any(axis=2)) & ((tiles == 0).any(axis=2)) & (((tiles >= 1) & (tiles <= 4)).any(axis=2))).any()
    t_before = np.vstack([np.zeros((1, COVER_N)), ref["t_last"][:-1]])
    now_before = np.vstack([np.zeros((1, COVER_N)), now[:-1]])
    assert (now == now_before).any()                               # a clock that did not advance
    assert (now < t_before).any()                                  # a clock below t_last
    assert ((now > t_before) & (n == 0)).any()                     # time passed, but less than half a step
    if dtname == "2^-10":                                          # exact ties: floor even -> down, floor odd -> up
        tie = (now > t_before) & (ref["scaled"] - np.floor(ref["scaled"]) == 0.5)
        fl = np.floor(ref["scaled"]).astype(np.int64)
        assert (tie & (fl % 2 == 0) & (n == fl)).any() and (tie & (fl % 2 == 1) & (n == fl + 1)).any()
        assert (tie & (n == 0)).any() and (tie & (n > 64)).any()


@pytest.mark.parametrize("model", list(PLANT_MODELS))
def test_models_reach_negative_angles(model):
    """int() truncates towards zero, which differs from floor only below zero: the feedback check needs such angles."""
    deg = np.asarray(schedule_run(model, "1e-3", COVER_N)["ref"]["x"][:, :, 2], np.float64) * (180.0 / np.pi)
    assert ((deg < -1.0) & (deg != np.trunc(deg))).any() and (deg > 1.0).any()


# ---- plant_update_kernel --------------------------------------------------------------------------------------------------
WORST = {}                                   # model -> worst (err_gpu, err_orc, err_emu): printed by every case


def _drive_plant(plant, run, update, N):
    """The schedule of ``run`` on ``plant``; ``update(t)`` advances it to run["now"][t] and returns (obs, reward, angle_deg)
    tensors or None.  Integers exact after every update, the state within the bound, the feedback by its formulas."""
    import torch
    ref, now = run["ref"], run["now"]
    plant.setMotorVelocity(torch.tensor(run["u_init"]))
    worst, negative = 0.0, False
    for t in range(len(now)):
        fb = update(t)
        x = plant.state()
        assert (plant.get_state("substeps") == ref["substeps"][t]).all(), t
        assert (plant.get_state("t_last") == ref["t_last"][t]).all(), t
        worst = max(worst, plant_err(x, ref["x"][t]))
        if fb is not None:
            obs, rew, ang = (v.cpu().numpy() for v in fb)
            deg = x[:, 2] * (180.0 / np.pi)                        # math.degrees, in float64 from the returned state
            assert (ang.view(np.uint64) == deg.view(np.uint64)).all(), t
            assert (obs == np.trunc(deg).astype(np.int64)).all(), t
            assert (rew.view(np.uint32) == np.abs(180.0 - deg).astype(np.float32).view(np.uint32)).all(), t
            negative |= bool(((deg < -1.0) & (deg != np.trunc(deg))).any())
        if t in run["changes"]:
            u, mask = run["changes"][t]
            plant.setMotorVelocity(torch.from_numpy(u), torch.from_numpy(mask))
    assert (plant.get_state("u") == np.where(run["changes"][8][1], run["changes"][8][0],
                                             np.where(run["changes"][3][1], run["changes"][3][0], run["u_init"]))).all()
    return worst, negative


def _check_bound(tag, worst, run):
    bound = plant_error_bound(run["err_orc"], run["err_emu"])
    print("PLANT_ERR %s err_gpu=%.3g err_orc=%.3g err_emu=%.3g bound=%.3g" % (tag, worst, run["err_orc"], run["err_emu"], bound))
    assert worst <= bound, "%s: err(x_gpu) = %g above 16 x max(err_orc %g, err_emu %g, 64 ulp)" % (
        tag, worst, run["err_orc"], run["err_emu"])
    assert worst < 1e-9


def _make_plant(run, N):
    import gymwipe_amd
    m = run["model"]
    return gymwipe_amd.VecLinearPlant(N, A=m["A"], B=m["B"], dt=run["dt"], x0=m["x0"], u0=m["u0"])


@pytest.mark.gpu
@pytest.mark.parametrize("model,dtname,N", [(m, d, n) for n in UPDATE_NS for m, d in MODEL_DT] + [(m, d, BIG_N) for m, d in BIG_CASES])
def test_plant_update_kernel_models(model, dtname, N):
    """gw_plant_update_feedback over the schedule, for every model and step size at the tile-edge sizes, and for the default and
    one dense model at 65 553 envs (the grid-stride loop's second iteration)."""
    import torch
    from gymwipe_amd import _native as nat
    run = schedule_run(model, dtname, N)
    plant = _make_plant(run, N)
    cfg = plant.config
    assert list(cfg.A) == run["model"]["A"].reshape(16).tolist() and cfg.dt == run["dt"]      # the arguments arrived
    assert (plant.state() == run["model"]["x0"]).all() and (plant.get_state("u") == run["model"]["u0"]).all()
    obs = torch.full((N,), -77, dtype=torch.int32, device="cuda")
    rew = torch.full((N,), -1.0, dtype=torch.float32, device="cuda")
    ang = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")

    def update(t):
        now = torch.tensor(run["now"][t]).cuda()
        nat.check(plant._L.gw_plant_update_feedback(plant._h, now.data_ptr(), 8, obs.data_ptr(), rew.data_ptr(), ang.data_ptr(),
                                                    torch.cuda.current_stream().cuda_stream))
        return obs, rew, ang

    worst, negative = _drive_plant(plant, run, update, N)
    assert negative or N < COVER_N
    _check_bound("update %s dt=%s N=%d" % (model, dtname, N), worst, run)
    plant.close()


@pytest.mark.gpu
def test_plant_update_strided_now():
    """``now`` as a (data_ptr, stride) pair: the middle column of a [N, 3] float64 tensor whose other columns hold poison."""
    import torch
    N = 65
    run = schedule_run("dense1", "3e-4", N)
    plant = _make_plant(run, N)
    table = torch.empty((N, 3), dtype=torch.float64, device="cuda")

    def update(t):
        table[:, 0], table[:, 2] = float("nan"), 1e300
        table[:, 1] = torch.tensor(run["now"][t]).cuda()
        plant.updateState((table.data_ptr() + 8, 24))
        return None

    worst, _ = _drive_plant(plant, run, update, N)
    _check_bound("strided dense1 dt=3e-4 N=65", worst, run)
    plant.close()


# ---- pend_step_kernel -----------------------------------------------------------------------------------------------------
PEND_DT = 2.5e-4                              # a network step of up to ~22 ms is up to ~88 substeps: three passes
NET_FIELDS = ("now", "wake", "counter", "qlen", "queue", "rx_power")


def _pend_cfg():
    from oracle.ct_oracle import default_config
    return default_config(2, positions=[(0.0, 0.0), (0.0, -1.0)], rrm_pos=(0.0, 1.0), mult=[1, 0], dest=[1, 0])


def _pend_env(N, model, dt, u):
    import torch
    from gymwipe_amd import VecInvertedPendulumEnv, VecLinearPlant
    m = PLANT_MODELS[model]
    env = VecInvertedPendulumEnv(N, plant=VecLinearPlant(N, A=m["A"], B=m["B"], dt=dt, x0=m["x0"], u0=m["u0"]))
    if u is not None:
        env.plant.setMotorVelocity(torch.from_numpy(u))
    return env


def _same_bits(a, b):
    return (np.ascontiguousarray(a).view(np.uint8) == np.ascontiguousarray(b).view(np.uint8)).all()


def _twins_agree(fused, split, fb1, fb2, where):
    import torch
    (o1, r1, d1, i1), (o2, r2, d2, i2) = fb1, fb2
    assert torch.equal(o1, o2) and torch.equal(r1, r2), where
    assert _same_bits(i1["Sensor angle"].cpu().numpy(), i2["Sensor angle"].cpu().numpy()), where
    for f in ("x", "substeps", "t_last"):
        assert _same_bits(fused.plant.get_state(f), split.plant.get_state(f)), (f, where)


def run_pendulum_pair(N, K, model="dense0", dt=PEND_DT, seed=77, lag=0, tag=None):
    """A fused and a two-launch env with the same plant through K steps of one action stream: bit-equal after every step; the
    network against CtOracle; the plant against the references advanced to the oracle's clocks (integers exact, the state
    within plant_error_bound).  ``lag``: network-only steps before each plant step, so that the plant falls behind.
    Returns (fused env, per-step substep counts int64[K][N])."""
    from gymwipe_amd.actions import actions_torch
    from oracle.ct_oracle import CtOracle
    from oracle.plant_oracle import PlantOracle
    m = PLANT_MODELS[model]
    u = np.random.default_rng(seed).normal(0.0, 0.3, N)
    fused, split = _pend_env(N, model, dt, u), _pend_env(N, model, dt, u)
    net = CtOracle(N, 2, config=_pend_cfg(), nthreads=8)
    porc = PlantOracle(N, m["A"], m["B"], dt, m["x0"], m["u0"])
    porc.set_input(u)
    emu = PlantEmulation(m["A"], m["B"], dt, m["x0"], u, N)
    a_dev, a_dur = actions_torch(seed, 0, N, 0, K * (lag + 1), 2, device="cuda")
    h_dev, h_dur = a_dev.cpu().numpy(), a_dur.cpu().numpy()
    nows, xs, j = [], [], 0
    for k in range(K):
        for _ in range(lag):                                       # the network alone: the plant is not told
            act = {"device": a_dev[j], "duration": a_dur[j]}
            fused.network.step(act)
            split.network.step(act)
            net.step(h_dev[j], h_dur[j])
            j += 1
        act = {"device": a_dev[j], "duration": a_dur[j]}
        fb1, fb2 = fused.step(act), split.step(act, fused=False)
        _twins_agree(fused, split, fb1, fb2, k)
        net.step(h_dev[j], h_dur[j])
        j += 1
        now = net.get("now").copy()
        porc.update(now)
        emu.update(now)
        assert (fused.plant.get_state("substeps") == porc.substeps).all(), k
        assert (fused.plant.get_state("t_last") == porc.t_last).all(), k
        x = fused.plant.state()
        deg = x[:, 2] * (180.0 / np.pi)
        assert (fb1[0].cpu().numpy() == np.trunc(deg).astype(np.int64)).all(), k
        assert _same_bits(fb1[1].cpu().numpy(), np.abs(180.0 - deg).astype(np.float32)), k
        assert _same_bits(fb1[3]["Sensor angle"].cpu().numpy(), deg), k
        nows.append(now)
        xs.append((x, porc.x.copy(), emu.x.copy()))
        if k % 8 == 7 or k == K - 1:
            for f in NET_FIELDS:
                assert _same_bits(fused.network.get_state(f), net.get(f)), (f, k)
                assert _same_bits(split.network.get_state(f), net.get(f)), (f, k)
    ref = plant_reference_ld(m["A"], m["B"], dt, m["x0"], u, np.array(nows))
    assert (ref["substeps"][-1] == porc.substeps).all() and (ref["t_last"][-1] == porc.t_last).all()
    err = [max(plant_err(v[i], ref["x"][k]) for k, v in enumerate(xs)) for i in range(3)]
    _check_bound(tag or "pend %s dt=%g N=%d lag=%d" % (model, dt, N, lag), err[0], {"err_orc": err[1], "err_emu": err[2]})
    assert int(fused.network.get_state("flags").max()) & 3 == 0
    split.close()
    return fused, ref["n"]


def assert_multi_pass_coverage(n, N):
    """From the oracle's clocks: three-pass and two-pass counts occur, and some wave holds envs with different pass counts."""
    assert (n > 2 * PLANT_KMAX).any() and ((n > PLANT_KMAX) & (n <= 2 * PLANT_KMAX)).any() and (n <= PLANT_KMAX).any()
    epw = 32 if N <= 32 * 1024 else 64                             # envs per wave (gw_launch_pend_step)
    passes = (n + PLANT_KMAX - 1) // PLANT_KMAX
    full = N // epw * epw
    per_wave = passes[:, :full].reshape(len(n), -1, epw)
    assert (per_wave.max(axis=2) > per_wave.min(axis=2)).any()
    rounds = per_wave.reshape(len(n), -1, epw // 16, 16).max(axis=3)   # and so do the 16-env rounds of one wave
    assert (rounds.max(axis=2) > rounds.min(axis=2)).any()
    chunks = {c for v in np.unique(n) for c in plant_chunks(int(v))}
    assert {(c - 1) >> 2 for c in chunks} == set(range(PLANT_KMAX // 4))   # every candidate group, 6 and 7 (k = 25..32) among them


@pytest.mark.gpu
@pytest.mark.parametrize("N,K", [(100, 24), (33000, 12)])
def test_pend_step_dense_plant_several_passes(N, K):
    """A dense plant at dt = 2.5e-4 under both wave mappings (32 envs per wave at N = 100, 64 at 33 000, both with a ragged
    last wave): the pass loop of pend_step_kernel runs up to three times, with different counts inside one wave."""
    fused, n = run_pendulum_pair(N, K)
    assert_multi_pass_coverage(n, N)
    fused.close()


@pytest.mark.gpu
def test_pend_step_lagging_default_plant():
    """The default plant at dt = 1e-3 left behind for five network steps: about 100 substeps in one launch."""
    fused, n = run_pendulum_pair(100, 2, model="default", dt=1e-3, lag=5)
    assert n.max() > 3 * PLANT_KMAX and (n > 2 * PLANT_KMAX).mean() > 0.2, n.max()
    fused.close()


@pytest.mark.gpu
def test_pend_step_bad_action_leaves_env_and_plant_alone():
    """device = 2 in a few envs: their network and plant state stay, FLAG_BADACT is raised, obs and reward are still written
    from the current plant, and the fused and the two-launch step agree; every other env goes on as the oracle says."""
    import torch
    from gymwipe_amd import _native as nat
    from gymwipe_amd.actions import actions_torch
    from oracle.ct_oracle import CtOracle
    N, K, bad = 100, 6, [0, 31, 32, 50, 99]
    good = np.ones(N, bool)
    good[bad] = False
    u = np.random.default_rng(3).normal(0.0, 0.3, N)
    fused, split = _pend_env(N, "dense0", PEND_DT, u), _pend_env(N, "dense0", PEND_DT, u)
    net = CtOracle(N, 2, config=_pend_cfg(), nthreads=8)
    a_dev, a_dur = actions_torch(11, 0, N, 0, K, 2, device="cuda")
    for k in range(K):
        dev = a_dev[k].clone()
        if k == 3:
            dev[bad] = 2
            before = {f: fused.network.get_state(f)[bad].copy() for f in NET_FIELDS}
            before.update({f: fused.plant.get_state(f)[bad].copy() for f in ("x", "substeps", "t_last")})
            sentinel = [(fused._obs, -77), (fused._rew, -1.0), (split._obs, -77), (split._rew, -1.0)]
            for buf, v in sentinel:
                buf.fill_(v)
        act = {"device": dev, "duration": a_dur[k]}
        fb1, fb2 = fused.step(act), split.step(act, fused=False)
        _twins_agree(fused, split, fb1, fb2, k)
        if k == 3:
            for env in (fused, split):
                fl = env.network.get_state("flags")
                assert (fl[bad] & nat.FLAG_BADACT).all() and not (fl[good] & nat.FLAG_BADACT).any()
                for f in NET_FIELDS:
                    assert _same_bits(env.network.get_state(f)[bad], before[f]), f
                for f in ("x", "substeps", "t_last"):
                    assert _same_bits(env.plant.get_state(f)[bad], before[f]), f
            deg = before["x"][:, 2] * (180.0 / np.pi)
            assert (fb1[0].cpu().numpy()[bad] == np.trunc(deg).astype(np.int64)).all()
            assert _same_bits(fb1[1].cpu().numpy()[bad], np.abs(180.0 - deg).astype(np.float32))
            assert _same_bits(fb1[3]["Sensor angle"].cpu().numpy()[bad], deg)
            assert (fused.plant.get_state("substeps")[good] > 0).all()
        if k <= 3:                                                 # the oracle takes no invalid action: the good envs only
            net.step(a_dev[k].cpu().numpy(), a_dur[k].cpu().numpy())
            for f in NET_FIELDS:
                assert _same_bits(fused.network.get_state(f)[good], net.get(f)[good]), (f, k)
    for f in NET_FIELDS:                                           # the flagged envs went on afterwards, in step with each other
        assert _same_bits(fused.network.get_state(f), split.network.get_state(f)), f
    assert (fused.network.get_state("now")[bad] > before["now"]).all()
    assert fused.network.stats()["bad_actions"] == len(bad)
    fused.close()
    split.close()
