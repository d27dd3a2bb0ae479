"""The closed control loop (second half) -- builder-defined, so its oracle is the event-driven
ControlLoopModel of the same rules (oracle/des_model.py); the HIP kernel must match it bit for bit: integers, the f64
clock, the plant state, the controller's angle, the motor velocity, queue lengths, deliveries, received powers."""
import functools

import numpy as np
import pytest

from ctrl_fixtures import DENSE_CTRL, STREAMS, stream_of          # the streams' layout and the dense plant: shared with the references
from oracle import des_model as dm
from util import assert_dense


def test_control_loop_model_closes_the_loop():
    """CPU tier: in the model, sensor packets reach the controller, commands reach the actuator and change the plant's
    input; an open loop (nobody assigned) leaves it untouched."""
    m = dm.ControlLoopModel()
    for k in range(30):
        m.step(k % 2, 12)
    s = m.snapshot()
    assert s["received"][1] > 0 and s["received"][2] > 0 and s["commands"] >= s["received"][2]
    assert s["u"] != 0.1 and s["angle_deg"] != 0.0
    assert s["substeps"] == m.tick                       # one plant substep per sensor tick
    idle = dm.ControlLoopModel()
    for k in range(10):
        idle.step(0, 0)                                   # zero-length windows: nothing is ever transmitted but announcements
    assert idle.snapshot()["received"] == [0, 0, 0] and idle.snapshot()["u"] == 0.1


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,start,period", [(1, 20, 10), (2, 0, 3), (3, 50, 1)])
def test_control_loop_kernel_matches_event_driven_model(seed, start, period):
    import torch
    from gymwipe_amd import VecControlLoopEnv
    N, K = 6, 70
    rng = np.random.default_rng(seed)
    env = VecControlLoopEnv(N, ctrl_start_tick=start, ctrl_period_ticks=period)
    models = [dm.ControlLoopModel(start=start, period=period) for _ in range(N)]
    for k in range(K):
        dev = rng.integers(0, 2, N).astype(np.int32)
        dur = rng.integers(0, 20, N).astype(np.int32)
        obs, rew, done, info = env.step({"device": torch.from_numpy(dev), "duration": torch.from_numpy(dur)})
        obs, rew, ang = obs.cpu().numpy(), rew.cpu().numpy(), info["Sensor angle"].cpu().numpy()
        st = {f: env.get_state(f) for f in ("now", "x", "u", "angle_deg", "qlen", "received", "n_tx", "commands", "substeps",
                                            "rx_power", "flags")}
        for e, m in enumerate(models):
            o, r, d, i = m.step(int(dev[e]), int(dur[e]))
            s = m.snapshot()
            where = (seed, k, e)
            assert obs[e] == o and rew[e] == np.float32(r) and _bits(ang[e]) == _bits(i["Sensor angle"]), where
            assert _bits(st["now"][e]) == _bits(s["now"]), where
            assert (_bits(st["x"][e]) == _bits(s["x"])).all(), where
            assert _bits(st["u"][e]) == _bits(s["u"]) and _bits(st["angle_deg"][e]) == _bits(s["angle_deg"]), where
            assert st["qlen"][e].tolist() == s["qlen"][:2] and s["qlen"][2] == 0, where
            assert st["received"][e].tolist() == s["received"][1:], where
            assert int(st["n_tx"][e]) == s["n_tx"] and int(st["commands"][e]) == s["commands"], where
            assert int(st["substeps"][e]) == s["substeps"], where
            assert (_bits(st["rx_power"][e]) == _bits(s["rx_power"])).all(), where
            assert int(st["flags"][e]) & 3 == 0, where
    assert env.get_state("received").sum() > 0


@pytest.mark.gpu
def test_control_loop_env_surface():
    import torch
    import gymwipe_amd
    env = gymwipe_amd.make("VecControlLoop-v0", num_envs=1024)
    assert env.action_space.contains({"device": 1, "duration": 19}) and env.observation_space.n == 180
    z = torch.zeros(1024, dtype=torch.int32, device="cuda")
    assert (env.reset() == 2).all()                                    # int(degrees(0.05 rad)), nothing is reset
    obs, rew, done, info = env.step({"device": z, "duration": z + 7})
    assert env.reset() is obs
    assert obs.shape == (1024,) and rew.dtype == torch.float32 and not done.any()
    env.step({"device": z + 2, "duration": z})                         # the actuator is not assignable: flagged, env untouched
    assert (env.get_state("flags") & 8).all()
    env.close()


# ---- more than one block, and another plant ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model_streams(plant, K, seed, start, period):
    """STREAMS action streams of K steps through one ControlLoopModel each: the actions, and per step and stream the model's
    feedback and snapshot as arrays.  Computed once per plant, shared and never modified."""
    rng = np.random.default_rng(seed)
    dev = rng.integers(0, 2, (K, STREAMS)).astype(np.int32)
    dur = rng.integers(0, 20, (K, STREAMS)).astype(np.int32)
    kw = {} if plant is None else {"A": DENSE_CTRL["A"].tolist(), "B": DENSE_CTRL["B"].tolist(), "x0": tuple(DENSE_CTRL["x0"]),
                                   "u0": DENSE_CTRL["u0"]}
    models = [dm.ControlLoopModel(start=start, period=period, **kw) for _ in range(STREAMS)]
    steps = []
    for k in range(K):
        fb = [m.step(int(dev[k, s]), int(dur[k, s])) for s, m in enumerate(models)]
        sn = [m.snapshot() for m in models]
        want = {"obs": np.array([f[0] for f in fb], np.int64), "rew": np.array([np.float32(f[1]) for f in fb], np.float32),
                "ang": np.array([f[3]["Sensor angle"] for f in fb], np.float64)}
        for f in ("now", "x", "u", "angle_deg", "rx_power"):
            want[f] = np.array([q[f] for q in sn], np.float64)
        want["qlen"] = np.array([q["qlen"][:2] for q in sn], np.int64)
        assert all(q["qlen"][2] == 0 for q in sn)
        want["received"] = np.array([q["received"][1:] for q in sn], np.int64)
        for f in ("n_tx", "commands", "substeps"):
            want[f] = np.array([q[f] for q in sn], np.int64)
        for v in want.values():
            v.setflags(write=False)
        steps.append(want)
    return dev, dur, steps


def test_dense_control_loop_model_stays_bounded_and_closes():
    """CPU tier: the dense plant of the multi-block GPU test, checked on the model before use -- dense, bounded under the
    controller's commands, its loop closed, and far from the default plant's trajectory."""
    assert_dense(DENSE_CTRL["A"])
    _, _, steps = model_streams("dense", 40, 21, 5, 3)
    x = np.array([w["x"] for w in steps])
    assert np.isfinite(x).all() and np.abs(x).max() < 50.0, np.abs(x).max()
    assert np.abs(np.array([w["ang"] for w in steps])).max() < 2000.0           # int32 obs, far from overflow
    last = steps[-1]
    assert (last["commands"] > 0).all() and (last["received"] > 0).all() and (last["u"] != DENSE_CTRL["u0"]).any()
    assert len({w["x"].tobytes() for w in steps}) == len(steps)                 # the state moves in every step
    assert len({last["x"][s].tobytes() for s in range(STREAMS)}) == STREAMS     # and the streams differ from each other


def _run_streams(N, K, seed, plant, start=5, period=3):
    import torch
    from gymwipe_amd import VecControlLoopEnv
    dev, dur, steps = model_streams(plant, K, seed, start, period)
    so = stream_of(N)
    kw = {} if plant is None else {"A": DENSE_CTRL["A"], "B": DENSE_CTRL["B"], "x0": DENSE_CTRL["x0"], "u0": DENSE_CTRL["u0"]}
    env = VecControlLoopEnv(N, ctrl_start_tick=start, ctrl_period_ticks=period, **kw)
    for k in range(K):
        obs, rew, done, info = env.step({"device": torch.from_numpy(dev[k][so]), "duration": torch.from_numpy(dur[k][so])})
        want = steps[k]
        got = {"obs": obs.cpu().numpy(), "rew": rew.cpu().numpy(), "ang": info["Sensor angle"].cpu().numpy()}
        for f in ("now", "x", "u", "angle_deg", "rx_power", "qlen", "received", "n_tx", "commands", "substeps"):
            got[f] = env.get_state(f)
        for f, w in want.items():
            w, g = w[so], got[f]
            same = (g.view(np.uint64) == w.view(np.uint64)) if w.dtype == np.float64 else (
                (g.view(np.uint32) == w.view(np.uint32)) if w.dtype == np.float32 else (g == w))
            assert same.all(), (f, k, np.argwhere(~same)[:4].tolist())
        assert not (env.get_state("flags") & 3).any(), k
        assert not done.any()
    assert (env.get_state("received") > 0).all() and (env.get_state("commands") > 0).all()
    env.close()


@pytest.mark.gpu
def test_control_loop_kernel_across_blocks():
    """N = 200: three full 64-env blocks and a ragged wave of 8, every env compared bit for bit with the model of its stream
    (the N-strided arrays and the per-lane LDS columns at blockIdx.x > 0)."""
    _run_streams(200, 40, 20, None)


@pytest.mark.gpu
def test_control_loop_kernel_dense_plant():
    """N = 70 with a dense A, a dense B and another u0: VecControlLoopEnv(A=, B=, u0=) reach the kernel."""
    _run_streams(70, 40, 21, "dense")
