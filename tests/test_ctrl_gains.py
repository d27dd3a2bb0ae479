"""Per-env PID gains of the control loop on the GPU (gw_ctrl_set_gains): the PID instantiations of the step kernel and of the
fused rollout kernels against the event-driven model of tests/ctrl_pid_model.py, bit for bit, over every state field and the
controller's own two (``gains``, ``last_error``).  A reset env is a freshly constructed model with the same gains.  The
fixtures are defined in tests/ctrl_pid_model.py and qualified on the model alone in tests/test_ctrl_gains_cpu.py (every gain
matters, a kept last error would show, both ending causes occur).  What this file does as the disturbance's and the loss's do
is in tests/ctrl_gpu_harness.py; what belongs to the gains alone is asserted here.  Every test calls ``set_gains``: none passes
without it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctrl_gpu_harness as h
import ctrl_pid_model as pm
from ctrl_fixtures import T, assert_same
from ctrl_tiers import PID

PID_FIELDS = h.state_fields(PID)
MODEL_FIELDS = h.model_fields(PID)
GAINS = h.GAINS


# ---- 1. step -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("plant", [None, "dense"])
@pytest.mark.parametrize("seed,start,period", [(1, 20, 10), (2, 0, 3), (3, 50, 1)])
def test_step_with_per_env_gains_matches_the_model(seed, start, period, plant):
    r = h.step_matches_the_model(PID, 70, seed, start, period, plant)
    assert_same(r.first["gains"], GAINS[r.gi], "gains at construction")
    assert not (r.final["flags"] & 3).any()
    assert (r.final["commands"] > 0).all() and (r.final["last_error"] != 0).all()


# ---- 2. gains (1, 0, 0) are the unswitched handle --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_default_gains_set_explicitly_equal_a_handle_that_never_set_any():
    one, two = h.fused_env(), h.fused_env()
    one.set_gains((1.0, 0.0, 0.0))                       # one set is broadcast; `two` stays on the kernels without gains
    d, u = h.fused_actions()
    fields = tuple(f for f in PID_FIELDS if f != "last_error")

    def same_state(what):
        a, b = h.state_of(PID, one), h.state_of(PID, two)
        h.assert_states_equal(PID, a, b, what, fields)
        assert (b["last_error"] == 0).all(), what        # never read, never written
        return a["last_error"]

    h.twin_steps(one, two, d, u, 0, 12)
    moved = same_state("step")
    assert (moved != 0).sum() > 100
    assert h.twin_rollout(one, two, d[12:], u[12:]).any()
    same_state("rollout")
    h.twin_schedules(one, two)
    same_state("schedules")
    h.twin_feedback(one, two, record=True)
    h.twin_feedback(one, two, record=False)
    moved = same_state("feedback")
    assert (moved != 0).sum() > 100
    one.close(), two.close()


# ---- 3. the fused rollouts with per-env gains -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("max_steps", [pm.MAX_STEPS, pm.SHORT_MAX_STEPS])
def test_rollout_with_per_env_gains_matches_the_wrapper(max_steps):
    h.rollout_matches_the_wrapper(PID, max_steps)        # the halves: last_error is handle state, as age and cost are


@pytest.mark.gpu
@pytest.mark.parametrize("max_steps", [pm.MAX_STEPS, pm.SHORT_MAX_STEPS])
def test_rollout_schedules_with_per_env_gains_matches_the_wrapper(max_steps):
    h.rollout_schedules_matches_the_wrapper(PID, max_steps)


@pytest.mark.gpu
@pytest.mark.parametrize("max_steps", [pm.MAX_STEPS, pm.SHORT_MAX_STEPS])
def test_rollout_feedback_with_per_env_gains_matches_the_wrapper(max_steps):
    h.rollout_feedback_matches_the_wrapper(PID, max_steps)


# ---- 4. set_gains with a mask, mid-run -------------------------------------------------------------------------------------------------
MASKED = (5, 6, 7, 40, 63, 64, 69)                     # inside the full block, its last lane, the partial block's first and last
NEW_GAINS = (0.07, 0.015, 0.12)


@pytest.mark.gpu
def test_set_gains_with_a_mask_mid_run_touches_the_masked_gains_and_nothing_else():
    def change(model, e):
        model.gains = NEW_GAINS
    r = h.masked_set_mid_run(PID, MASKED, lambda env, mask: env.set_gains(NEW_GAINS, mask=mask), change, own=("gains",))
    assert (r.before["last_error"] != 0).any()
    assert_same(r.after["gains"][r.m], np.tile(NEW_GAINS, (r.m.sum(), 1)), "masked gains")
    assert (r.st["x"][r.m] != r.last["x"][r.m]).any()


# ---- 5. reset ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_reset_clears_the_last_error_of_the_masked_envs_and_keeps_their_gains():
    gi, _, _, _ = h.step_layout(PID, h.N70)
    env = h.step_env(PID, h.N70, 20, 10, gains=False)
    env.set_gains(T(GAINS[gi]))
    r = h.reset_mid_run(PID, MASKED, env)
    assert (r.before["last_error"][list(MASKED)] != 0).all()
    assert (r.after["last_error"][r.m] == 0).all() and (r.after["now"][r.m] == 0).all()
    assert_same(r.after["gains"], r.before["gains"], "the gains survive a reset")


# ---- 6. refusals and surface ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_set_gains_refusals_come_before_any_launch_and_the_env_has_the_new_verbs():
    import torch
    import gymwipe_amd
    from gymwipe_amd import _native as nat
    N = 128
    some = torch.zeros((N, 3), dtype=torch.float64, device="cuda")
    env, L = h.refusals_come_before_any_launch(PID, "set_gains", (("gains", (N, 3), np.float64), ("last_error", (N,), np.float64)), [some],
                                               ["gains_dev"], [([1.0, 0.0],), (np.zeros((N - 1, 3)),), (np.zeros((N, 4)),)])
    assert (env.get_state("gains") == [1.0, 0.0, 0.0]).all() and (env.get_state("last_error") == 0).all()
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
