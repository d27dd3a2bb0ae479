"""gw_ctrl_rollout_feedback on the GPU: angle-feedback band schedulers inside the fused control-loop rollout.  The specification is
the event-driven ControlLoopModel under the rules restated in tests/ctrl_feedback_model.py, and every comparison is bit for bit
unless stated.  Env e follows stream (5 e + e // 64) % 8 of X0S / U0S (tests/test_ctrl_rollout.py) and policy e // (N / P); the
fixture policies are defined in ctrl_feedback_model.py and checked on the model alone in tests/test_ctrl_feedback_cpu.py (every
bin visited, resets into several bins, both ending causes, angles far inside the int32 observation's range).
The key (|o| or o) is one flag per call, and fixtures 1 and 2 are made for |o|, fixture 3 for o: the launches of all three run
once under each key, the second with the short step limit.  Their common L is 6, a multiple of every schedule's length, so the
cyclic padding changes nothing and each policy's reference is the one computed at its own length."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctrl_feedback_model as fm
import test_ctrl_rollout as g
from ctrl_episodes_model import FIELDS
from test_ctrl_rollout import T, assert_same, assert_states_equal, make_env, state_of

K = fm.STEPS
ROWS = ("device", "duration", "obs", "reward", "angle", "ended")
COUNTS, SUMS = (0, 1, 2, 4, 7), (3, 5, 6)                               # tally columns: whole numbers, running f64 sums


def policies_of(names, L=None):
    from gymwipe_amd import actions
    return actions.make_ctrl_feedback([list(fm.FIXTURES[n][2]) for n in names], [list(fm.FIXTURES[n][1]) for n in names], L)


def reference(names, abs_key, max_steps, N):
    """The model's rows [K][N], tally [N][8] and final state {field: [N]...} for N envs under the policies `names`."""
    so, p_of = g.stream_of(N), np.arange(N) // (N // len(names))
    refs = [fm.fixture_streams(n, abs_key, max_steps) for n in names]
    tally = np.stack([refs[p][0][s] for p, s in zip(p_of, so)])
    rows = {f: np.stack([refs[p][1][f][:, s] for p, s in zip(p_of, so)], 1) for f in ROWS}
    final = {f: np.stack([refs[p][2][f][s] for p, s in zip(p_of, so)]) for f in FIELDS + ("age", "cost")}
    return rows, tally, final


def run(env, sched, edges, max_steps, steps=K, abs_key=True, record=True):
    out = env.rollout_feedback(T(sched) if isinstance(sched, np.ndarray) else sched, T(edges) if isinstance(edges, np.ndarray) else edges,
                               (max_steps, fm.FAIL_DEG), steps, abs_key=abs_key, record=record)
    return tuple(v.cpu().numpy() for v in out[:2]) + (({f: v.cpu().numpy() for f, v in out[2].items()},) if record else ())


# (names, abs_key or None for the fixture's own, max_steps, N, L)
CASES = [((1,), None, fm.MAX_STEPS, 256, None), ((2,), None, fm.MAX_STEPS, 256, None), ((3,), None, fm.MAX_STEPS, 256, None),
         ((4,), None, fm.MAX_STEPS, 256, None), ((1, 2, 3), True, fm.MAX_STEPS, 192, 6), ((1, 2, 3), False, fm.SHORT_MAX_STEPS, 192, 6)]


# ---- 1. model parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("names,abs_key,max_steps,N,L", CASES)
def test_rollout_feedback_matches_the_model(names, abs_key, max_steps, N, L):
    P, M = len(names), N // len(names)
    key = fm.FIXTURES[names[0]][0] if abs_key is None else abs_key
    w_rows, w_tally, final = reference(names, abs_key, max_steps, N)
    sched, edges = policies_of(names, L)
    env = make_env(N, own_states=True)
    tally, sums, rows = run(env, sched, edges, max_steps, abs_key=key)
    assert tally.shape == (N, 8) and sums.shape == (P, 8)
    for f in ROWS:
        assert_same(rows[f], w_rows[f], f)
    for col in range(8):
        assert_same(tally[:, col], w_tally[:, col], ("tally", col))
    st = state_of(env)
    for f in FIELDS + ("age", "cost"):
        assert_same(st[f], final[f], f)
    assert not (st["flags"] & (3 | 8)).any()                             # no tie, no carry, and never GW_FLAG_BADACT
    for p in range(P):
        mine = tally[p * M:(p + 1) * M]
        for col in COUNTS:
            assert sums[p, col] == mine[:, col].sum(), (p, col)
        assert sums[p, 2] == K * M
        for col in SUMS:
            exact = math.fsum(mine[:, col].tolist())
            assert abs(sums[p, col] - exact) <= M * 2.0 ** -52 * exact, (p, col, sums[p, col], exact)
    env.close()


# ---- 2. without rows -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("names,abs_key,max_steps,N,L", [CASES[3], CASES[5]])
def test_rollout_feedback_without_rows_leaves_the_same_state_and_tally(names, abs_key, max_steps, N, L):
    key = fm.FIXTURES[names[0]][0] if abs_key is None else abs_key
    sched, edges = policies_of(names, L)
    with_rows, without = make_env(N, own_states=True), make_env(N, own_states=True)
    a = run(with_rows, sched, edges, max_steps, abs_key=key)
    b = run(without, sched, edges, max_steps, abs_key=key, record=False)
    assert len(a) == 3 and len(b) == 2
    assert_same(b[0], a[0], "tally") and assert_same(b[1], a[1], "sums")
    assert_states_equal(state_of(without), state_of(with_rows), "without rows")
    assert_same(b[0], reference(names, abs_key, max_steps, N)[1], "tally against the model")
    with_rows.close(), without.close()


# ---- 3. B = 1 is the schedule call -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("P,L", [(4, 3), (2, 64), (1, 1)])
@pytest.mark.parametrize("abs_key", [True, False])
def test_rollout_feedback_with_one_bin_is_rollout_schedules(P, L, abs_key):
    N = 256
    sch = g.schedules_of(P, L)                                           # uint8[P][L][2], bytes outside the action space among them
    env, twin = make_env(N, own_states=True), make_env(N, own_states=True)
    tally, sums = run(env, np.ascontiguousarray(sch[:, None]), np.zeros((P, 0), np.int32), g.SCHED_MAX, abs_key=abs_key, record=False)
    w_tally, w_sums = twin.rollout_schedules(T(sch), (g.SCHED_MAX, g.SCHED_FAIL), K)
    assert_same(tally[:, :4], w_tally.cpu().numpy(), "tally")
    assert_same(sums[:, :3], w_sums.cpu().numpy()[:, :3], "sums")        # (column 3 is a torch reduction over another stride: test 1's bound)
    M = N // P
    for p in range(P):
        exact = math.fsum(tally[p * M:(p + 1) * M, 3].tolist())
        assert abs(sums[p, 3] - exact) <= M * 2.0 ** -52 * exact, (p, sums[p, 3], exact)
    assert (tally[:, 7] == K).all()                                      # one bin: every step is taken in bin 0
    assert_states_equal(state_of(env), state_of(twin), "rollout_schedules")
    env.close(), twin.close()


# ---- 4. replay -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rollout_replays_the_actions_the_feedback_call_took():
    names, abs_key, max_steps, N, L = CASES[5]
    sched, edges = policies_of(names, L)
    env, twin = make_env(N, own_states=True), make_env(N, own_states=True)
    _, _, rows = run(env, sched, edges, max_steps, abs_key=abs_key)
    obs, rew, ended, info = twin.rollout(T(rows["device"]), T(rows["duration"]), episodes=(max_steps, fm.FAIL_DEG))
    assert_same(obs.cpu().numpy(), rows["obs"], "obs") and assert_same(rew.cpu().numpy(), rows["reward"], "reward")
    assert_same(info["Sensor angle"].cpu().numpy(), rows["angle"], "angle") and assert_same(ended.cpu().numpy(), rows["ended"], "ended")
    assert_states_equal(state_of(twin), state_of(env), "replayed")
    env.close(), twin.close()


# ---- 5. split --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("names,abs_key,max_steps,N,L", [CASES[1], CASES[5]])
def test_two_calls_of_half_the_steps_equal_one_call(names, abs_key, max_steps, N, L):
    key = fm.FIXTURES[names[0]][0] if abs_key is None else abs_key
    sched, edges = policies_of(names, L)
    one, halves = make_env(N, own_states=True), make_env(N, own_states=True)
    tally, _, rows = run(one, sched, edges, max_steps, abs_key=key)
    a = run(halves, sched, edges, max_steps, steps=K // 2, abs_key=key)
    b = run(halves, sched, edges, max_steps, steps=K - K // 2, abs_key=key)
    for f in ROWS:
        assert_same(np.concatenate([a[2][f], b[2][f]]), rows[f], f)
    assert_states_equal(state_of(halves), state_of(one), "halves")
    for col in COUNTS:                                                   # (the f64 sums restart at 0 in the second call)
        assert_same(a[0][:, col] + b[0][:, col], tally[:, col], ("tally", col))
    one.close(), halves.close()


# ---- 6. the policies are read when the launch runs -------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rewriting_a_policy_in_device_memory_changes_the_second_call_only():
    import torch
    N, L, half = 256, 6, K // 2
    first, second = policies_of((1,), L), policies_of((2,), L)
    sched, edges = T(first[0]).cuda(), T(first[1]).cuda()
    ptrs = (sched.data_ptr(), edges.data_ptr())
    env, twin, same = make_env(N, own_states=True), make_env(N, own_states=True), make_env(N, own_states=True)
    a = run(env, sched, edges, fm.MAX_STEPS, steps=half)
    sched.copy_(T(second[0]))                                            # in place, stream-ordered behind the first call
    edges.copy_(T(second[1]))
    assert (sched.data_ptr(), edges.data_ptr()) == ptrs
    b = run(env, sched, edges, fm.MAX_STEPS, steps=half)
    torch.cuda.synchronize()
    wa = run(twin, first[0], first[1], fm.MAX_STEPS, steps=half)         # the same from fresh uploads
    wb = run(twin, second[0], second[1], fm.MAX_STEPS, steps=half)
    for f in ROWS:
        assert_same(a[2][f], wa[2][f], ("first call", f)) and assert_same(b[2][f], wb[2][f], ("second call", f))
    assert_same(a[0], wa[0], "first tally") and assert_same(b[0], wb[0], "second tally")
    assert_states_equal(state_of(env), state_of(twin), "rewritten")
    w_rows, _, _ = reference((1,), None, fm.MAX_STEPS, N)                # the first call followed policy 1 ...
    for f in ROWS:
        assert_same(a[2][f], w_rows[f][:half], ("policy 1", f))
    run(same, first[0], first[1], fm.MAX_STEPS, steps=half)
    c = run(same, first[0], first[1], fm.MAX_STEPS, steps=half)
    assert (c[2]["duration"] != b[2]["duration"]).any() and (c[2]["angle"] != b[2]["angle"]).any()      # ... the second did not
    for e in (env, twin, same):
        e.close()


# ---- 7. refusal ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rollout_feedback_refuses_blocks_that_would_span_two_policies():
    from gymwipe_amd import _native as nat
    env = make_env(192, own_states=True)
    before = state_of(env)
    sched, edges = policies_of((1, 2), 6)
    for record in (False, True):
        with pytest.raises(nat.NativeError) as err:
            env.rollout_feedback(T(sched), T(edges), (fm.MAX_STEPS, fm.FAIL_DEG), 10, record=record)
        assert err.value.code == nat.EUNSUPPORTED and "multiple of 64" in str(err.value)
    assert_states_equal(state_of(env), before, "refused")
    env.close()


# ---- 8. surface ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rollout_feedback_surface():
    import torch
    import gymwipe_amd
    N, steps = 128, 6
    env = gymwipe_amd.make("VecControlLoop-v0", num_envs=N)
    sched, edges = policies_of((1, 3))
    out = env.rollout_feedback(T(sched), T(edges), (4, 0.0), steps)
    assert isinstance(out, tuple) and len(out) == 2                      # record=False: no rows
    tally, sums = out
    assert tally.shape == (N, 8) and sums.shape == (2, 8) and tally.dtype == sums.dtype == torch.float64 and tally.is_cuda
    assert (tally[:, 2] == steps).all() and (tally[:, 0] == 1).all() and (tally[:, 1] == 0).all() and (sums[:, 2] == steps * N // 2).all()
    tally, sums, rows = env.rollout_feedback(T(sched), T(edges), (4, 0.0), steps, abs_key=False, record=True)
    assert sorted(rows) == sorted(ROWS)
    for f, dt in (("device", torch.int32), ("duration", torch.int32), ("obs", torch.int32), ("reward", torch.float32),
                  ("angle", torch.float64), ("ended", torch.uint8)):
        assert rows[f].shape == (steps, N) and rows[f].dtype == dt and rows[f].is_cuda, f
    ended = rows["ended"].cpu().numpy()
    assert (ended[1] == 1).all() and (ended[5] == 1).all() and ended.sum() == 2 * N     # age was 2 when the second call began
    assert (tally[:, 4] == rows["duration"].sum(0)).all()
    with pytest.raises(ValueError):
        env.rollout_feedback(T(sched[0]), T(edges), (4, 0.0), steps)
    with pytest.raises(ValueError):
        env.rollout_feedback(T(sched), T(edges.astype(np.int64)), (4, 0.0), steps)
    from gymwipe_amd import _native as nat
    with pytest.raises(nat.NativeError):
        env.rollout_feedback(T(sched), T(edges), None, steps)            # episodes are required
    env.close()
