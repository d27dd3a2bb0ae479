"""
gw_rollout_controller / gw_rollout_controller_population, the part that needs no GPU: the restatement of a finite-state
controller's draw and transition (actions.controller_step_numpy / controller_move_numpy) on hand-computed rows, the argument
rules of actions.make_controller, the reference loop the GPU file compares against (oracle_controller_steps(): the restatement,
CtOracle.step, the difference of CtOracle.get("n_delivered") across the step, actions.score_numpy, actions.episodes_numpy fed
the score, CtOracle.reset(mask), the transition), the premise that a controller with a delivered bit out-delivers round-robin
and stays below the queue-aware scheduler, argument validation of the two entry points, the catalogue of the two fused
families, and agents.ControllerSearchAgent on the oracle alone.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from gymwipe_amd import actions

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from util import kernel_instantiations

CENTER, MAX_DURATION = 65536, 20        # counter_traffic.py:35, envs/core.py:25 (the default configuration)
NAMES = ("device", "duration", "obs", "reward", "done", "ended", "delivered", "node")
DTYPES = (np.int32, np.int32, np.int32, np.float32, np.uint8, np.uint8, np.int32, np.uint8)


def delivered_now(orc):
    return orc.get("n_delivered").astype(np.int64).copy()


def oracle_controller_steps(orc, controller, score, steps, seed, step0, env_id0, obs_prev, state, node, max_steps, on_done,
                            center=CENTER):
    """The oracle under the controller with episodes scored by ``score``: the eight [steps][n] outputs in NAMES' order
    (``reward`` holds the score, ``node`` the node each step was taken at), the built-in reward [steps][n] beside them, the
    observation each env acts on next and the episode tally; ``state`` ({age, ret}, int32[n][2]) and ``node`` (uint8[n]) are
    updated in place."""
    n = orc.n
    out = [np.empty((steps, n), t) for t in DTYPES]
    plain = np.empty((steps, n), np.float32)
    tally = np.zeros(actions.EP_COLS, np.int64)
    acts_on = np.asarray(obs_prev, np.int32).copy()
    assert node.dtype == np.uint8 and node.shape == (n,)
    for k in range(steps):
        d, u, at = actions.controller_step_numpy(seed, env_id0, env_id0 + n, step0 + k, controller, node, acts_on, center,
                                                 MAX_DURATION)
        before = delivered_now(orc)
        obs, r, dn = orc.step(d, u)
        dl = (delivered_now(orc) - before).astype(np.int32)
        sc = actions.score_numpy(score, r, d, dl)
        ended, t = actions.episodes_numpy(state, sc, dn, max_steps, on_done)
        tally += t
        if ended.any():
            orc.reset((ended != 0).astype(np.uint8))
        node[:] = actions.controller_move_numpy(controller, at, obs, dl, ended, center)
        for a, v in zip(out, (d, u, obs, sc.astype(np.float32), dn, ended, dl, at)):
            a[k] = v
        plain[k] = r
        acts_on = np.where(ended != 0, center, obs).astype(np.int32)
    return tuple(out), plain, acts_on, tally


def one_hot(A, a):
    """The row that draws action ``a`` whatever the hash says."""
    row = np.zeros(A, np.uint32)
    row[a:] = 0xffffffff
    return row


# ---- 1. the restatement -------------------------------------------------------------------------------------------------------------
def test_the_restatement_on_hand_computed_rows():
    D, A = 2, 2 * MAX_DURATION
    S = 3
    cdf = np.zeros((S, 3, A), np.uint32)
    for n in range(S):
        for c in range(3):
            cdf[n, c] = one_hot(A, 10 * n + 3 * c + 1)          # node n, class c: action 10 n + 3 c + 1, with certainty
    nxt = np.array([[[1, 2], [0, 1], [2, 0]],
                    [[2, 2], [1, 0], [0, 7]],                   # 7 >= S: clamps to node 2
                    [[0, 1], [200, 2], [1, 1]]], np.uint8)      # 200 >= S: clamps to node 2
    need = np.array([0, 255, 3], np.uint8)
    ctl = (cdf, nxt, need)
    # the draw: node 9 >= S acts as node 2; the classes are below / at / above the centre
    node = np.array([0, 1, 2, 9, 1], np.uint8)
    obs = np.array([CENTER - 2, CENTER, CENTER + 2, CENTER, CENTER + 2], np.int32)
    dev, dur, at = actions.controller_step_numpy(5, 0, 5, 17, ctl, node, obs, CENTER, MAX_DURATION)
    acts = [1, 14, 27, 24, 17]
    assert at.tolist() == [0, 1, 2, 2, 1] and at.dtype == np.uint8
    assert dev.tolist() == [a // MAX_DURATION for a in acts] and dur.tolist() == [a % MAX_DURATION for a in acts]
    assert dev.dtype == dur.dtype == np.int32
    # a deterministic row does not depend on the stream; a row with two steps does, exactly at its threshold
    again = actions.controller_step_numpy(99, 1000, 1005, 3, ctl, node, obs, CENTER, MAX_DURATION)
    assert again[0].tolist() == dev.tolist() and again[1].tolist() == dur.tolist()
    half = cdf.copy()
    half[0, 1] = one_hot(A, 30)
    half[0, 1, 5:30] = 1 << 31                                  # u < 2^31: action 5; otherwise action 30
    u = actions.policy_u_numpy(5, 0, 64, 0)
    d2, u2, _ = actions.controller_step_numpy(5, 0, 64, 0, (half, nxt, need), np.zeros(64, np.uint8), np.full(64, CENTER), CENTER,
                                              MAX_DURATION)
    assert ((d2 * MAX_DURATION + u2) == np.where(u < (1 << 31), 5, 30)).all() and 0 < (u < (1 << 31)).sum() < 64
    # the transition: need 0 -> the bit is always set; need 255 -> never; need 3 -> delivered >= 3
    #                  node  new obs      delivered  ended   -> next[n][cls][b]
    rows = [(0, CENTER - 2, 0, 0, 2),      # next[0][0][1]: need 0, zero packets still set the bit
            (0, CENTER, 0, 0, 1),          # next[0][1][1]
            (1, CENTER, 250, 0, 1),        # next[1][1][0]: need 255 is never reached
            (1, CENTER + 2, 255, 0, 2),    # next[1][2][1] = 7, clamped to S - 1 (delivered == need sets the bit)
            (2, CENTER, 2, 0, 2),          # next[2][1][0] = 200, clamped
            (2, CENTER, 3, 0, 2),          # next[2][1][1]
            (2, CENTER - 2, 3, 0, 1),      # next[2][0][1]
            (9, CENTER - 2, 2, 0, 0),      # node 9 acts as node 2: next[2][0][0]
            (2, CENTER + 2, 9, 1, 0),      # the step ended an episode: node 0 whatever the tables say
            (1, CENTER + 2, 9, 2, 0)]
    got = actions.controller_move_numpy(ctl, np.array([r[0] for r in rows], np.uint8), np.array([r[1] for r in rows], np.int32),
                                        np.array([r[2] for r in rows], np.int32), np.array([r[3] for r in rows], np.uint8), CENTER)
    assert got.dtype == np.uint8 and got.tolist() == [r[4] for r in rows]
    # a tie of classes is no tie: the class is the sign, so CENTER + 1 and CENTER + 2 are one class
    a = actions.controller_move_numpy(ctl, np.array([0, 0], np.uint8), np.array([CENTER + 1, CENTER + 2]), [0, 0], [0, 0], CENTER)
    assert a.tolist() == [0, 0]                                 # next[0][2][1]


def test_make_controller_argument_rules_and_the_two_builders():
    D, A = 3, 3 * MAX_DURATION
    cdf = actions.policy_cdf(np.full((2, 3, A), 1.0 / A))
    nxt = np.zeros((2, 3, 2), np.int64)
    nxt[0] = 1
    c, x, d = actions.make_controller(D, cdf, nxt, [4, 255])
    assert c.dtype == np.uint32 and c.shape == (2, 3, A) and x.dtype == np.uint8 and x.shape == (2, 3, 2)
    assert d.dtype == np.uint8 and d.tolist() == [4, 255] and (c == cdf).all() and (x == nxt).all()
    big = actions.policy_cdf(np.full((17, 3, A), 1.0 / A))
    falling = cdf.copy()
    falling[1, 2, 5] = 0
    for bad in (dict(num_devices=1, cdf=cdf, next=nxt, need=[0, 0]), dict(num_devices=33, cdf=cdf, next=nxt, need=[0, 0]),
                dict(num_devices=4, cdf=cdf, next=nxt, need=[0, 0]),                    # A does not match
                dict(num_devices=D, cdf=cdf[0], next=nxt, need=[0, 0]), dict(num_devices=D, cdf=big, next=np.zeros((17, 3, 2), int),
                                                                              need=np.zeros(17, int)),
                dict(num_devices=D, cdf=cdf[:0], next=nxt[:0], need=[]), dict(num_devices=D, cdf=falling, next=nxt, need=[0, 0]),
                dict(num_devices=D, cdf=cdf.astype(np.float64), next=nxt, need=[0, 0]),
                dict(num_devices=D, cdf=cdf, next=nxt + 2, need=[0, 0]), dict(num_devices=D, cdf=cdf, next=nxt - 1, need=[0, 0]),
                dict(num_devices=D, cdf=cdf, next=nxt[:, :2], need=[0, 0]), dict(num_devices=D, cdf=cdf, next=nxt, need=[0, 256]),
                dict(num_devices=D, cdf=cdf, next=nxt, need=[0, -1]), dict(num_devices=D, cdf=cdf, next=nxt, need=[0]),
                dict(num_devices=D, cdf=cdf, next=nxt, need=[0.5, 1])):
        with pytest.raises(ValueError):
            actions.make_controller(**bad)
    rr = actions.round_robin_controller(4, 19)
    sw = actions.stay_while_productive_controller(4, 19, 8)
    assert rr[0].shape == sw[0].shape == (4, 3, 80) and (rr[0] == sw[0]).all() and rr[2].tolist() == [255] * 4
    assert sw[2].tolist() == [8] * 4 and sw[1][:, :, 0].tolist() == rr[1][:, :, 1].tolist() == [[1] * 3, [2] * 3, [3] * 3, [0] * 3]
    assert sw[1][:, :, 1].tolist() == [[i] * 3 for i in range(4)]
    for node in range(4):                                        # node i serves sender i for 19, whatever it sees
        dev, dur, _ = actions.controller_step_numpy(3, 0, 6, 0, sw, np.full(6, node, np.uint8), CENTER + np.array([-2, 0, 2] * 2),
                                                    CENTER, MAX_DURATION)
        assert dev.tolist() == [node] * 6 and dur.tolist() == [19] * 6
    pop = actions.make_controller_population([rr, sw])
    assert [a.shape for a in pop] == [(2, 4, 3, 80), (2, 4, 3, 2), (2, 4)] and (pop[2][1] == 8).all()
    with pytest.raises(ValueError):
        actions.make_controller_population([rr, actions.round_robin_controller(3, 19)])
    with pytest.raises(ValueError):
        actions.make_controller_population([])


# ---- 2. the reference loop ------------------------------------------------------------------------------------------------------------
def test_the_reference_loop_with_one_node_is_the_scored_composition():
    from test_rollout_scored_cpu import new_oracle, oracle_scored_steps
    D, n, steps = 4, 64, 24
    rng = np.random.default_rng(3)
    cdf = actions.policy_cdf(rng.dirichlet(np.full(D * MAX_DURATION, 0.3), size=3))
    score = actions.make_score(D, reward=3, delivered=[5, -7, 11, 13])
    ctl = actions.make_controller(D, cdf[None], np.zeros((1, 3, 2), np.uint8), [2])
    a, b = new_oracle(D, n), new_oracle(D, n)
    sa, sb = np.zeros((n, 2), np.int32), np.zeros((n, 2), np.int32)
    node = np.full(n, 7, np.uint8)                              # any stored node is node 0 of a one-node controller
    want = oracle_scored_steps(a, cdf, score, steps, 5, 2, 100, a.reset(), sa, 5, True)
    got = oracle_controller_steps(b, ctl, score, steps, 5, 2, 100, b.reset(), sb, node, 5, True)
    for name, x, y in zip(NAMES, got[0], want[0]):
        assert x.dtype == y.dtype and (x.view(np.uint8) == y.view(np.uint8)).all(), name
    assert (got[0][7] == 0).all() and (node == 0).all()
    assert (got[1] == want[1]).all() and (got[2] == want[2]).all() and (got[3] == want[3]).all() and (sa == sb).all()
    assert want[3][0] > 0 and got[0][6].sum() > 0


# ---- 3. the premise -------------------------------------------------------------------------------------------------------------------
def test_a_delivered_bit_out_delivers_round_robin_and_stays_below_the_queue_aware_scheduler():
    """D = 4, counter_interval = 0.02, 32 envs behind tests/test_rollout_backlog_cpu.py's prologue, 96 steps in episodes of 8,
    through the restatement.  Counts of this run: round-robin at duration 19: 18 126 packets (the figure that file pins);
    stay-while-productive (19, need 8): 20 286; need 255: round-robin's trajectory; need 6: 17 280; the backlog default:
    23 895 -- the controller closes 37 % of the gap between round-robin and the scheduler that reads the queues."""
    import test_rollout_backlog_cpu as bl
    D, n, K, E = 4, 32, 96, 8
    neutral = actions.make_score(D)

    def prepared():
        orc = bl.new_oracle(D, n, bl.MODERATE)
        dev, dur = bl.prologue_actions(D, n)
        orc.reset()
        for k in range(bl.PROLOGUE):
            orc.step(dev[k], dur[k])
        return orc, orc.reset(bl.prologue_mask(n))

    def run(ctl):
        orc, obs = prepared()
        out, _, _, tally = oracle_controller_steps(orc, ctl, neutral, K, 1, 0, 0, obs, np.zeros((n, 2), np.int32),
                                                   np.zeros(n, np.uint8), E, True)
        assert tally[0] == n * (K // E)
        return int(out[6].sum()), out

    rr, rr_out = run(actions.round_robin_controller(D, 19))
    assert (rr_out[0] == (np.arange(K) % D)[:, None]).all() and (rr_out[1] == 19).all()
    stay, stay_out = run(actions.stay_while_productive_controller(D, 19, 8))
    never, never_out = run(actions.stay_while_productive_controller(D, 19, 255))
    six, _ = run(actions.stay_while_productive_controller(D, 19, 6))
    ten, ten_out = run(actions.stay_while_productive_controller(D, 19, 10))
    orc, _ = prepared()
    pol = actions.make_backlog_policy(D)
    bout, _, _ = bl.oracle_chosen_steps(orc, lambda k, q: actions.backlog_sample_numpy(pol, q, MAX_DURATION), neutral, K,
                                        np.zeros((n, 2), np.int32), E, True)
    backlog = int(bout[4].sum())
    print("round-robin 19: %d, stay-while-productive (19, 8): %d, need 6: %d, need 10: %d, need 255: %d, backlog: %d"
          % (rr, stay, six, ten, never, backlog))
    for a, b in zip(never_out, rr_out):                          # need 255: a step never delivers that many
        assert (a == b).all()
    assert never == rr
    assert (stay_out[0] != rr_out[0]).any() and (stay_out[7] == stay_out[0]).all()
    assert stay > rr, (stay, rr)
    assert backlog > stay and backlog > rr, (backlog, stay, rr)
    assert int(rr_out[6].max()) <= 9 and ten == rr               # duration 19 carries at most 9 packets


# ---- 4. argument validation -----------------------------------------------------------------------------------------------------------
def test_argument_validation_without_a_gpu(native_lib):
    from gymwipe_amd import _native as nat
    L = native_lib
    one = 16
    fake = C.c_void_p(4096)                                             # never dereferenced: validation comes first
    ep = nat.Episodes(5, 1, one, None)                                  # tally_dev may be NULL
    ok = nat.Score.from_buffer_copy(actions.make_score(4, 1, 3).tobytes())

    def image(**kw):
        w = actions.make_score(4, 1, 3).astype(np.int32)
        for i, v in kw.items():
            w[int(i[1:])] = v
        return nat.Score.from_buffer_copy(w.tobytes())

    def ctl(S=3, cdf=one, nxt=one, need=one, node=one):
        return nat.Controller(S, cdf, nxt, need, node)

    def pop(P=3, M=128, S=3, cdf=one, nxt=one, need=one, node=one, tally=one):
        return nat.ControllerPopulation(P, M, S, cdf, nxt, need, node, tally)

    def records(env=fake, steps=4, c=ctl(), ep=ep, score=ok, ptrs=(one,) * 10):
        return L.gw_rollout_controller(env, steps, C.byref(c) if c is not None else None, 1, 0, 0,
                                       C.byref(ep) if ep is not None else None, C.byref(score) if score is not None else None,
                                       *ptrs, None)

    def population(env=fake, steps=4, c=pop(), ep=ep, score=ok, ptrs=(one,) * 2):
        return L.gw_rollout_controller_population(env, steps, C.byref(c) if c is not None else None, 1, 0, 0,
                                                  C.byref(ep) if ep is not None else None,
                                                  C.byref(score) if score is not None else None, *ptrs, None)

    for call, make, holes in ((records, ctl, 10), (population, pop, 2)):
        assert call(env=None) == nat.EINVAL and b"env is NULL" in L.gw_last_error()
        assert call(c=None) == nat.EINVAL and b"NULL" in L.gw_last_error()
        assert call(score=None) == nat.EINVAL and b"NULL" in L.gw_last_error()
        assert call(ep=None) == nat.EINVAL and b"NULL" in L.gw_last_error()
        assert call(ep=nat.Episodes(5, 1, None, one)) == nat.EINVAL and b"NULL" in L.gw_last_error()
        assert call(steps=-1) == nat.EINVAL and b"steps" in L.gw_last_error()
        assert call(ep=nat.Episodes(-1, 1, one, one)) == nat.EINVAL and b"max_steps" in L.gw_last_error()
        for hole in range(holes):                                       # every pointer in turn, node_out_dev last
            ptrs = (one,) * hole + (None,) + (one,) * (holes - 1 - hole)
            assert call(ptrs=ptrs) == nat.EINVAL and b"NULL" in L.gw_last_error(), hole
            assert call(ptrs=ptrs, steps=0) == nat.EINVAL, hole         # (before steps == 0 is looked at)
        for array in ("cdf", "nxt", "need", "node"):                    # every array of the controller
            assert call(c=make(**{array: None})) == nat.EINVAL and b"NULL" in L.gw_last_error(), array
            assert call(c=make(**{array: None}), steps=0) == nat.EINVAL, array
        for S in (0, -1, nat.FSC_MAX_STATES + 1):
            assert call(c=make(S=S)) == nat.EINVAL and b"num_states" in L.gw_last_error(), S
            assert call(c=make(S=S), steps=0) == nat.EINVAL, S
        for bad in (image(w0=nat.SCORE_W_MAX + 1), image(w0=-nat.SCORE_W_MAX - 1), image(w2=nat.SCORE_W_MAX + 1),
                    image(w32=-nat.SCORE_W_MAX - 1)):
            assert call(score=bad) == nat.EINVAL and b"weight" in L.gw_last_error()
            assert call(score=bad, steps=0) == nat.EINVAL
        assert call(steps=0) == nat.OK
        assert call(steps=0, c=make(S=1)) == nat.OK and call(steps=0, c=make(S=nat.FSC_MAX_STATES)) == nat.OK
        assert call(steps=0, ep=nat.Episodes(0, 0, one, None)) == nat.OK
    assert population(c=pop(tally=None)) == nat.EINVAL and b"NULL" in L.gw_last_error()
    for P, M in ((0, 128), (3, 0), (-1, 128)):
        assert population(c=pop(P=P, M=M)) == nat.EINVAL and b">= 1" in L.gw_last_error()
        assert population(c=pop(P=P, M=M), steps=0) == nat.EINVAL


# ---- 5. the catalogue -----------------------------------------------------------------------------------------------------------------
def test_the_controller_instantiations_are_the_librarys(native_lib):
    from gymwipe_amd import _native
    import test_rollout_controller as rc
    for family, cases in (("ct_rollout_fsc", rc.INSTANTIATIONS), ("ct_rollout_fsc_pop", rc.POP_INSTANTIATIONS)):
        lib_set = kernel_instantiations(_native.LIB_PATH, family)
        assert len(lib_set) == 30, sorted(lib_set)
        assert sorted(lib_set - set(cases)) == [], "instantiations the catalogue does not name"
        assert sorted(set(cases) - lib_set) == [], "names for instantiations the library does not have"


# ---- 6. the agent on the oracle -------------------------------------------------------------------------------------------------------
AGENT = dict(D=4, P=4, M=64, steps=16, episode_steps=8, generations=3, seed=0)


def oracle_agent(cfg=None):
    """ControllerSearchAgent with the oracle standing in for the GPU: fresh envs before every generation, as the default
    evaluate restores the snapshot it took behind env.reset(); controller p on envs [p M, (p + 1) M)."""
    from gymwipe_amd.agents import ControllerSearchAgent
    from test_rollout_scored_cpu import new_oracle
    cfg = cfg or AGENT
    D, P, M = cfg["D"], cfg["P"], cfg["M"]
    score = actions.make_score(D, reward=0, delivered=1)

    def evaluate(population, generation):
        tally = np.zeros((P, actions.EP_COLS), np.int64)
        for p in range(P):
            orc = new_oracle(D, M)
            ctl = tuple(a[p] for a in population)
            _, _, _, tally[p] = oracle_controller_steps(orc, ctl, score, cfg["steps"], cfg["seed"], generation * cfg["steps"], p * M,
                                                        orc.reset(), np.zeros((M, 2), np.int32), np.zeros(M, np.uint8),
                                                        cfg["episode_steps"], True)
        return tally

    return ControllerSearchAgent(None, P, cfg["steps"], cfg["episode_steps"], seed=cfg["seed"], evaluate=evaluate, num_devices=D,
                                 score=score)


def test_controller_search_starts_at_stay_while_productive_and_is_deterministic():
    one, two = oracle_agent(), oracle_agent()
    start = one.controller()
    want = actions.stay_while_productive_controller(AGENT["D"], MAX_DURATION - 1, 8)
    assert (start[1] == want[1]).all() and (start[2] == want[2]).all()
    for node in range(AGENT["D"]):                               # the start's rows: sender `node` for duration 19, nearly always
        dev, dur, _ = actions.controller_step_numpy(1, 0, 512, 0, start, np.full(512, node, np.uint8), np.full(512, CENTER), CENTER,
                                                    MAX_DURATION)
        assert (dur == MAX_DURATION - 1).all() and (dev == node).mean() > 0.97
    h = one.fit(AGENT["generations"])
    two.fit(AGENT["generations"])
    assert len(h) == AGENT["generations"]
    for x, y in zip(h, two.history):
        assert x["mean"] == y["mean"] and x["best"] == y["best"] and (x["fitness"] == y["fitness"]).all()
    assert (one.mu == two.mu).all() and (one.sigma == two.sigma).all()
    assert all(np.isfinite(e["fitness"]).all() and (e["fitness"] >= 0).all() and e["best"] > 0 for e in h)
    assert h[0]["of_mu"] == h[0]["fitness"][0] > 0
    made = one.controller()
    assert made[0].shape == (AGENT["D"], 3, AGENT["D"] * MAX_DURATION) and int(made[1].max()) < AGENT["D"]
