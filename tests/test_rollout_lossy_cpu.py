"""
The fused rollouts where packets are lost and grants are refused, the part that needs no GPU: the references
tests/test_rollout_lossy.py compares the 16 fused families (and their per-step forms) against, and the gates that make those
references worth comparing against.

Every sibling file runs on the default layout, on which every announcement is granted and every popped packet is decoded
(n_popped == n_delivered), so a kernel that reported the packets it popped as delivered, that read the popped half of the
counter word, or whose `granted == false` branch or per-packet decode were wrong would pass all of them.  util.lossy_layout()
puts one sender where only some of its packets reach the RRM and two where no announcement is ever decoded.

The references are the sibling files' own oracle compositions (oracle_policy_steps, oracle_episode_steps, oracle_scored_steps,
oracle_population_steps, oracle_scored_population_steps, oracle_autoreset_steps, oracle_scored_autoreset_steps,
oracle_backlog_steps, the backlog population's oracle_population_steps, oracle_controller_steps, transition_stats_numpy), run
on an oracle of that layout through Tap, which records per (step, env) what the step popped, delivered and transmitted.
reference() builds a case once (lru_cache, read-only arrays) and raises RuntimeError -- instead of letting a test pass --
unless, on the reference alone:
  * every partly decoded sender that was addressed has 0 < delivered < popped, and no never-granted sender popped a packet;
  * at least MIN_CELLS (step, env) cells have 0 < delivered_k < popped_k;
  * at least MIN_CELLS cells address a never-granted sender with duration > 0 and a non-empty queue and transmit the
    announcement alone;
  * at least two senders deliver; an episodic case ends at least MIN_EPISODES episodes (per policy in a population);
  * the same composition run with the step's popped count where it reads the delivered count (Tap(swap=True)) differs from the
    true reference in one of the outputs the GPU test compares for that family (SENSITIVE): the cases would catch the confusion;
  * backlog cases: the partly decoded sender is chosen at least MIN_CELLS times; controller cases: the bit
    delivered_k >= need[n] differs from popped_k >= need[n] in at least MIN_CELLS cells.
test_the_layout_keeps_the_fused_forms_available() checks with gw_selftest_fastmath that the layout keeps every exact fast form
and a closed noise-state set, so a fused case cannot quietly become a live-PHY one.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from gymwipe_amd import actions

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_backlog_population_cpu import oracle_population_steps as oracle_backlog_population_steps      # noqa: E402
from test_kernel_variants import NEAR_LIMIT                                                              # noqa: E402
from test_rollout_autoreset import oracle_autoreset_steps                                                # noqa: E402
from test_rollout_autoreset_scored_cpu import oracle_scored_autoreset_steps                              # noqa: E402
from test_rollout_backlog_cpu import MODERATE, new_oracle as new_backlog_oracle, oracle_backlog_steps, oracle_prologue   # noqa: E402
from test_rollout_controller_cpu import oracle_controller_steps                                          # noqa: E402
from test_rollout_episodes import MIN_EPISODES, oracle_episode_steps                          # noqa: E402
from test_rollout_policy import CENTER, MAX_DURATION, SEED, oracle_policy_steps, oracle_prep, policy_table   # noqa: E402
from test_rollout_population import population_tables                                                    # noqa: E402
from test_rollout_population_cpu import oracle_population_steps                                          # noqa: E402
from test_rollout_scored_cpu import new_oracle, oracle_scored_population_steps, oracle_scored_steps      # noqa: E402
from util import LOSSY_NEVER, LOSSY_PARTLY, action_stream, lossy_layout                                  # noqa: E402

N, STEPS = 192, 70                      # three blocks; launches of 64 + 6 steps
P, M = 3, 64                            # the population families: one block per policy
MAX_STEPS = 6                           # divides neither 64 nor 70: episodes straddle the launches, and {age, ret} are not 0 at the end
MIN_CELLS = 10
LIMIT, LIMIT_STEPS = 1.0e6, 64          # the fast forms' validity limit on simulated time; one launch
STAGED_SEED = 3                         # the staged rows of gw_rollout / gw_rollout_autoreset: action_stream(3, 70, 192, D)
FLAGS_FATAL = 1 | 2                     # FLAG_CARRY | FLAG_REFEXC: what env.check() raises on
S_CASE = 3

# run kind -> the fused families it is the reference of
FAMILIES = {
    "sync": ("ct_rollout_sync_kernel",), "plain": ("ct_rollout_policy", "ct_rollout_pstats", "ct_rollout_pstats_d"),
    "episodic": ("ct_rollout_policy_ep", "ct_rollout_pstats_ep", "ct_rollout_pstats_epd"), "scored": ("ct_rollout_policy_eps",),
    "pop": ("ct_rollout_pop_ep",), "pop_scored": ("ct_rollout_pop_eps",), "auto": ("ct_rollout_sync_ep",),
    "auto_scored": ("ct_rollout_sync_eps",), "backlog": ("ct_rollout_backlog",), "backlog_pop": ("ct_rollout_backlog_pop",),
    "fsc": ("ct_rollout_fsc",), "fsc_pop": ("ct_rollout_fsc_pop",),
}
# family -> the compared outputs (keys of a run's "cmp") of which the popped-for-delivered substitute must change at least one
SENSITIVE = {
    "ct_rollout_sync_kernel": ("n_delivered",), "ct_rollout_policy": ("n_delivered",), "ct_rollout_pstats": ("n_delivered",),
    "ct_rollout_policy_ep": ("n_delivered",), "ct_rollout_pstats_ep": ("n_delivered",), "ct_rollout_pop_ep": ("n_delivered",),
    "ct_rollout_sync_ep": ("n_delivered",), "ct_rollout_pstats_d": ("table8_col7",), "ct_rollout_pstats_epd": ("table8_col7",),
    "ct_rollout_policy_eps": ("reward", "delivered", "state", "tally"), "ct_rollout_sync_eps": ("reward", "delivered", "state", "tally"),
    "ct_rollout_pop_eps": ("state", "tally"), "ct_rollout_backlog": ("reward", "delivered", "state", "tally"),
    "ct_rollout_backlog_pop": ("state", "tally"), "ct_rollout_fsc": ("node", "reward", "delivered", "state", "tally"),
    "ct_rollout_fsc_pop": ("node_dev", "state", "tally"),
}
EPISODIC = frozenset(FAMILIES) - {"sync", "plain"}


class Tap:
    """A CtOracle behind the surface the compositions use (n, D, reset, step, get), recording per step and env the sender and
    duration, the packets popped and delivered, the transmissions, the addressed sender's queue length before the step and the
    clock after it.  ``swap``: get("n_delivered") answers with the popped counter -- the composition then scores, tallies and
    moves by the packets the step popped."""

    def __init__(self, orc, swap=False):
        self.orc, self.swap, self.n, self.D = orc, swap, orc.n, orc.D
        self.clear()

    def clear(self):
        self.rows = {k: [] for k in ("dev", "dur", "pop", "dlv", "tx", "qlen", "now")}

    def reset(self, mask=None):
        return self.orc.reset(mask)

    def get(self, field):
        return self.orc.get("n_popped" if self.swap and field == "n_delivered" else field)

    def step(self, device, duration):
        o = self.orc
        d = np.asarray(device).astype(np.int64)
        before = [o.get(f).astype(np.int64) for f in ("n_popped", "n_delivered", "n_tx")]
        qlen = o.get("qlen")[np.arange(self.n), d]
        res = o.step(device, duration)
        after = [o.get(f).astype(np.int64) for f in ("n_popped", "n_delivered", "n_tx")]
        for k, v in zip(("dev", "dur", "pop", "dlv", "tx", "qlen", "now"),
                        (d, np.asarray(duration).astype(np.int64), after[0] - before[0], after[1] - before[1], after[2] - before[2],
                         qlen.astype(np.int64), o.get("now"))):
            self.rows[k].append(v)
        return res

    def rec(self, key):
        return np.stack(self.rows[key])

    def seen_delivered(self):
        """[steps][n] int32: what a composition that differences get("n_delivered") across the step reads."""
        return self.rec("pop" if self.swap else "dlv").astype(np.int32)


def layout_kw(layout, D):
    if layout == "default":
        return {}
    pos, rrm = lossy_layout(D)
    return {"positions": pos, "rrm_pos": rrm}


def env_kw(layout, D):
    """The same layout as VecCounterTrafficEnv's arguments."""
    kw = layout_kw(layout, D)
    return {"positions": kw["positions"], "rrm_position": kw["rrm_pos"]} if kw else {}


def case_score(D):
    """w_reward = 3 and a weight per sender, all distinct and none 0, every third one negative."""
    return actions.make_score(D, reward=3, delivered=[(5 + 2 * d) * (-1 if d % 3 == 2 else 1) for d in range(D)])


def never_granted(D):
    return [i for i in range(D) if i % 5 in LOSSY_NEVER]


def partly_decoded(D):
    return [i for i in range(D) if i % 5 in LOSSY_PARTLY]


def backlog_policy(D, w_never, w_other, slope, cap=9):
    """Never-granted senders weigh ``w_never``, the others ``w_other`` (sender i: w_other + i, so ties are rare): a never-granted
    sender's queue fills to its cap of 100 and stays there, so it is chosen exactly while no other priority exceeds
    100 * w_never.  duration_of_len[L] = min(cap, slope * L + 1); the partly decoded sender decodes the announcement of a
    one-digit duration only, so a cap of 9 keeps it granted and a larger one refuses it whenever its queue is long."""
    w = [w_never if i in never_granted(D) else w_other + i for i in range(D)]
    return actions.make_backlog_policy(D, w, np.minimum(cap, slope * np.arange(actions.QUEUE_CAP + 1) + 1))


def case_backlog_policy(D):
    """A never-granted sender is chosen while every other priority is below 100 (400 at D = 9, where five senders deliver and
    some queue is nearly always above 4: at weight 3 the oracle never chose one, at 4 it does 160 times)."""
    return backlog_policy(D, 1 if D <= 5 else 4, 24, 3)


def case_backlog_population(D):
    """Three policies: the never-granted senders at weight 0 (the scheduler never parks on them), at weight 1 and at weight 2
    (there with durations of up to 19, which the partly decoded sender is refused)."""
    return actions.make_backlog_population([backlog_policy(D, 0, 24, 2), backlog_policy(D, 1, 24, 3), backlog_policy(D, 2, 30, 4, 19)])


def case_controller(D, salt=0):
    """tests/test_rollout_controller.py's recipe with thresholds of 1 .. 3 packets rotated by ``salt``: a step of the partly
    decoded sender pops up to 9 packets and delivers some of them, so the thresholds separate popped from delivered."""
    A = D * MAX_DURATION
    rng = np.random.default_rng(100000 * salt + 1000 * SEED + 10 * S_CASE + D)
    p = rng.dirichlet(np.full(A, 0.3), size=(S_CASE, 3))
    nxt = rng.integers(0, S_CASE, size=(S_CASE, 3, 2))
    for n in range(S_CASE):
        nxt[n, 1, n % 2] = (n + 1) % S_CASE
    return actions.make_controller(D, actions.policy_cdf(p), nxt, 1 + (np.arange(S_CASE) + salt) % 3)


def prep_cols(lo, n):
    return np.arange(lo, lo + n) % 200                     # (the PREP stream is 200 envs wide)


def run(kind, D, swap=False, layout="lossy", start_time=None, steps=STEPS):
    """One composition on a fresh oracle: {"taps", "orcs", "cmp": the outputs the GPU test compares, by name, ...inputs}."""
    kw = dict(layout_kw(layout, D), **({"start_time": start_time} if start_time is not None else {}))
    if kind == "fsc_pop":                                   # (an oracle per controller, below)
        tap = None
    elif kind in ("backlog", "backlog_pop"):
        tap = Tap(new_backlog_oracle(D, N, MODERATE, **kw), swap)
    else:
        tap = Tap(new_oracle(D, N, **kw), swap)
    taps, res, cmp = [tap], {}, {}
    state = np.zeros((N, 2), np.int32)
    if kind in ("sync", "auto", "auto_scored"):
        dev, dur = action_stream(STAGED_SEED, steps, N, D)
        tap.reset()
        res.update(dev=dev, dur=dur, now0=tap.get("now"))
        if kind == "sync":
            rows = [np.empty((steps, N), t) for t in (np.int32, np.float32, np.uint8)]
            for k in range(steps):
                for a, v in zip(rows, tap.step(dev[k], dur[k])):
                    a[k] = v
            cmp.update(obs=rows[0], reward=rows[1], done=rows[2])
        elif kind == "auto":
            out, obs_next, tally = oracle_autoreset_steps(tap, dev, dur, state, MAX_STEPS, True)
            cmp.update(zip(("obs", "reward", "done", "ended"), out), obs_next=obs_next, state=state, tally=tally)
        else:
            res["score"] = case_score(D)
            out, _, obs_next, tally = oracle_scored_autoreset_steps(tap, dev, dur, res["score"], state, MAX_STEPS, True)
            cmp.update(zip(("obs", "reward", "done", "ended", "delivered"), out), obs_next=obs_next, state=state, tally=tally)
    elif kind in ("plain", "episodic", "scored"):
        _, cdf = policy_table(D)
        obs_prev = oracle_prep(tap, D, prep_cols(0, N))
        tap.clear()
        res.update(cdf=cdf, obs_prev=obs_prev, now0=tap.get("now"))
        if kind == "plain":
            out, _ = oracle_policy_steps(tap, cdf, steps, SEED, 0, 0, obs_prev)
            cmp.update(zip(("device", "duration", "obs", "reward", "done"), out), obs_next=out[2][-1].copy(),
                       returns=out[3].astype(np.int64).sum(axis=0).astype(np.int32))
            ended = None
        elif kind == "episodic":
            out, obs_next, tally = oracle_episode_steps(tap, cdf, steps, SEED, 0, 0, obs_prev, state, MAX_STEPS, True)
            cmp.update(zip(("device", "duration", "obs", "reward", "done", "ended"), out), obs_next=obs_next, state=state, tally=tally)
            ended = out[5]
        else:
            res["score"] = case_score(D)
            out, _, obs_next, tally = oracle_scored_steps(tap, cdf, res["score"], steps, SEED, 0, 0, obs_prev, state, MAX_STEPS, True)
            cmp.update(zip(("device", "duration", "obs", "reward", "done", "ended", "delivered"), out), obs_next=obs_next, state=state,
                       tally=tally)
        if kind != "scored":
            table8 = actions.transition_stats_numpy(obs_prev, *out[:5], CENTER, MAX_DURATION, D, ended=ended,
                                                    delivered=tap.seen_delivered())
            table7 = actions.transition_stats_numpy(obs_prev, *out[:5], CENTER, MAX_DURATION, D, ended=ended)
            assert (table8[..., :7] == table7).all()
            cmp.update(table7=table7, table8=table8, table8_col7=table8[..., 7].copy())
    elif kind in ("pop", "pop_scored"):
        cdfs = population_tables(D, P)
        obs_prev = oracle_prep(tap, D, prep_cols(0, N))
        tap.clear()
        res.update(cdfs=cdfs)
        if kind == "pop":
            obs_next, tally = oracle_population_steps(tap, cdfs, M, steps, SEED, 0, 0, obs_prev, state, MAX_STEPS, True)
        else:
            res["score"] = case_score(D)
            obs_next, tally, _ = oracle_scored_population_steps(tap, cdfs, M, res["score"], steps, SEED, 0, 0, obs_prev, state, MAX_STEPS,
                                                                True)
        cmp.update(obs_next=obs_next, state=state, tally=tally)
    elif kind in ("backlog", "backlog_pop"):
        res["score"] = case_score(D)
        oracle_prologue(tap)
        tap.clear()
        names = ("obs", "reward", "done", "ended", "delivered", "device", "duration", "seen_len")
        if kind == "backlog":
            res["policy"] = case_backlog_policy(D)
            out, obs_next, tally = oracle_backlog_steps(tap, res["policy"], res["score"], steps, state, MAX_STEPS, True)
            cmp.update(zip(names, out), obs_next=obs_next, state=state, tally=tally)
        else:
            res["population"] = case_backlog_population(D)
            _, obs_next, total, tally = oracle_backlog_population_steps(tap, res["population"], M, res["score"], steps, state, MAX_STEPS,
                                                                        True)
            cmp.update(obs_next=obs_next, state=state, tally=tally, total=total)
    elif kind == "fsc":
        res.update(score=case_score(D), controller=case_controller(D))
        obs_prev = oracle_prep(tap, D, prep_cols(0, N))
        tap.clear()
        node = np.zeros(N, np.uint8)
        out, _, obs_next, tally = oracle_controller_steps(tap, res["controller"], res["score"], steps, SEED, 0, 0, obs_prev, state, node,
                                                          MAX_STEPS, True)
        cmp.update(zip(("device", "duration", "obs", "reward", "done", "ended", "delivered", "node"), out), obs_next=obs_next,
                   state=state, tally=tally, node_dev=node)
    elif kind == "fsc_pop":                                 # controller p's envs: the records-form composition on its columns
        res.update(score=case_score(D), controllers=[case_controller(D, salt=p + 1) for p in range(P)])
        taps, outs, nexts, tallies, node = [], [], [], [], np.zeros(N, np.uint8)      # (taps: the slices', in order)
        for p in range(P):
            t = Tap(new_oracle(D, M, **kw), swap)
            obs_prev = oracle_prep(t, D, prep_cols(p * M, M))
            t.clear()
            s = slice(p * M, (p + 1) * M)
            out, _, nxt, tally = oracle_controller_steps(t, res["controllers"][p], res["score"], steps, SEED, 0, p * M, obs_prev, state[s],
                                                       node[s], MAX_STEPS, True)
            taps.append(t)
            outs.append(out)
            nexts.append(nxt)
            tallies.append(tally)
        cmp.update(obs_next=np.concatenate(nexts), state=state, tally=np.stack(tallies), node_dev=node)
        res["rows"] = {"node": np.concatenate([o[7] for o in outs], axis=1), "ended": np.concatenate([o[5] for o in outs], axis=1)}
    else:
        raise KeyError(kind)
    res["taps"], res["orcs"] = taps, [t.orc for t in taps]
    cmp["n_delivered"] = np.concatenate([t.get("n_delivered") for t in taps])
    res["cmp"] = cmp
    res["rec"] = {k: np.concatenate([t.rec(k) for t in taps], axis=1) for k in taps[0].rows}
    res["flags"] = int(np.bitwise_or.reduce(np.concatenate([t.get("flags") for t in taps])))
    return res


def measure(kind, D, res):
    """What the gates look at, counted on the reference's own records."""
    r = res["rec"]
    dev = r["dev"]
    by_sender = {i: (int(r["pop"][dev == i].sum()), int(r["dlv"][dev == i].sum())) for i in range(D)}
    never = np.isin(dev, never_granted(D))
    m = {"by_sender": by_sender,
         "partly_cells": int(((r["dlv"] > 0) & (r["dlv"] < r["pop"])).sum()),
         "announcement_only_cells": int((never & (r["dur"] > 0) & (r["qlen"] > 0) & (r["tx"] == 1) & (r["pop"] == 0)).sum()),
         "senders_delivering": sorted(i for i, (_, d) in by_sender.items() if d > 0),
         "partly_chosen": int(np.isin(dev, partly_decoded(D)).sum()), "flags": res["flags"]}
    if kind in EPISODIC:
        m["episodes"] = np.atleast_2d(res["cmp"]["tally"])[:, 0].tolist()
    return m


def gated(kind, D, res, who):
    m = measure(kind, D, res)
    for i in partly_decoded(D):
        pop, dlv = m["by_sender"][i]
        if pop and not 0 < dlv < pop:
            raise RuntimeError("%s: the partly decoded sender %d popped %d and delivered %d" % (who, i, pop, dlv))
    if not any(m["by_sender"][i][0] for i in partly_decoded(D)):
        raise RuntimeError("%s: no partly decoded sender popped a packet" % who)
    if any(m["by_sender"][i][0] for i in never_granted(D)):
        raise RuntimeError("%s: a never-granted sender popped packets: %s" % (who, m["by_sender"]))
    if m["partly_cells"] < MIN_CELLS:
        raise RuntimeError("%s: %d cells with 0 < delivered < popped, fewer than %d" % (who, m["partly_cells"], MIN_CELLS))
    if m["announcement_only_cells"] < MIN_CELLS:
        raise RuntimeError("%s: %d announcement-only cells, fewer than %d" % (who, m["announcement_only_cells"], MIN_CELLS))
    if len(m["senders_delivering"]) < 2:
        raise RuntimeError("%s: only senders %s deliver" % (who, m["senders_delivering"]))
    if kind in EPISODIC and min(m["episodes"]) < MIN_EPISODES:
        raise RuntimeError("%s: %s episodes ended, fewer than %d somewhere" % (who, m["episodes"], MIN_EPISODES))
    if kind in ("backlog", "backlog_pop") and m["partly_chosen"] < MIN_CELLS:
        raise RuntimeError("%s: the partly decoded sender is chosen %d times, fewer than %d" % (who, m["partly_chosen"], MIN_CELLS))
    return m


def controller_bits(kind, res):
    """The cells (no episode ended there) in which delivered_k >= need[node] and popped_k >= need[node] differ."""
    r = res["rec"]
    if kind == "fsc":
        at, ended = res["cmp"]["node"].astype(np.int64), res["cmp"]["ended"]
        need = np.asarray(res["controller"][2]).astype(np.int64)[at]
    else:                                                   # (the population call records no rows: the slices' compositions do)
        at, ended = res["rows"]["node"].astype(np.int64), res["rows"]["ended"]
        need = np.stack([np.asarray(c[2]) for c in res["controllers"]]).astype(np.int64)[np.arange(N)[None, :] // M, at]
    return int((((r["dlv"] >= need) != (r["pop"] >= need)) & (ended == 0)).sum())


def freeze(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, (tuple, list)):
        for y in x:
            freeze(y)


@functools.lru_cache(maxsize=None)
def reference(kind, D):
    """The lossy case of run kind ``kind`` at D senders: built once, gated, checked for sensitivity, read only from then on."""
    who = "reference(%r, %d)" % (kind, D)
    res = run(kind, D)
    res["measured"] = m = gated(kind, D, res, who)
    swapped = run(kind, D, swap=True)["cmp"]
    changed = sorted(k for k, v in res["cmp"].items() if not np.array_equal(v, swapped[k]))
    res["changed"] = {fam: [k for k in SENSITIVE[fam] if k in changed] for fam in FAMILIES[kind]}
    for fam, keys in res["changed"].items():
        if not keys:
            raise RuntimeError("%s: popped for delivered changes none of %s, which is what %s is compared in" % (who, SENSITIVE[fam], fam))
    if kind in ("fsc", "fsc_pop"):
        m["bit_cells"] = controller_bits(kind, res)
        if m["bit_cells"] < MIN_CELLS:
            raise RuntimeError("%s: the delivered bit differs from the popped bit in %d cells, fewer than %d"
                               % (who, m["bit_cells"], MIN_CELLS))
    for k in ("dev", "dur", "obs_prev", "now0", "score", "policy", "population", "controller", "controllers"):      # the inputs
        freeze(res.get(k))
    freeze(list(res["cmp"].values()))
    return res


@functools.lru_cache(maxsize=None)
def limit_reference(kind):
    """The fast forms' limit on simulated time crossed inside one launch: the default layout at D = 4 started at NEAR_LIMIT,
    LIMIT_STEPS steps of gw_rollout ("sync") or of the scored episodic call ("scored")."""
    who = "limit_reference(%r)" % kind
    res = run(kind, 4, layout="default", start_time=NEAR_LIMIT, steps=LIMIT_STEPS)
    now = res["rec"]["now"]
    if not (res["now0"] < LIMIT).all():
        raise RuntimeError("%s: a clock is past the limit before the call" % who)
    below = int((now[3] < LIMIT).sum())
    if 4 * below < N:
        raise RuntimeError("%s: %d of %d envs below the limit after step 4, fewer than a quarter" % (who, below, N))
    if not (now[-1] > LIMIT).all():
        raise RuntimeError("%s: %d envs have not crossed the limit at the end" % (who, int((now[-1] <= LIMIT).sum())))
    res["measured"] = {"below_after_step_4": below, "flags": res["flags"]}
    freeze(list(res["cmp"].values()))
    return res


CASES = [(kind, 4) for kind in FAMILIES] + [(kind, 9) for kind in ("sync", "scored", "backlog", "fsc")]


# ---- the gates ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,D", CASES)
def test_reference_passes_its_gates_and_would_catch_popped_for_delivered(kind, D):
    res = reference(kind, D)
    m = res["measured"]
    print("%s D=%d: popped/delivered by sender %s; partly cells %d; announcement-only cells %d; episodes %s; bit cells %s; flags %d; "
          "popped for delivered changes %s" % (kind, D, m["by_sender"], m["partly_cells"], m["announcement_only_cells"],
                                               m.get("episodes"), m.get("bit_cells"), m["flags"], res["changed"]))
    assert all(res["changed"].values()) and set(res["changed"]) == set(FAMILIES[kind])
    assert not m["flags"] & FLAGS_FATAL                      # (the GPU test then holds env.check() to the same)
    assert reference(kind, D) is res and not res["cmp"]["n_delivered"].flags.writeable


@pytest.mark.parametrize("kind", ["sync", "scored"])
def test_limit_reference_crosses_the_limit_inside_the_launch(kind):
    res = limit_reference(kind)
    print(kind, res["measured"])
    assert 4 * res["measured"]["below_after_step_4"] >= N and not res["measured"]["flags"] & FLAGS_FATAL


def test_the_backlog_policies_weigh_the_never_granted_senders_both_ways():
    D = 4
    pop = case_backlog_population(D)
    w = np.stack([np.frombuffer(row.tobytes(), "<i4", actions.MAX_DEVICES)[:D] for row in pop])
    never = never_granted(D)
    assert never == [2, 3] and partly_decoded(D) == [1]
    assert (w[0, never] == 0).all() and (w[1:, never] > 0).all() and (np.delete(w, never, axis=1) > 0).all()
    assert (np.frombuffer(case_backlog_policy(D).tobytes(), "<i4", actions.MAX_DEVICES)[never] > 0).all()


def test_the_substitute_counts_what_the_step_popped():
    """Tap(swap=True) changes what the compositions read, not the trajectory of a staged run."""
    a, b = run("auto_scored", 4), run("auto_scored", 4, swap=True)
    for k in ("obs", "done"):
        assert (a["cmp"][k] == b["cmp"][k]).all()
    assert (a["cmp"]["delivered"] == a["rec"]["dlv"]).all() and (b["cmp"]["delivered"] == a["rec"]["pop"]).all()
    assert (a["rec"]["pop"] >= a["rec"]["dlv"]).all() and (a["rec"]["pop"] > a["rec"]["dlv"]).any()


# ---- the layout keeps the fused forms ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3, 4, 5, 8, 9, 16])
def test_the_layout_keeps_the_fused_forms_available(native_lib, D):
    from gymwipe_amd import _native as nat
    cfg = nat.default_config(N, D)
    pos, rrm = lossy_layout(D)
    for i, (x, y) in enumerate(pos):
        cfg.pos[i][0], cfg.pos[i][1] = x, y
    cfg.pos[D][0], cfg.pos[D][1] = rrm
    mx = C.c_int32()
    assert native_lib.gw_selftest_fastmath(C.byref(cfg), C.byref(mx)) == 31
    assert 1 <= mx.value <= nat.MAX_NSTATES, mx.value
