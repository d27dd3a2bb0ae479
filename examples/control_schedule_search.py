#!/usr/bin/env python3
"""
Which band schedule keeps the pendulum quiet?  A random search over cyclic schedules of the closed control loop, every
candidate averaged over envs that start from different angles -- one launch per generation, no [steps][N] array
(env.rollout_schedules), the reduction per schedule one torch sum.

    python examples/control_schedule_search.py [--schedules 64] [--envs-per-schedule 64] [--length 8] [--generations 6]

Cost of an episode: the sum of |angle in degrees| over its steps.  With the default gains (the reference's shipped kp = 1 on
degrees) the more the controller talks the harder it drives the plant, so "nobody assigned" and "sensor only" are printed
beside the best schedule; --gains, below, searches the controller as well.

    python examples/control_schedule_search.py --feedback [--bins 3] [--airtime-price 0.002]

searches angle-feedback schedulers instead (env.rollout_feedback): a policy is B - 1 thresholds on |observed angle| and one
cyclic schedule per bin, so "leave the band alone while the pendulum is near upright" is a candidate.  The per-step sum above
favours whoever takes short steps, so this search ranks by the time-weighted mean |angle| (area / elapsed, degrees) plus
--airtime-price times the duration units assigned per second of simulated time, and prints the best open-loop schedule -- the
same search with one bin -- under the same ranking beside the result.

    python examples/control_schedule_search.py --gains [--envs-per-pair 8]

ranks controllers and schedulers together: G sets of PID gains (env.set_gains, laid across the envs of every schedule by
actions.make_ctrl_gains) times the P schedules named below, all G x P pairs in ONE env.rollout_schedules launch, and again in
one env.rollout_feedback launch with every schedule turned into "idle while |angle| < 2 degrees, else the schedule".  The
tally is reduced to a [G][P] table here; printed are the table, the best gains per schedule, and the shipped gains' row.

    python examples/control_schedule_search.py --disturbance 0.01 [--envs-per-pair 8] [--disturbance-steps 120]

ranks the same G x P grid twice by the time-weighted mean |angle|, every env starting upright: on the exact plant, where all
there is to regulate is the transient of the first command, and with seeded noise of weight A on the pendulum's angular rate at
every plant substep (env.set_disturbance), something to hold the pendulum against.  Env j of every cell gets noise stream j
(actions.make_ctrl_disturbance(streams=arange(N) % envs_per_pair)): all cells face the same m noise sequences, so two cells'
difference is a paired one.  Printed are both rankings side by side and, for the two best disturbed cells, in how many of the
m sequences the better one wins.

    python examples/control_schedule_search.py --loss 0.5 [--loss-links 1,1,1,1] [--disturbance 0.01] [--envs-per-pair 8]

ranks the grid twice on the disturbed plant (weight --disturbance, default 0.01): on the PHY's own links, which drop nothing at
this geometry, and with every transmission erased with probability P times its link's entry of --loss-links (announcement to the
sensor, to the controller, sensor's data, controller's data; env.set_loss).  Env j of every cell gets noise stream j and loss
stream j (actions.make_ctrl_loss(streams=arange(N) % envs_per_pair)): all cells lose the same transmissions, counted in the
order they go on the air.  Printed are both rankings side by side, how the ranking moves, and the erasures per link.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--schedules", type=int, default=64, help="P")
    ap.add_argument("--envs-per-schedule", type=int, default=64, help="a multiple of 64")
    ap.add_argument("--length", type=int, default=8, help="L: entries of a schedule")
    ap.add_argument("--episode-steps", type=int, default=40)
    ap.add_argument("--episodes", type=int, default=2, help="episodes per env and generation")
    ap.add_argument("--angle", type=float, default=0.3, help="initial angles are drawn from [-angle, angle] rad")
    ap.add_argument("--generations", type=int, default=6)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--feedback", action="store_true", help="search angle-feedback schedulers (thresholds and per-bin schedules)")
    ap.add_argument("--bins", type=int, default=3, help="B of --feedback, 1 .. 8")
    ap.add_argument("--airtime-price", type=float, default=0.002, help="degrees per duration unit assigned per simulated second")
    ap.add_argument("--gains", action="store_true", help="rank a grid of PID gain sets x schedules in one launch")
    ap.add_argument("--envs-per-pair", type=int, default=8, help="initial angles per (gain set, schedule) pair of --gains")
    ap.add_argument("--disturbance", type=float, default=None, metavar="A",
                    help="rank the gain x schedule grid with and without plant noise of weight A on x[3], common random numbers")
    ap.add_argument("--loss", type=float, default=None, metavar="P",
                    help="rank the gain x schedule grid on the disturbed plant with and without packet loss P, common random numbers")
    ap.add_argument("--loss-links", default="1,1,1,1", help="a,b,c,d: P is multiplied by these per link "
                    "(announcement to sensor, to controller, sensor -> controller, controller -> actuator)")
    ap.add_argument("--disturbance-steps", type=int, default=120, help="steps per env of --disturbance")
    args = ap.parse_args()

    import torch
    from gymwipe_amd import VecControlLoopEnv, actions

    if args.loss is not None:
        loss_grid(args, torch, VecControlLoopEnv, actions)
        return
    if args.disturbance is not None:
        disturbance_grid(args, torch, VecControlLoopEnv, actions)
        return
    if args.gains:
        gains_grid(args, torch, VecControlLoopEnv, actions)
        return

    P, M, L = args.schedules, args.envs_per_schedule, args.length
    N = P * M
    rng = np.random.default_rng(args.seed)
    env = VecControlLoopEnv(N)
    x0 = np.zeros((M, 4))
    x0[:, 2] = rng.uniform(-args.angle, args.angle, M)
    env.set_initial_state(torch.from_numpy(np.tile(x0, (P, 1))))        # every schedule meets the same M initial states
    episodes = (args.episode_steps, 0.0)                                # a time limit, no failure angle
    steps = args.episode_steps * args.episodes

    if args.feedback:
        feedback_search(args, env, actions, rng, episodes, steps)
        env.close()
        return

    def evaluate(candidates):
        """Mean episode cost of each schedule: every env restarts, runs whole episodes, and the tally is summed per schedule."""
        env.reset_envs()
        _, sums = env.rollout_schedules(actions.make_ctrl_schedules(candidates, L), episodes, steps)
        sums = sums.cpu().numpy()
        assert (sums[:, 0] == M * args.episodes).all()
        cost = sums[:, 3] / sums[:, 0]
        return np.where(np.isfinite(cost), cost, np.inf)                # a schedule that drives the plant out of range loses

    def random_schedule():
        return list(zip(rng.integers(0, 2, L).tolist(), rng.integers(0, 20, L).tolist()))

    def mutated(s):
        s = list(s)
        j = int(rng.integers(0, L))
        s[j] = (int(rng.integers(0, 2)), int(rng.integers(0, 20)))
        return s

    idle, sensor_only = [(0, 0)] * L, [(0, 19)] * L
    best, best_cost = None, np.inf
    for g in range(args.generations):
        keep = [idle, sensor_only] + ([best] if best is not None else [])
        fresh = [mutated(best) if best is not None and i % 2 else random_schedule() for i in range(P - len(keep))]
        candidates = keep + fresh
        cost = evaluate(candidates)
        i = int(cost.argmin())
        if cost[i] < best_cost:
            best, best_cost = candidates[i], float(cost[i])
        print("generation %d: nobody assigned %.1f, sensor only %.1f, best of %d schedules %.1f (median %.3g)"
              % (g, cost[0], cost[1], P, cost[i], float(np.median(cost))))
    print("best schedule (device, duration) x %d: %s" % (L, best))
    print("mean cost per episode of %d steps over %d initial angles: best %.1f | nobody assigned %.1f | sensor only %.1f"
          % (args.episode_steps, M, best_cost, cost[0], cost[1]))
    env.close()


def feedback_search(args, env, actions, rng, episodes, steps):
    """Random search over (thresholds, one schedule per bin), and over open-loop schedules as policies of one bin, both ranked
    by area / elapsed + price * airtime / elapsed from the tally of one launch per generation and kind."""
    P, L, B = args.schedules, args.length, args.bins

    def evaluate(candidates):
        env.reset_envs()
        sched, edges = actions.make_ctrl_feedback([c[1] for c in candidates], [c[0] for c in candidates], L)
        _, sums = env.rollout_feedback(sched, edges, episodes, steps, abs_key=True)
        sums = sums.cpu().numpy()
        error, airtime = sums[:, 6] / sums[:, 5], sums[:, 4] / sums[:, 5]
        score = error + args.airtime_price * airtime
        return np.where(np.isfinite(score), score, np.inf), error, airtime

    def random_schedule():
        return list(zip(rng.integers(0, 2, L).tolist(), rng.integers(0, 20, L).tolist()))

    def random_policy(bins):
        return sorted(rng.integers(1, 60, bins - 1).tolist()), [random_schedule() for _ in range(bins)]

    def mutated(policy):
        edges, scheds = list(policy[0]), [list(s) for s in policy[1]]
        if edges and rng.integers(0, 3) == 0:                           # move a threshold ...
            j = int(rng.integers(0, len(edges)))
            edges[j] = int(np.clip(edges[j] + rng.integers(-5, 6), 1, 89))
        else:                                                           # ... or rewrite one entry of one bin's schedule
            scheds[int(rng.integers(0, len(scheds)))][int(rng.integers(0, L))] = (int(rng.integers(0, 2)), int(rng.integers(0, 20)))
        return edges, scheds

    best = {}
    for g in range(args.generations):
        for kind, bins in (("feedback", B), ("open loop", 1)):
            have = best.get(kind)
            keep = [have[0]] if have else []
            if kind == "feedback" and B > 1 and not have:               # idle near upright, alternate beyond: the README's policy
                keep = [([2] + [89] * (B - 2), [[(0, 0)] * L] + [[(0, 19), (1, 19)] * (L // 2) + [(0, 19)] * (L % 2)] * (B - 1))]
            candidates = keep + [mutated(have[0]) if have and i % 2 else random_policy(bins) for i in range(P - len(keep))]
            score, error, airtime = evaluate(candidates)
            i = int(score.argmin())
            if not have or score[i] < have[1]:
                best[kind] = (candidates[i], float(score[i]), float(error[i]), float(airtime[i]))
            print("generation %d, %-9s: best of %d score %.3f (error %.3f deg, airtime %.1f units/s), median score %.3g"
                  % (g, kind, P, score[i], error[i], airtime[i], float(np.median(score))))
    for kind in ("feedback", "open loop"):
        (edges, scheds), score, error, airtime = best[kind]
        print("best %s: score %.3f = %.3f deg time-weighted mean |angle| + %g x %.1f duration units per second"
              % (kind, score, error, args.airtime_price, airtime))
        if edges:
            print("  thresholds on |observed angle|: %s" % edges)
        for b, sch in enumerate(scheds):
            print("  bin %d (device, duration) x %d: %s" % (b, L, sch))


GAIN_SETS = [(1.0, 0.0, 0.0), (0.5, 0.0, 0.0), (0.2, 0.0, 0.0), (0.1, 0.0, 0.0), (0.05, 0.0, 0.0), (0.02, 0.0, 0.0),
             (0.05, 0.01, 0.0), (0.1, 0.0, 0.2)]                       # (kp, ki, kd); the first is the shipped set
SCHEDULES = [("alternate 19/19", [(0, 19), (1, 19)]), ("19/5", [(0, 19), (1, 5)]), ("8/8", [(0, 8), (1, 8)]),
             ("3/3", [(0, 3), (1, 3)]), ("19/19/5", [(0, 19), (0, 19), (1, 5)]), ("12/2", [(0, 12), (1, 2)]),
             ("sensor only", [(0, 19)]), ("nobody", [(0, 0)])]


def gains_grid(args, torch, VecControlLoopEnv, actions):
    """G gain sets x P schedules, m initial angles per pair: env e runs schedule e // (G m) under gain set (e // m) % G."""
    G, P, m = len(GAIN_SETS), len(SCHEDULES), args.envs_per_pair
    if (G * m) % 64:
        sys.exit("--envs-per-pair times %d gain sets must be a multiple of 64 (one schedule per 64-env block)" % G)
    N = P * G * m
    rng = np.random.default_rng(args.seed)
    x0 = np.zeros((m, 4))
    x0[:, 2] = rng.uniform(-args.angle, args.angle, m)
    env = VecControlLoopEnv(N, gains=actions.make_ctrl_gains(GAIN_SETS, N, envs_per_set=m))
    env.set_initial_state(torch.from_numpy(np.tile(x0, (P * G, 1))))    # every pair meets the same m initial states
    episodes = (args.episode_steps, 0.0)
    steps = args.episode_steps * args.episodes
    names = [n for n, _ in SCHEDULES]
    scheds = [s for _, s in SCHEDULES]

    def table(title, unit, cell):
        """``cell`` [P][G] -> the [G][P] table, the best gains per schedule, the shipped gains' row."""
        t = np.where(np.isfinite(cell), cell, np.inf).T
        print("%s (%s); rows: gain sets, columns: schedules" % (title, unit))
        print("%-20s" % "(kp, ki, kd)" + "".join("%16s" % n for n in names))
        for g in range(G):
            print("%-20s" % (GAIN_SETS[g],) + "".join("%16.4g" % v for v in t[g]))
        for p in range(P):
            g = int(t[:, p].argmin())
            print("  %-16s best gains %-18s %10.4g | shipped gains %10.4g" % (names[p], GAIN_SETS[g], t[g, p], t[0, p]))
        g, p = np.unravel_index(int(t.argmin()), t.shape)
        print("  best pair: gains %s with schedule '%s': %.4g; the shipped gains' best: %.4g ('%s')"
              % (GAIN_SETS[g], names[p], t[g, p], t[0].min(), names[int(t[0].argmin())]))

    env.reset_envs()
    tally, _ = env.rollout_schedules(actions.make_ctrl_schedules(scheds), episodes, steps)
    cell = tally.view(P, G, m, 4).sum(2).cpu().numpy()                  # the caller's reduction: per (schedule, gain set)
    assert (cell[..., 0] == m * args.episodes).all()
    table("open-loop schedules: mean episode cost", "sum of |angle in degrees| over %d steps" % args.episode_steps,
          cell[..., 3] / cell[..., 0])

    env.reset_envs()                                                    # the same pairs, the schedule only while |angle| >= 2 degrees
    sched, edges = actions.make_ctrl_feedback([[[(0, 0)], s] for s in scheds], [[2]] * P)
    tally, _ = env.rollout_feedback(sched, edges, episodes, steps, abs_key=True)
    cell = tally.view(P, G, m, tally.shape[1]).sum(2).cpu().numpy()
    table("\nfeedback: idle below 2 degrees, else the schedule", "time-weighted mean |angle| in degrees", cell[..., 6] / cell[..., 5])
    env.close()


def disturbance_grid(args, torch, VecControlLoopEnv, actions):
    """gains_grid's layout, every env from x0 = 0: the time-weighted mean |angle| of every (gain set, schedule) cell on the exact
    plant and under noise, m noise streams shared by all cells."""
    closing = [(n, s) for n, s in SCHEDULES if any(d == 1 and u > 0 for d, u in s)]     # the schedules that let the controller talk:
    G, P, m = len(GAIN_SETS), len(closing), args.envs_per_pair          # without it there is no loop to rank
    if (G * m) % 64:
        sys.exit("--envs-per-pair times %d gain sets must be a multiple of 64 (one schedule per 64-env block)" % G)
    N = P * G * m
    episodes = (0, 0.0)                                                 # no episode ends: one long run per env
    steps = args.disturbance_steps
    names = [n for n, _ in closing]
    sched, edges = actions.make_ctrl_feedback([[s] for _, s in closing], [[]] * P)      # one bin: the open-loop schedules
    weights, key = actions.make_ctrl_disturbance((0.0, 0.0, 0.0, args.disturbance), N, seed=args.seed, streams=np.arange(N) % m)

    def run(disturbed):
        env = VecControlLoopEnv(N, x0=(0.0, 0.0, 0.0, 0.0), gains=actions.make_ctrl_gains(GAIN_SETS, N, envs_per_set=m))
        if disturbed:
            env.set_disturbance(weights, key)
        tally, _ = env.rollout_feedback(sched, edges, episodes, steps, abs_key=True)
        t = tally.view(P, G, m, tally.shape[1]).cpu().numpy()
        env.close()
        err = t[..., 6] / t[..., 5]                                     # [P][G][m]: per env, area / elapsed
        return np.where(np.isfinite(err), err, np.inf)

    calm, noisy = run(False), run(True)
    assert (calm == calm[..., :1]).all()                                # on the exact plant the m envs of a cell are copies
    c, n = calm[..., 0], noisy.mean(2)
    order_c, order_n = np.argsort(c, axis=None), np.argsort(n, axis=None)
    rank_c, rank_n = np.empty(P * G, int), np.empty(P * G, int)
    rank_c[order_c], rank_n[order_n] = np.arange(P * G), np.arange(P * G)

    def cell(i):
        p, g = np.unravel_index(i, c.shape)
        return "%-16s %-18s" % (names[p], GAIN_SETS[g])
    print("time-weighted mean |angle| in degrees over %d steps from upright; noise weight %g on the angular rate, %d streams shared by all %d cells"
          % (steps, args.disturbance, m, P * G))
    print("%4s  %-35s %10s %10s %6s   |  %-35s %10s %10s %6s" % ("rank", "exact plant: schedule, gains", "exact", "disturbed", "there",
                                                               "disturbed: schedule, gains", "disturbed", "spread", "exact"))
    for r in range(min(10, P * G)):
        i, j = order_c[r], order_n[r]
        print("%4d  %s %10.4g %10.4g %6d   |  %s %10.4g %10.4g %6d"
              % (r + 1, cell(i), c.flat[i], n.flat[i], rank_n[i] + 1, cell(j), n.flat[j],
                 noisy.reshape(P * G, m)[j].max() - noisy.reshape(P * G, m)[j].min(), rank_c[j] + 1))
    a, b = noisy.reshape(P * G, m)[order_n[0]], noisy.reshape(P * G, m)[order_n[1]]
    print("the best disturbed cell against the second: means %.4g and %.4g, spread over streams %.4g and %.4g; paired on the same"
          " stream it wins in %d of %d" % (a.mean(), b.mean(), a.max() - a.min(), b.max() - b.min(), int((a < b).sum()), m))
    print("the exact plant's winner is rank %d of %d under disturbance; the disturbed winner is rank %d on the exact plant"
          % (rank_n[order_c[0]] + 1, P * G, rank_c[order_n[0]] + 1))


def loss_grid(args, torch, VecControlLoopEnv, actions):
    """disturbance_grid's layout and disturbed plant: the time-weighted mean |angle| of every (gain set, schedule) cell without
    and with packet loss, m noise streams and m loss streams shared by all cells."""
    closing = [(n, s) for n, s in SCHEDULES if any(d == 1 and u > 0 for d, u in s)]
    G, P, m = len(GAIN_SETS), len(closing), args.envs_per_pair
    if (G * m) % 64:
        sys.exit("--envs-per-pair times %d gain sets must be a multiple of 64 (one schedule per 64-env block)" % G)
    links = [float(v) for v in args.loss_links.split(",")]
    if len(links) != 4:
        sys.exit("--loss-links takes four factors a,b,c,d")
    N = P * G * m
    steps = args.disturbance_steps
    names = [n for n, _ in closing]
    sched, edges = actions.make_ctrl_feedback([[s] for _, s in closing], [[]] * P)
    a = 0.01 if args.disturbance is None else args.disturbance
    streams = np.arange(N) % m
    weights, nkey = actions.make_ctrl_disturbance((0.0, 0.0, 0.0, a), N, seed=args.seed, streams=streams)
    p_link = [args.loss * f for f in links]
    _, lkey = actions.make_ctrl_loss(p_link, N, seed=args.seed + 1, streams=streams)

    def run(lossy):
        env = VecControlLoopEnv(N, x0=(0.0, 0.0, 0.0, 0.0), gains=actions.make_ctrl_gains(GAIN_SETS, N, envs_per_set=m))
        env.set_disturbance(weights, nkey)
        if lossy:
            env.set_loss(p_link, lkey)
        tally, _ = env.rollout_feedback(sched, edges, (0, 0.0), steps, abs_key=True)
        t = tally.view(P, G, m, tally.shape[1]).cpu().numpy()
        lost, sent = env.get_state("lost").sum(0), int(env.get_state("loss_count").sum())
        env.close()
        err = t[..., 6] / t[..., 5]
        return np.where(np.isfinite(err), err, np.inf), lost, sent

    (clean, _, _), (lossy, lost, sent) = run(False), run(True)
    c, n = clean.mean(2), lossy.mean(2)
    order_c, order_n = np.argsort(c, axis=None), np.argsort(n, axis=None)
    rank_c, rank_n = np.empty(P * G, int), np.empty(P * G, int)
    rank_c[order_c], rank_n[order_n] = np.arange(P * G), np.arange(P * G)

    def cell(i):
        p, g = np.unravel_index(i, c.shape)
        return "%-16s %-18s" % (names[p], GAIN_SETS[g])
    print("time-weighted mean |angle| in degrees over %d steps from upright, noise weight %g; loss probability per link %s;"
          " %d noise and loss streams shared by all %d cells" % (steps, a, ["%g" % v for v in np.clip(p_link, 0, 1)], m, P * G))
    print("%4s  %-35s %10s %10s %6s   |  %-35s %10s %10s %6s" % ("rank", "no loss: schedule, gains", "no loss", "lossy", "there",
                                                               "lossy: schedule, gains", "lossy", "spread", "no loss"))
    for r in range(min(10, P * G)):
        i, j = order_c[r], order_n[r]
        print("%4d  %s %10.4g %10.4g %6d   |  %s %10.4g %10.4g %6d"
              % (r + 1, cell(i), c.flat[i], n.flat[i], rank_n[i] + 1, cell(j), n.flat[j],
                 lossy.reshape(P * G, m)[j].max() - lossy.reshape(P * G, m)[j].min(), rank_c[j] + 1))
    moved = np.abs(rank_c - rank_n)
    print("how the ranking moves: the lossless winner is rank %d of %d under loss; the lossy winner is rank %d without loss; %d of %d cells"
          " change rank, by %.1f places on average and %d at most" % (rank_n[order_c[0]] + 1, P * G, rank_c[order_n[0]] + 1,
                                                                       int((moved > 0).sum()), P * G, moved.mean(), moved.max()))
    best = np.array([n[p].min() for p in range(P)])
    print("best cell per schedule under loss: " + ", ".join("%s %.3g (no loss %.3g)" % (names[p], best[p], c[p].min()) for p in range(P)))
    print("erased of %d transmissions, per link: %s" % (sent, ", ".join("%s %d" % (l, v) for l, v in zip(actions.CTRL_LOSS_LINKS, lost))))


if __name__ == "__main__":
    main()
