#!/usr/bin/env python3
"""
Which band schedule keeps the pendulum quiet?  A random search over cyclic schedules of the closed control loop, every
candidate averaged over envs that start from different angles -- one launch per generation, no [steps][N] array
(env.rollout_schedules), the reduction per schedule one torch sum.

    python examples/control_schedule_search.py [--schedules 64] [--envs-per-schedule 64] [--length 8] [--generations 6]

Cost of an episode: the sum of |angle in degrees| over its steps.  With the shipped gain (kp = 1 on degrees) the more the
controller talks the harder it drives the plant, so "nobody assigned" and "sensor only" are printed beside the best schedule.
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
    args = ap.parse_args()

    import torch
    from gymwipe_amd import VecControlLoopEnv, actions

    P, M, L = args.schedules, args.envs_per_schedule, args.length
    N = P * M
    rng = np.random.default_rng(args.seed)
    env = VecControlLoopEnv(N)
    x0 = np.zeros((M, 4))
    x0[:, 2] = rng.uniform(-args.angle, args.angle, M)
    env.set_initial_state(torch.from_numpy(np.tile(x0, (P, 1))))        # every schedule meets the same M initial states
    episodes = (args.episode_steps, 0.0)                                # a time limit, no failure angle
    steps = args.episode_steps * args.episodes

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


if __name__ == "__main__":
    main()
