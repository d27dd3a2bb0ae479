#!/usr/bin/env python3
"""
Policy search for what a band-assignment scheduler exists for: delivered packets.

The built-in reward is lastAbs - abs of received[0] - received[1]; over an episode it telescopes to -|final difference|, so an
episode's return is 0 or -payload_value whatever the policy does -- and the policy that never lets anyone transmit attains the
maximum.  env.rollout_population(score=...) ranks the candidates by a score of the caller's instead: here one point per data
packet of the assigned sender that the RRM decoded (actions.make_score(D, reward=0, delivered=1)).

    python examples/throughput_search.py [--envs 65536] [--policies 256] [--generations 10] [--baseline]
                                          [--tune-baseline [--counter-interval 0.03] [--tune-policies 64] [--tune-generations 8]]
                                          [--controller [--controller-policies 64] [--controller-generations 8]]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--devices", type=int, default=4)
    ap.add_argument("--policies", type=int, default=256, help="P; envs / P a multiple of 64 takes the fused form")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--episode-steps", type=int, default=8)
    ap.add_argument("--generations", type=int, default=10)
    ap.add_argument("--baseline", action="store_true", help="also run the queue-aware backlog scheduler (env.rollout_backlog)")
    ap.add_argument("--tune-baseline", action="store_true",
                    help="tune the scheduler's policy for this configuration first (BacklogSearchAgent) and use the tuned policy as the baseline")
    ap.add_argument("--counter-interval", type=float, default=None, help="the senders' counter_interval (default: the reference's 1 ms)")
    ap.add_argument("--tune-policies", type=int, default=64)
    ap.add_argument("--tune-generations", type=int, default=8)
    ap.add_argument("--controller", action="store_true",
                    help="also search finite-state controllers (ControllerSearchAgent): memory and a delivered bit, no queue lengths")
    ap.add_argument("--controller-policies", type=int, default=64)
    ap.add_argument("--controller-generations", type=int, default=8)
    args = ap.parse_args()

    from gymwipe_amd import VecCounterTrafficEnv, actions
    from gymwipe_amd.agents import BacklogSearchAgent, ControllerSearchAgent, PopulationSearchAgent

    env = VecCounterTrafficEnv(args.envs, num_devices=args.devices, counter_interval=args.counter_interval)
    D, md = args.devices, int(env.config.max_duration)
    packets = actions.make_score(D, reward=0, delivered=1)

    # 1. what return-ranking prefers: the idle policy (always sender 0 for duration 0, which assigns nothing) against a busy one
    def always(sender, duration):
        p = np.zeros((3, D * md))
        p[:, sender * md + duration] = 1.0
        return p
    P = args.policies
    pair = actions.policy_cdf(np.stack([always(0, 0), always(0, md - 1)] * (P // 2)))
    for name, score in (("return", None), ("packets", packets)):
        env.reset()
        env.episode_state.zero_()
        stats = env.population_stats(env.rollout_population(pair, args.steps, seed=1, max_steps=args.episode_steps, score=score))
        print("ranked by %-7s  idle policy %7.3f per episode, busy policy %7.3f" %
              (name, float(stats["mean_return"][0]), float(stats["mean_return"][1])))

    # 2. cross-entropy search ranked by delivered packets: each generation is one rollout_population call
    agent = PopulationSearchAgent(env, P, args.steps, args.episode_steps, seed=0, score=packets)
    e = {"best": float("nan")}
    for _ in range(args.generations):
        e = agent.step()
        print("generation %2d  mean packets per episode %.3f  best %.3f" % (e["generation"], e["mean"], e["best"]))

    # 3. the yardstick: a scheduler that sees the queues (the longest queue, for as long as its backlog needs), on the same
    #    handle -- what the three-valued observation leaves undelivered.  Its default table is a guess; --tune-baseline searches
    #    weights and table for this configuration, every generation one rollout_backlog_population call from the same state.
    policy = None
    if args.tune_baseline:
        tuner = BacklogSearchAgent(env, args.tune_policies, args.steps, args.episode_steps, seed=0, score=packets)
        for _ in range(args.tune_generations):
            t = tuner.step()
            print("tuning generation %2d  packets per episode: the mean policy %.3f  best %.3f" % (t["generation"], t["of_mu"], t["best"]))
        policy = tuner.policy()
        both = actions.make_backlog_population([actions.make_backlog_policy(D, max_duration=md), policy] * (args.tune_policies // 2))
        tally = tuner.evaluate(both, 0).cpu().numpy()
        print("scheduler's default policy %.3f packets per episode, tuned %.3f"
              % (tally[0::2, 3].sum() / tally[0::2, 0].sum(), tally[1::2, 3].sum() / tally[1::2, 0].sum()))
    if args.baseline or args.tune_baseline:
        env.reset()
        env.episode_state.zero_()
        out = env.rollout_backlog(args.steps, policy, max_steps=args.episode_steps, score=packets)
        per_step = float(out[4].sum()) / (args.steps * args.envs)
        print("backlog scheduler%s %.4f packets per env-step; the search's best policy %.4f"
              % (" (tuned)" if policy is not None else "      ", per_step, e["best"] / args.episode_steps))
    # 4. between the two: a finite-state controller knows what it did and whether the step it granted delivered enough, which a
    #    real RRM knows too.  The search starts at stay-while-productive; every generation is one rollout_controller_population
    #    call from the same state.
    if args.controller:
        search = ControllerSearchAgent(env, args.controller_policies, args.steps, args.episode_steps, seed=0, score=packets)
        for _ in range(args.controller_generations):
            c = search.step()
            print("controller generation %2d  packets per episode: the mean controller %.3f  best %.3f"
                  % (c["generation"], c["of_mu"], c["best"]))
        rr = actions.round_robin_controller(D, md - 1, md)
        both = actions.make_controller_population([rr, search.controller()] * (args.controller_policies // 2))
        tally = search.evaluate(both, 0).cpu().numpy()
        print("round-robin %.4f packets per env-step, the searched controller %.4f"
              % (tally[0::2, 3].sum() / tally[0::2, 2].sum(), tally[1::2, 3].sum() / tally[1::2, 2].sum()))
    env.check()


if __name__ == "__main__":
    main()
