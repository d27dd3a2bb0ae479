#!/usr/bin/env python3
"""
A tabular agent on the closed loop's table: collect -> learn, with nothing sized by the number of envs on the caller's side.

The agent of this env sees one of three observation values and picks one of D * 20 flat actions, so its Q function is a
[3][A] table and everything it learns from is ``env.rollout_policy_stats``' tally over (observation class, action).  One
iteration is one launch per 64 steps plus arithmetic on [3][A] tensors.

Episodes run inside the launch (``--episode-steps``, ``env.rollout_episodes_stats``): an env is reset after that many steps,
or when a step returns done, and acts on the reset's observation next.  Without that an env soon sits in its absorbing state
-- both observed senders have delivered, every further reward is 0 -- and ``--episode-steps 0`` goes back to what keeps it
out of there on the caller's side, an ``env.reset()`` before every collect.

    python examples/tabular_counter_traffic.py --envs 65536 --devices 4 --iterations 20
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--devices", type=int, default=4)
    ap.add_argument("--steps", type=int, default=64, help="env steps per collect()")
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--sweeps", type=int, default=8, help="Q-iteration sweeps per learn()")
    ap.add_argument("--gamma", type=float, default=0.9)
    ap.add_argument("--tau", type=float, default=0.5)
    ap.add_argument("--episode-steps", type=int, default=8, help="episode length inside the launch; 0: reset() per iteration instead")
    ap.add_argument("--score-packets", action="store_true",
                    help="learn from the packets a step delivered (the table's eighth column), not from the built-in reward")
    args = ap.parse_args()
    if args.score_packets and not args.episode_steps:
        ap.error("--score-packets counts packets per episode: it needs --episode-steps > 0")

    import torch
    from gymwipe_amd import VecCounterTrafficEnv, actions
    from gymwipe_amd.agents import TabularCounterTrafficAgent

    env = VecCounterTrafficEnv(args.envs, num_devices=args.devices)
    score = actions.make_score(args.devices, reward=0, delivered=1) if args.score_packets else None
    agent = TabularCounterTrafficAgent(env, gamma=args.gamma, tau=args.tau, episode_steps=args.episode_steps or None, score=score)

    def fmt(mean, err):
        return "%+.4f" % mean if err is None else "%+.4f +- %.4f" % (mean, err)

    def packets_per_episode():
        """The current policy from a reset, in whole episodes: the eighth column's sum over the episodes that ended."""
        env.reset()
        env.episode_tally.zero_()
        steps = -(-args.steps // args.episode_steps) * args.episode_steps
        t = env.rollout_episodes_stats(agent.policy_cdf(), steps, agent.seed, max_steps=args.episode_steps, step0=agent.stream_pos,
                                       packets=True)
        agent.stream_pos += steps
        return float(t[..., 7].sum().cpu()) / max(int(env.episode_tally[0].cpu()), 1)

    what = "score" if args.score_packets else "reward"
    if args.score_packets:
        uniform = packets_per_episode()                  # (Q = 0: the Boltzmann policy is uniform)
    env.reset()
    mean, err = agent.evaluate(args.steps)
    print("before: mean %s per step %s" % (what, fmt(mean, err)))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iterations):
        if not args.episode_steps:
            env.reset()
        agent.collect(args.steps)
        agent.learn(args.sweeps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("%d iterations of collect(%d) + learn(%d): %.2f G env-steps/s"
          % (args.iterations, args.steps, args.sweeps, args.iterations * args.steps * args.envs / dt / 1e9))
    env.reset()
    mean, err = agent.evaluate(args.steps)
    print("after:  mean %s per step %s   (pairs visited: %d of %d)"
          % (what, fmt(mean, err), int((agent.table[..., 0] > 0).sum()), 3 * agent.nb_actions))
    if args.score_packets:
        print("packets per episode of %d steps: learned policy %.2f, uniform policy %.2f" % (args.episode_steps, packets_per_episode(), uniform))
    elif args.episode_steps:
        print("episodes: %(episodes)d ended (%(by_done)d by done), mean length %(mean_length).2f, "
              "mean return %(mean_return)+.3f +- %(return_stderr).3f" % env.episode_stats())
    env.check()


if __name__ == "__main__":
    main()
