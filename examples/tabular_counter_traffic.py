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
    args = ap.parse_args()

    import torch
    from gymwipe_amd import VecCounterTrafficEnv
    from gymwipe_amd.agents import TabularCounterTrafficAgent

    env = VecCounterTrafficEnv(args.envs, num_devices=args.devices)
    agent = TabularCounterTrafficAgent(env, gamma=args.gamma, tau=args.tau, episode_steps=args.episode_steps or None)
    env.reset()
    mean, err = agent.evaluate(args.steps)
    print("before: mean reward per step %+.4f +- %.4f" % (mean, err))
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
    print("after:  mean reward per step %+.4f +- %.4f   (pairs visited: %d of %d)"
          % (mean, err, int((agent.table[..., 0] > 0).sum()), 3 * agent.nb_actions))
    if args.episode_steps:
        print("episodes: %(episodes)d ended (%(by_done)d by done), mean length %(mean_length).2f, "
              "mean return %(mean_return)+.3f +- %(return_stderr).3f" % env.episode_stats())
    env.check()


if __name__ == "__main__":
    main()
