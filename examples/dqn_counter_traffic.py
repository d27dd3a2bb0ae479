#!/usr/bin/env python3
"""The reference's agents/dqn_counter_traffic.py, on the vectorised env: a torch DQN whose policy, the env
step and the replay memory all stay on the GPU.  python examples/dqn_counter_traffic.py [num_envs] [steps] [--score-packets]

--score-packets: per-env episodes of 8 steps through env.step_autoreset(score=), the agent rewarded with one point per data
packet the RRM decoded in the step (make_score(D, reward=0, delivered=1)) instead of the built-in reward, whose episode return
is 0 or -payload_value whatever the policy does.  Prints the mean packets per episode early against late in training."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import gymwipe_amd
from gymwipe_amd.actions import make_score
from gymwipe_amd.agents import DqnCounterTrafficAgent

args = [a for a in sys.argv[1:] if not a.startswith("--")]
SCORE_PACKETS = "--score-packets" in sys.argv[1:]
N = int(args[0]) if len(args) > 0 else 4096
STEPS = int(args[1]) if len(args) > 1 else 300
D, EPISODE = 2, 8
env = gymwipe_amd.make("VecCounterTraffic-v0", num_envs=N, num_devices=D)
agent = DqnCounterTrafficAgent(env)
kw = dict(episode_steps=EPISODE, score=make_score(D, reward=0, delivered=1)) if SCORE_PACKETS else {}


def packets_per_episode(steps):
    """fit() for `steps` steps; the mean score -- packets -- of the episodes that ended in them, from the env's tally."""
    env.episode_tally.zero_()
    loss = agent.fit(steps, **kw)
    return loss, env.episode_stats()["mean_return"]


if SCORE_PACKETS:
    _, early = packets_per_episode(4 * EPISODE)  # warm-up: the untrained policy
else:
    agent.fit(20)                                # warm-up
torch.cuda.synchronize()
t0 = time.perf_counter()
loss = agent.fit(STEPS, **kw)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print("%d envs x %d steps with a GPU-resident DQN in the loop: %.3f s -> %.2f M env-steps/s (last loss %.4f)"
      % (N, STEPS, dt, N * STEPS / dt / 1e6, float(loss.detach()) if loss is not None else float("nan")))
if SCORE_PACKETS:
    _, late = packets_per_episode(4 * EPISODE)
    print("mean packets per episode of %d steps: %.3f in the first %d steps, %.3f in %d steps after %d of training"
          % (EPISODE, early, 4 * EPISODE, late, 4 * EPISODE, 4 * EPISODE + STEPS))
env.check()
