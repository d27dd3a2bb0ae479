#!/usr/bin/env python3
"""Five-minute tour (needs an MI355X): the reference's scalar env, the vectorised env, a fused rollout, a custom
interpreter, the pendulum env (open and closed loop) and the PHY grid.  `python examples/quickstart.py`"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import gymwipe_amd
from gymwipe_amd import VecInterpreter

# 1. the reference's own usage, unchanged (tests/envs/test_counter_traffic.py:17-34)
env = gymwipe_amd.make("CounterTraffic-v0")
print("scalar env:", env.step({"device": 0, "duration": 3}), env.step({"device": 1, "duration": 12}))

# 2. the same environment 65 536 times on one GPU; actions and results are tensors that never leave it
N = 65536
venv = gymwipe_amd.VecCounterTrafficEnv(N, num_devices=4)
obs = venv.reset()
for _ in range(32):
    action = {"device": torch.randint(0, 4, (N,), dtype=torch.int32, device="cuda"),
              "duration": torch.randint(0, 20, (N,), dtype=torch.int32, device="cuda")}
    obs, reward, done, info = venv.step(action)
print("vectorised:", obs[:4].tolist(), reward[:4].tolist(), venv.stats())

# 2b. preallocated outputs (their device addresses are taken once): what a tight loop, or a multi-GPU gather record, steps into
slot = gymwipe_amd.StepOutputs(torch.empty(N, dtype=torch.int32, device="cuda"), torch.empty(N, dtype=torch.float32, device="cuda"),
                               torch.empty(N, dtype=torch.uint8, device="cuda"),
                               feedback_bytes=torch.empty(N, dtype=torch.uint8, device="cuda"))   # + the one-byte exchange format
obs, reward, done, info = venv.step(action, out=slot)
print("step(out=):", obs is slot.obs, slot.feedback_bytes[:4].tolist())

# 3. pre-staged actions: 64 steps in one persistent launch
dev = torch.randint(0, 4, (64, N), dtype=torch.int32, device="cuda")
dur = torch.randint(0, 20, (64, N), dtype=torch.int32, device="cuda")
o, r, d = venv.rollout(dev, dur)
print("rollout:", tuple(o.shape), float(r.float().mean()))

# 3b. the same with the policy inside the launch: each env draws its action from the observation it just got.  A policy over
#     the last observation is three rows of probabilities (below / at / above COUNTER_BOUND) over the 4 * 20 flat actions.
from gymwipe_amd.actions import policy_cdf
table = policy_cdf(torch.softmax(torch.randn(3, 4 * 20, device="cuda"), dim=-1))
a_dev, a_dur, o, r, d = venv.rollout_policy(table, 64, seed=1)          # acts on the last observation first; step0 += 64 next time
print("rollout_policy:", tuple(a_dev.shape), float(r.float().mean()))

# 3c. ... and for a caller that wants the tally, not the transitions: int64[3][A][7] over (observation class, action) with
#     n, reward sum, reward-square sum, next observation below / at / above the bound, done -- no [steps][N] array at all
stats = venv.rollout_policy_stats(table, 64, seed=1, step0=64)          # continues from the observations 3b ended on
n, r_sum = int(stats[..., 0].sum()), int(stats[..., 1].sum())
print("rollout_policy_stats:", tuple(stats.shape), n, r_sum / n)

# 3d. episodes inside the launch: an env is reset after 8 steps (or when a step returns done) and acts on the reset's
#     observation next -- without this an env soon sits in its absorbing state, where every reward is 0.  `ended` marks the
#     terminal steps (1 done, 2 step limit); the env keeps each env's age and return and tallies the ended episodes.
a_dev, a_dur, o, r, d, ended = venv.rollout_episodes(table, 64, seed=1, max_steps=8, step0=128)
print("rollout_episodes:", int((ended != 0).sum()), "episodes ended,", venv.episode_stats())

# 3e. ... and when you choose the actions yourself: one step with autoreset (a rollout_autoreset of one step; `nxt` is what to act on)
o, r, d, ended, nxt = venv.step_autoreset(action, max_steps=8)
print("step_autoreset:", int((ended != 0).sum()), "episodes ended,", int((nxt != o).sum()), "envs act on the reset's observation")

# 3f. ... scored by what the step delivered instead of the built-in reward: `r` is 1 point per packet of the sender you chose
from gymwipe_amd.actions import make_score
o, r, d, ended, nxt, delivered = venv.step_autoreset(action, max_steps=8, score=make_score(4, reward=0, delivered=1))
print("step_autoreset(score=):", int(delivered.sum()), "packets decoded in the step,", float(r.sum()), "points")

# 4. your own Interpreter (envs/core.py:59-159), fed with what the RRM sniffed each step
class CountDeliveries(VecInterpreter):
    def __init__(self, n):
        self.total = torch.zeros(n, dtype=torch.int64, device="cuda")
        self.last = torch.zeros(n, dtype=torch.int32, device="cuda")

    def onPacketReceived(self, senderIndex, receiverIndex, payload):
        self.last = payload.count
        self.total += payload.count

    def getObservation(self):
        return self.last

    def getReward(self):
        return self.last.float()

    def getDone(self):
        return torch.zeros_like(self.last, dtype=torch.bool)

    def reset(self):
        self.total.zero_()


cenv = gymwipe_amd.VecCounterTrafficEnv(1024, num_devices=2, interpreter=CountDeliveries(1024))
cenv.reset()
for k in range(16):
    fb = cenv.step({"device": torch.full((1024,), k % 2, dtype=torch.int32, device="cuda"),
                    "duration": torch.full((1024,), 10, dtype=torch.int32, device="cuda")})
print("custom interpreter: packets decoded by the RRM per env so far:", int(cenv.interpreter.total[0]))

# 5. the pendulum band-assignment env (builder-defined linear plant on the f64 matrix cores)
penv = gymwipe_amd.make("VecInvertedPendulum-v0", num_envs=4096)
for _ in range(8):
    pobs, prew, pdone, pinfo = penv.step({"device": torch.zeros(4096, dtype=torch.int32, device="cuda"),
                                          "duration": torch.full((4096,), 19, dtype=torch.int32, device="cuda")})
print("pendulum:", int(pobs[0]), float(prew[0]), float(pinfo["Sensor angle"][0]))

# 5b. the same env with its control loop closed over receive-mode MACs (sensor -> controller -> actuator)
loop = gymwipe_amd.make("VecControlLoop-v0", num_envs=4096)
for k in range(60):                                   # alternate the band between sensor and controller, 5 ms each
    lobs, lrew, ldone, linfo = loop.step({"device": torch.full((4096,), k % 2, dtype=torch.int32, device="cuda"),
                                          "duration": torch.full((4096,), 5, dtype=torch.int32, device="cuda")})
rec = loop.get_state("received")
print("control loop: angle %.3f deg, %d samples reached the controller, %d commands the actuator, motor velocity %.3f"
      % (float(linfo["Sensor angle"][0]), int(rec[0, 0]), int(rec[0, 1]), float(loop.get_state("u")[0])))

# 5c. start over, every env from an angle of its own, and compare four cyclic band schedules in one launch
from gymwipe_amd import actions
zero = torch.zeros(4096, dtype=torch.float64)
angles = torch.linspace(-0.3, 0.3, 1024, dtype=torch.float64).repeat(4)           # the same 1 024 angles for every schedule
loop.set_initial_state(torch.stack([zero, zero, angles, zero], 1))
loop.reset_envs()
scheds = actions.make_ctrl_schedules([[(0, 0)], [(0, 19)], [(0, 5), (1, 5)], [(0, 19), (1, 19)]])
tally, sums = loop.rollout_schedules(scheds, episodes=(40, 0.0), steps=40)      # env e follows schedule e // 1024
print("control loop: mean sum of |angle| over a 40-step episode, nobody assigned / sensor only / alternating 5 / alternating 19:",
      [round(v, 1) for v in (sums[:, 3] / sums[:, 0]).tolist()])
loop.set_gains((0.1, 0.0, 0.0))                       # the controller's PID gains (kp, ki, kd), per env if given as [N][3]; default (1, 0, 0)
loop.reset_envs()
print("control loop: the same with kp = 0.1:", [round(v, 1) for v in (lambda s: s[:, 3] / s[:, 0])(loop.rollout_schedules(scheds, (40, 0.0), 40)[1]).tolist()])
loop.set_disturbance((0.0, 0.0, 0.0, 0.01))           # seeded noise on the plant's state at every substep, one key per env (default: its own)
loop.reset_envs()
print("control loop: ... and a plant that is pushed:", [round(v, 1) for v in (lambda s: s[:, 3] / s[:, 0])(loop.rollout_schedules(scheds, (40, 0.0), 40)[1]).tolist()])
loop.set_loss((0.3, 0.3, 0.3, 0.3))                   # seeded packet erasures: a loss probability per link (two announcements, two data links)
loop.reset_envs()
print("control loop: ... over links that lose 30 %:", [round(v, 1) for v in (lambda s: s[:, 3] / s[:, 0])(loop.rollout_schedules(scheds, (40, 0.0), 40)[1]).tolist()],
      "erased per link:", loop.get_state("lost").sum(0).tolist())

# 6. the reference's PHY-grid benchmark (tests/test_benchmark.py), 1 024 replicas of a 16-device grid
import numpy as np
grid = gymwipe_amd.VecPhyGrid(1024, 16, np.random.default_rng(0).uniform(0, 1e-2, (1024, 16)))
grid.runSimulation(0.1)
print("grid: events per replica", float(grid.get_state("events").mean()))
