#!/usr/bin/env python3
"""
Finite-state controllers inside the fused rollout: what env.rollout_controller costs beside its parent, the scored
env.rollout_episodes, and beside the composition a caller could write before it (profiles/rollout_controller/README.md).

N envs x D senders, episodes of T steps, one point per delivered packet, calls of 64 steps.  Every handle first runs the same
prologue (six steps of seeded random actions, a reset of every third env), so that the envs differ.  Six legs in ONE process,
alternated block by block so that clock and thermal drift hit all alike; the five fused ones share a handle, the composed one
has its own:
  e   env.rollout_episodes(score=)            the parent, under a uniform three-row table
  s1  env.rollout_controller, S = 1           the same table as a one-node controller: the parent's rows bit for bit, plus one
                                              LDS byte read and one byte store per step
  s4  env.rollout_controller, S = D           stay-while-productive (duration 19, need 8)
  pp  env.rollout_population(score=)          the population parent: P tables
  cp  env.rollout_controller_population       P controllers of S = D nodes
  t   per step env.step_autoreset(score=)     the composition available before the call existed: stay-while-productive kept
      and the node's update in torch          in torch tensors on the device, no host round trip; `--t-steps` steps per block
A block is `--block` steps (a multiple of 64) of one leg between two HIP events and two wall-clock reads (the second after a
synchronize); blocks are repeated until every leg has at least `--seconds` of stream time.  Reported per leg: the median and
the spread over blocks of the wall-clock and of the event microseconds per step, and the ratios s1/e, s4/e, cp/pp, t/s4 of the
wall-clock medians.  Before the timing, s1 is checked to give e's rows and t to deliver what s4 delivers over the first 64
steps, each pair from one state.  One JSON line; --out appends it to a file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--devices", type=int, default=4)
    ap.add_argument("--max-steps", type=int, default=8, help="episode length T")
    ap.add_argument("--policies", type=int, default=256, help="P of the two population legs")
    ap.add_argument("--interval", type=float, default=None, help="counter_interval (default: the reference's 1 ms)")
    ap.add_argument("--block", type=int, default=512, help="steps per timed block (a multiple of 64)")
    ap.add_argument("--t-steps", type=int, default=64, help="steps per block of leg t")
    ap.add_argument("--seconds", type=float, default=0.25, help="stream time per leg at least")
    ap.add_argument("--legs", default="e,s1,s4,pp,cp,t")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.block > 0 and args.block % 64 == 0

    import torch
    from gymwipe_amd import StepOutputs, VecCounterTrafficEnv, actions

    N, D, T, B, P = args.envs, args.devices, args.max_steps, args.block, args.policies
    dev = torch.device("cuda:0")
    K, md, NEED = 64, 20, 8
    score = actions.make_score(D, reward=0, delivered=1)
    table = actions.policy_cdf(np.full((3, D * md), 1.0 / (D * md)))
    one = actions.make_controller(D, table[None], np.zeros((1, 3, 2), np.uint8), [0], md)
    stay = actions.stay_while_productive_controller(D, md - 1, NEED, md)
    p_dev, p_dur = actions.actions_torch(3, 0, N, 0, 6, D, md, device=dev)
    third = (torch.arange(N, device=dev) % 3 == 0).to(torch.uint8)

    def new_env():
        env = VecCounterTrafficEnv(N, num_devices=D, device=dev, counter_interval=args.interval)
        env.reset()
        for k in range(6):
            env.step({"device": p_dev[k], "duration": p_dur[k]})
        env.reset(third)
        return env

    names = [x for x in args.legs.split(",") if x]
    fused, composed = new_env(), new_env()
    kinds = (torch.int32, torch.int32, torch.int32, torch.float32, torch.uint8, torch.uint8, torch.int32, torch.uint8)
    rows = tuple(torch.empty((K, N), dtype=t, device=dev) for t in kinds)

    def up(arrays):                                                     # a controller's arrays as tensors the calls read in place
        return tuple(torch.from_numpy(np.array(a.view(np.int32) if a.dtype == np.uint32 else a, order="C")).to(dev) for a in arrays)

    table_d = torch.from_numpy(table.view(np.int32)).to(dev)
    tables_d = table_d[None].repeat(P, 1, 1).contiguous()
    one_d, stay_d = up(one), up(stay)
    stays_d = tuple(a[None].repeat((P,) + (1,) * a.dim()).contiguous() for a in stay_d)
    tally = torch.zeros((P, 5), dtype=torch.int64, device=dev)
    out_t = StepOutputs(torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.float32, device=dev),
                        torch.empty(N, dtype=torch.uint8, device=dev), ended=torch.empty(N, dtype=torch.uint8, device=dev),
                        delivered=torch.empty(N, dtype=torch.int32, device=dev))
    node_t = torch.zeros(N, dtype=torch.int32, device=dev)
    dur_t = torch.full((N,), md - 1, dtype=torch.int32, device=dev)
    packets = {n: torch.zeros((), dtype=torch.int64, device=dev) for n in names}
    steps_run = {n: 0 for n in names}
    step0 = {"v": 0}

    def calls(steps, one_call):
        for _ in range(0, steps, K):
            one_call(step0["v"])
            step0["v"] += K

    def leg_e(steps):
        calls(steps, lambda s: fused.rollout_episodes(table_d, K, 1, T, True, step0=s, out=rows[:7], score=score))

    def leg_s1(steps):
        calls(steps, lambda s: fused.rollout_controller(one_d, K, 1, T, True, step0=s, out=rows, score=score))

    def leg_s4(steps):
        calls(steps, lambda s: fused.rollout_controller(stay_d, K, 1, T, True, step0=s, out=rows, score=score))

    def leg_pp(steps):
        calls(steps, lambda s: fused.rollout_population(tables_d, K, 1, T, True, step0=s, tally=tally, score=score))

    def leg_cp(steps):
        calls(steps, lambda s: fused.rollout_controller_population(stays_d, K, 1, T, True, step0=s, tally=tally, score=score))

    def leg_t(steps):
        for _ in range(steps):
            composed.step_autoreset({"device": node_t, "duration": dur_t}, T, True, out_t, score=score)
            moved = torch.where(out_t.delivered >= NEED, node_t, (node_t + 1) % D)
            node_t.copy_(torch.where(out_t.ended != 0, torch.zeros_like(node_t), moved))
            packets["t"] += out_t.delivered.sum()

    legs = {"e": leg_e, "s1": leg_s1, "s4": leg_s4, "pp": leg_pp, "cp": leg_cp, "t": leg_t}
    block = {n: (args.t_steps if n == "t" else B) for n in names}

    # the legs mean what they say: from one state, the one-node controller gives the parent's rows, and the composition
    # delivers what the fused stay-while-productive controller delivers
    snap = fused.snapshot()
    first = fused._last[0].clone()
    want = [r.clone() for r in fused.rollout_episodes(table_d, K, 1, T, True, obs_prev=first, score=score)]
    fused.restore(snap)
    fused.episode_state.zero_()
    got = fused.rollout_controller(one_d, K, 1, T, True, obs_prev=first, score=score)
    assert all(torch.equal(a, b) for a, b in zip(want, got[:7])), "the one-node controller does not give the parent's rows"
    fused.restore(snap)
    fused.episode_state.zero_()
    fused.controller_node.zero_()
    fused_packets = int(fused.rollout_controller(stay_d, K, 1, T, True, obs_prev=first, score=score)[6].sum())
    if "t" in names:
        leg_t(K)
        steps_run["t"] += K
        assert int(packets["t"]) == fused_packets > 0, "the composition delivers %d, the fused controller %d" % (int(packets["t"]), fused_packets)

    def run(n):
        legs[n](block[n])
        steps_run[n] += block[n]

    for n in names:                                                     # warm-up: first launches, allocator, caches
        run(n)
    torch.cuda.synchronize(dev)
    wall = {n: [] for n in names}
    event = {n: [] for n in names}
    total = {n: 0.0 for n in names}
    while min(total.values()) < args.seconds:
        for n in names:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            e0.record()
            run(n)
            e1.record()
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            ms = e0.elapsed_time(e1)
            wall[n].append((t1 - t0) / block[n] * 1e6)
            event[n].append(ms * 1e3 / block[n])
            total[n] += ms * 1e-3
    fused.check()
    composed.check()

    def summary(xs):
        return {"median": round(float(np.median(xs)), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}

    res = {"label": args.label, "gpu": torch.cuda.get_device_name(dev), "envs": N, "devices": D, "max_steps": T, "policies": P,
           "counter_interval": args.interval, "block": block, "blocks": {n: len(wall[n]) for n in names}}
    for n in names:
        res[n] = {"wall_us_per_step": summary(wall[n]), "event_us_per_step": summary(event[n]), "stream_seconds": round(total[n], 3)}
    med = {n: res[n]["wall_us_per_step"]["median"] for n in names}
    res["ratios"] = {"%s/%s" % (a, b): round(med[a] / med[b], 3)
                     for a, b in (("s1", "e"), ("s4", "e"), ("cp", "pp"), ("t", "s4")) if a in med and b in med}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
