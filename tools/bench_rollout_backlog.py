#!/usr/bin/env python3
"""
The queue-aware scheduler inside the fused rollout: what env.rollout_backlog costs beside the same steps without a scheduler
and beside what a caller could write before it (profiles/rollout_backlog/README.md).

N envs x D senders, episodes of T steps, one point per delivered packet, calls of 64 steps.  Every handle first runs the same
prologue (six steps of seeded random actions, a reset of every third env), so that the envs differ.  Four legs, each on a
handle of its own, in ONE process, alternated block by block so that clock and thermal drift hit all alike:
  f  env.rollout_backlog(64)                          the fused call
  p  the same under GW_ROLLOUT_POLICY_UNFUSED=1       its per-step form (the switch is read per call)
  r  env.rollout_autoreset(score=) of 64              replays the actions leg f chose in the block before, from the same state:
                                                      the same steps without the scheduler, the cost floor
  c  per step env.get_state("qlen"),                  the composition available before the call existed (a host round trip
     backlog_sample_numpy, env.step_autoreset(score=) per step); `--c-steps` steps per block
A block is `--block` steps (a multiple of 64) of one leg between two HIP events and two wall-clock reads (the second after a
synchronize); blocks are repeated until every leg has at least `--seconds` of stream time.  Reported per leg: the median and
the spread over blocks of the wall-clock and of the event microseconds per step, and the ratios f/r, p/f, c/f of the wall-clock
medians.  Before the timing, f, p and c are checked to choose and deliver the same over the first 64 steps, and r is checked to
deliver what f delivered in every block.  One JSON line; --out appends it to a file.
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
    ap.add_argument("--interval", type=float, default=None, help="counter_interval (default: the reference's 1 ms)")
    ap.add_argument("--block", type=int, default=512, help="steps per timed block (a multiple of 64)")
    ap.add_argument("--c-steps", type=int, default=16, help="steps per block of leg c")
    ap.add_argument("--seconds", type=float, default=0.25, help="stream time per leg at least")
    ap.add_argument("--legs", default="f,p,r,c")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.block > 0 and args.block % 64 == 0

    import torch
    from gymwipe_amd import StepOutputs, VecCounterTrafficEnv, actions

    N, D, T, B = args.envs, args.devices, args.max_steps, args.block
    dev = torch.device("cuda:0")
    K = 64
    policy = actions.make_backlog_policy(D)
    score = actions.make_score(D, reward=0, delivered=1)
    p_dev, p_dur = actions.actions_torch(3, 0, N, 0, 6, D, 20, device=dev)
    third = (torch.arange(N, device=dev) % 3 == 0).to(torch.uint8)

    def new_env():
        env = VecCounterTrafficEnv(N, num_devices=D, device=dev, counter_interval=args.interval)
        env.reset()
        for k in range(6):
            env.step({"device": p_dev[k], "duration": p_dur[k]})
        env.reset(third)
        return env

    names = [x for x in args.legs.split(",") if x]
    envs = {n: new_env() for n in names}
    kinds = (torch.int32, torch.float32, torch.uint8, torch.uint8, torch.int32, torch.int32, torch.int32, torch.int32)
    rows = {n: tuple(torch.empty((K, N), dtype=t, device=dev) for t in kinds) for n in names if n in ("f", "p")}
    rows_r = tuple(torch.empty((K, N), dtype=t, device=dev) for t in kinds[:5])
    chosen = (torch.zeros((B, N), dtype=torch.int32, device=dev), torch.zeros((B, N), dtype=torch.int32, device=dev))
    out_c = StepOutputs(torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.float32, device=dev),
                        torch.empty(N, dtype=torch.uint8, device=dev), ended=torch.empty(N, dtype=torch.uint8, device=dev),
                        delivered=torch.empty(N, dtype=torch.int32, device=dev))
    packets = {n: torch.zeros((), dtype=torch.int64, device=dev) for n in names}
    steps_run = {n: 0 for n in names}

    def backlog_calls(n, steps, keep):
        env, r = envs[n], rows[n]
        for s in range(0, steps, K):
            out = r[:5] + (chosen[0][s:s + K], chosen[1][s:s + K], r[7]) if keep else r
            env.rollout_backlog(K, policy, T, True, score=score, out=out)
            packets[n] += out[4].sum()

    def leg_f(steps):
        backlog_calls("f", steps, "r" in names)

    def leg_p(steps):
        os.environ["GW_ROLLOUT_POLICY_UNFUSED"] = "1"
        try:
            backlog_calls("p", steps, False)
        finally:
            del os.environ["GW_ROLLOUT_POLICY_UNFUSED"]

    def leg_r(steps):
        env = envs["r"]
        for s in range(0, steps, K):
            env.rollout_autoreset(chosen[0][s:s + K], chosen[1][s:s + K], T, True, out=rows_r, score=score)
            packets["r"] += rows_r[4].sum()

    def leg_c(steps):
        env = envs["c"]
        for _ in range(steps):
            d, u, _ = actions.backlog_sample_numpy(policy, env.get_state("qlen"), 20)
            got = env.step_autoreset({"device": torch.from_numpy(d).to(dev), "duration": torch.from_numpy(u).to(dev)}, T, True, out_c,
                                     score=score)
            packets["c"] += got[5].sum()

    legs = {"f": leg_f, "p": leg_p, "r": leg_r, "c": leg_c}
    block = {n: (args.c_steps if n == "c" else B) for n in names}

    # the legs walk the same steps: over the first 64 the fused form, the per-step form and the composition deliver the same
    first = {}
    for n in [x for x in ("f", "p", "c") if x in names]:
        legs[n](K)
        first[n] = int(packets[n])
        steps_run[n] += K
    assert len(set(first.values())) <= 1 and all(v > 0 for v in first.values()), "the legs walk different steps: %r" % first
    if "r" in names:                                                    # (f's first 64 rows are in `chosen`)
        leg_r(K)
        steps_run["r"] += K
        assert int(packets["r"]) == first["f"], "the replay delivers %d, the scheduler %d" % (int(packets["r"]), first["f"])

    def run(n):                                                         # (r replays the block f ran just before it)
        legs[n](block[n])
        steps_run[n] += block[n]

    if "f" in names and "r" in names:
        order = [n for n in names if n not in ("f", "r")]
        order = ["f", "r"] + order
    else:
        order = [n for n in names if n != "r"]
    for n in order:                                                     # warm-up: first launches, allocator, caches
        run(n)
    torch.cuda.synchronize(dev)
    wall = {n: [] for n in order}
    event = {n: [] for n in order}
    total = {n: 0.0 for n in order}
    while min(total.values()) < args.seconds:
        for n in order:
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
    for env in envs.values():
        env.check()
    if "f" in order and "r" in order:
        assert int(packets["r"]) == int(packets["f"]), "the replay and the scheduler delivered different packets"

    def summary(xs):
        return {"median": round(float(np.median(xs)), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}

    res = {"label": args.label, "gpu": torch.cuda.get_device_name(dev), "envs": N, "devices": D, "max_steps": T,
           "counter_interval": args.interval, "block": block, "blocks": {n: len(wall[n]) for n in order}}
    for n in order:
        res[n] = {"wall_us_per_step": summary(wall[n]), "event_us_per_step": summary(event[n]), "stream_seconds": round(total[n], 3),
                  "delivered_per_env_step": round(int(packets[n]) / (steps_run[n] * N), 5)}
    med = {n: res[n]["wall_us_per_step"]["median"] for n in order}
    res["ratios"] = {"%s/%s" % (a, b): round(med[a] / med[b], 3) for a, b in (("f", "r"), ("p", "f"), ("c", "f")) if a in med and b in med}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
