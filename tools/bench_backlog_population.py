#!/usr/bin/env python3
"""
Tuning the queue-aware scheduler in one launch: what env.rollout_backlog_population costs beside its per-step form, beside the
rows-writing parent and beside what a caller could write before it (profiles/backlog_population/README.md).

N envs x D senders, P policies on M = N / P envs each, episodes of T steps, one point per delivered packet, calls of 64 steps.
Every handle first runs the same prologue (six steps of seeded random actions, a reset of every third env), so that the envs
differ.  By default the P policies are P copies of the default policy, so that all legs walk the same steps (`--slopes`: policy
p takes duration_of_len[L] = min(19, s L) with s cycling through 1 ... 8 and 19 instead; legs f, p and h then still walk the
same steps).  Four legs in ONE process, alternated block by block so that clock and thermal drift hit all alike:
  f  env.rollout_backlog_population(64)               the fused call, policies in a device tensor, the tally added into
  p  the same under GW_ROLLOUT_POLICY_UNFUSED=1       its per-step form (the switch is read per call), on a handle of its own
  b  env.rollout_backlog(64), the default policy      the rows-writing parent on a handle of the same size: eight [64][N] rows
  h  P handles of M envs, env.rollout_backlog(64)     the composition available before: one call per candidate, each tally
     on each, the tallies summed                      read from the handle's episode_tally
A block is `--block` steps (a multiple of 64) of one leg between two HIP events and two wall-clock reads (the second after a
synchronize); blocks are repeated until every leg has at least `--seconds` of stream time.  Reported per leg: the median and the
spread over blocks of the wall-clock and of the event microseconds per step (a step of leg h is one step of all P handles), and
the ratios p/f, f/b, h/f of the wall-clock medians.  Before the timing, the legs' episode tallies over the first 64 steps are
compared (`agree`).  One JSON line; --out appends it to a file.
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
    ap.add_argument("--policies", type=int, default=64)
    ap.add_argument("--max-steps", type=int, default=8, help="episode length T")
    ap.add_argument("--interval", type=float, default=None, help="counter_interval (default: the reference's 1 ms)")
    ap.add_argument("--slopes", action="store_true", help="P different duration tables instead of P copies of the default")
    ap.add_argument("--block", type=int, default=512, help="steps per timed block (a multiple of 64)")
    ap.add_argument("--seconds", type=float, default=0.25, help="stream time per leg at least")
    ap.add_argument("--legs", default="f,p,b,h")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.block > 0 and args.block % 64 == 0 and args.envs % args.policies == 0

    import torch
    from gymwipe_amd import VecCounterTrafficEnv, actions

    N, D, P, T, B = args.envs, args.devices, args.policies, args.max_steps, args.block
    M = N // P
    dev = torch.device("cuda:0")
    K = 64
    default = actions.make_backlog_policy(D)
    if args.slopes:
        slopes = (1, 2, 3, 4, 5, 6, 7, 8, 19)
        images = [actions.make_backlog_policy(D, 1, np.minimum(19, slopes[p % len(slopes)] * np.arange(actions.QUEUE_CAP + 1)))
                  for p in range(P)]
    else:
        images = [default] * P
    population = torch.from_numpy(actions.make_backlog_population(images)).to(dev)
    score = actions.make_score(D, reward=0, delivered=1)
    p_dev, p_dur = actions.actions_torch(3, 0, N, 0, 6, D, 20, device=dev)
    third = (torch.arange(N, device=dev) % 3 == 0).to(torch.uint8)

    def new_env(lo=0, n=N):
        env = VecCounterTrafficEnv(n, num_devices=D, device=dev, counter_interval=args.interval)
        env.reset()
        for k in range(6):
            env.step({"device": p_dev[k][lo:lo + n].contiguous(), "duration": p_dur[k][lo:lo + n].contiguous()})
        env.reset(third[lo:lo + n].contiguous())
        return env

    names = [x for x in args.legs.split(",") if x]
    envs = {n: new_env() for n in names if n != "h"}
    small = [new_env(p * M, M) for p in range(P)] if "h" in names else []
    kinds = (torch.int32, torch.float32, torch.uint8, torch.uint8, torch.int32, torch.int32, torch.int32, torch.int32)
    rows_b = tuple(torch.empty((K, N), dtype=t, device=dev) for t in kinds) if "b" in names else None
    rows_h = tuple(torch.empty((K, M), dtype=t, device=dev) for t in kinds) if small else None
    tally = {n: torch.zeros((P, actions.EP_COLS), dtype=torch.int64, device=dev) for n in names}
    steps_run = {n: 0 for n in names}

    def leg_f(steps):
        for _ in range(0, steps, K):
            envs["f"].rollout_backlog_population(population, K, T, True, score=score, tally=tally["f"])

    def leg_p(steps):
        os.environ["GW_ROLLOUT_POLICY_UNFUSED"] = "1"
        try:
            for _ in range(0, steps, K):
                envs["p"].rollout_backlog_population(population, K, T, True, score=score, tally=tally["p"])
        finally:
            del os.environ["GW_ROLLOUT_POLICY_UNFUSED"]

    def leg_b(steps):
        for _ in range(0, steps, K):
            envs["b"].rollout_backlog(K, default, T, True, score=score, out=rows_b)
        tally["b"][0] = envs["b"].episode_tally                          # (one policy: one row)

    def leg_h(steps):
        for _ in range(0, steps, K):
            for p, env in enumerate(small):
                env.rollout_backlog(K, images[p], T, True, score=score, out=rows_h)
        torch.stack([env.episode_tally for env in small], out=tally["h"])

    legs = {"f": leg_f, "p": leg_p, "b": leg_b, "h": leg_h}

    def run(n, steps=B):
        legs[n](steps)
        steps_run[n] += steps

    for n in names:                                                     # the first 64 steps: do the legs walk the same steps?
        run(n, K)
    torch.cuda.synchronize(dev)
    first = {n: tally[n].cpu().numpy() for n in names}
    agree = {}
    if "f" in first and "p" in first:
        agree["p == f"] = bool((first["p"] == first["f"]).all())
        assert agree["p == f"], "the per-step form and the fused one tally differently"
    if "f" in first and "h" in first:
        agree["h == f"] = bool((first["h"] == first["f"]).all())
    if "f" in first and "b" in first and not args.slopes:
        agree["b == sum f"] = bool((first["b"][0] == first["f"].sum(axis=0)).all())
    assert all(int(t[:, 0].sum()) > 0 for t in first.values()), "no episode ended"

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
            wall[n].append((t1 - t0) / B * 1e6)
            event[n].append(ms * 1e3 / B)
            total[n] += ms * 1e-3
    for env in list(envs.values()) + small:
        env.check()

    def summary(xs):
        return {"median": round(float(np.median(xs)), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}

    res = {"label": args.label, "gpu": torch.cuda.get_device_name(dev), "envs": N, "devices": D, "policies": P, "max_steps": T,
           "counter_interval": args.interval, "slopes": bool(args.slopes), "block": B, "blocks": {n: len(wall[n]) for n in names},
           "agree": agree}
    for n in names:
        t = tally[n].cpu().numpy()
        res[n] = {"wall_us_per_step": summary(wall[n]), "event_us_per_step": summary(event[n]), "stream_seconds": round(total[n], 3),
                  "steps": steps_run[n], "episodes": int(t[:, 0].sum()), "packets_per_episode": round(float(t[:, 3].sum()) / max(1, int(t[:, 0].sum())), 4)}
    med = {n: res[n]["wall_us_per_step"]["median"] for n in names}
    res["ratios"] = {"%s/%s" % (a, b): round(med[a] / med[b], 3) for a, b in (("p", "f"), ("f", "b"), ("h", "f")) if a in med and b in med}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
