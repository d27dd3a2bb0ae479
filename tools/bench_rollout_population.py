#!/usr/bin/env python3
"""
A population of policies in one launch: what env.rollout_population costs beside what a caller writes without it
(profiles/rollout_population/README.md).

N envs x D senders in all, episodes of at most T steps, P policy tables of M = N / P envs each, for every (P, M) of --shapes.
Legs, each on handles of its own, in ONE process, alternated block by block so that clock and thermal drift hit all alike:
  a<P>  env.rollout_population(cdfs[P], 64, ...)     the feature: one handle of N envs, one launch per 64 steps, the [P][5]
                                                     tally read back once per block
  b<P>  what a caller writes today                   P handles of M envs, env.rollout_episodes(cdfs[p], 64, ...) on each (into
                                                     one shared set of [64][M] buffers), the P episode tallies stacked and read
                                                     back once per block.  A shape whose P handles take longer than --b-budget
                                                     seconds to create is left out, and the result says so ("b_skipped")
  c     env.rollout_episodes(cdf, 64, ...)           one table on one handle of N envs: the same walk plus six [64][N] stores
A block is `--block` steps (a multiple of 64) of one leg between two HIP events and two wall-clock reads (the second after a
synchronize); blocks are repeated until every leg has at least `--seconds` of stream time (or `--wall-limit` is reached).  Reported per leg: the median and
the spread over blocks of the wall-clock and of the event microseconds per step of all N envs, and per shape the ratio b / a
block by block (median, min, max).  Before the timing: with all P tables the same table, a's per-policy rows sum to c's tally (on handles of the check's own);
after it: a and b, which ran the same envs, ids and tables, hold the same [P][5] tally ("a_equals_b").
One JSON line; --out appends it to a file.
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
    ap.add_argument("--shapes", default="1024,64", help="numbers of policies P (each divides --envs)")
    ap.add_argument("--block", type=int, default=1024, help="steps per timed block (a multiple of 64)")
    ap.add_argument("--seconds", type=float, default=0.25, help="stream time per leg at least")
    ap.add_argument("--b-budget", type=float, default=60.0, help="seconds the creation of one shape's P handles may take")
    ap.add_argument("--wall-limit", type=float, default=240.0, help="the timing loop ends after this many seconds at the latest")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.block > 0 and args.block % 64 == 0

    import torch
    from gymwipe_amd import VecCounterTrafficEnv, actions

    N, D, T, B = args.envs, args.devices, args.max_steps, args.block
    dev = torch.device("cuda:0")
    K, SEED = 64, 3
    A = D * 20
    shapes = [int(x) for x in args.shapes.split(",") if x]
    assert all(P > 0 and N % P == 0 for P in shapes)
    rng = np.random.default_rng(5)
    p_all = rng.dirichlet(np.full(A, 0.3), size=(max(shapes), 3))
    cdfs_np = actions.policy_cdf(p_all)                                 # [Pmax][3][A]; a shape uses its first P

    def new_env(n):
        env = VecCounterTrafficEnv(n, num_devices=D, device=dev)
        env.reset()
        return env

    def as_words(x):                                                   # the 32-bit form the env uses in place
        return torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).to(dev)

    kinds = (torch.int32, torch.int32, torch.int32, torch.float32, torch.uint8, torch.uint8)
    legs, pos, extra, skipped = {}, {}, {}, {}

    # c: one table, one handle
    env_c, cdf_c = new_env(N), as_words(cdfs_np[0])
    out_c = tuple(torch.empty((K, N), dtype=dt, device=dev) for dt in kinds)

    def leg_c(steps):
        for _ in range(steps // K):
            env_c.rollout_episodes(cdf_c, K, SEED, max_steps=T, step0=pos["c"], out=out_c)
            pos["c"] += K
        return env_c.episode_tally.cpu()

    legs["c"], pos["c"] = leg_c, 0

    for P in shapes:
        M = N // P
        env_a, cdfs_a = new_env(N), as_words(cdfs_np[:P])
        tally_a = torch.zeros((P, 5), dtype=torch.int64, device=dev)

        # the check, on two handles of its own: P copies of c's table -- the rows' column sums are c's tally
        chk_a, chk_c = new_env(N), new_env(N)
        rows = chk_a.rollout_population(as_words(np.broadcast_to(cdfs_np[0], (P, 3, A))), K, SEED, max_steps=T)
        chk_c.rollout_episodes(cdf_c, K, SEED, max_steps=T, out=out_c)
        want = chk_c.episode_tally.cpu()
        assert int(want[0]) == N * (K // T) and torch.equal(rows.sum(dim=0).cpu(), want), "a and c walk different steps"
        assert torch.equal(chk_a.episode_tally.cpu(), want) and torch.equal(chk_a.episode_state, chk_c.episode_state)
        chk_a.close()
        chk_c.close()

        def leg_a(steps, env=env_a, cdfs=cdfs_a, tally=tally_a, name="a%d" % P):
            for _ in range(steps // K):
                env.rollout_population(cdfs, K, SEED, max_steps=T, step0=pos[name], tally=tally)
                pos[name] += K
            return tally.cpu()

        legs["a%d" % P], pos["a%d" % P] = leg_a, 0

        t0 = time.perf_counter()
        envs_b = []
        for _ in range(P):
            envs_b.append(new_env(M))
            if time.perf_counter() - t0 > args.b_budget:
                break
        extra["b%d_create_seconds" % P] = round(time.perf_counter() - t0, 2)
        if len(envs_b) < P:
            skipped["b%d" % P] = "%d of %d handles in %.0f s" % (len(envs_b), P, args.b_budget)
            for env in envs_b:
                env.close()
            continue
        cdfs_b = [cdfs_a[p] for p in range(P)]
        out_b = tuple(torch.empty((K, M), dtype=dt, device=dev) for dt in kinds)

        def leg_b(steps, envs=envs_b, cdfs=cdfs_b, out=out_b, M=M, name="b%d" % P):
            for _ in range(steps // K):
                for p, env in enumerate(envs):
                    env.rollout_episodes(cdfs[p], K, SEED, max_steps=T, step0=pos[name], env_id0=p * M, out=out)
                pos[name] += K
            return torch.stack([env.episode_tally for env in envs]).cpu()

        legs["b%d" % P], pos["b%d" % P] = leg_b, 0

    names = list(legs)
    last = {}
    for n in names:                                                    # warm-up: first launches, allocator, caches
        legs[n](2 * K)
    torch.cuda.synchronize(dev)
    wall = {n: [] for n in names}
    event = {n: [] for n in names}
    total = {n: 0.0 for n in names}
    began = time.perf_counter()
    while min(total.values()) < args.seconds and not (wall[names[0]] and time.perf_counter() - began > args.wall_limit):
        for n in names:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            e0.record()
            last[n] = legs[n](B)
            e1.record()
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            ms = e0.elapsed_time(e1)
            wall[n].append((t1 - t0) / B * 1e6)
            event[n].append(ms * 1e3 / B)
            total[n] += ms * 1e-3

    def summary(xs):
        return {"median": round(float(np.median(xs)), 3), "min": round(float(min(xs)), 3), "max": round(float(max(xs)), 3)}

    res = {"label": args.label, "gpu": torch.cuda.get_device_name(dev), "envs": N, "devices": D, "max_steps": T, "block": B,
           "shapes": [[P, N // P] for P in shapes], "blocks": {n: len(wall[n]) for n in names}, "b_skipped": skipped}
    res.update(extra)
    for n in names:
        res[n] = {"wall_us_per_step": summary(wall[n]), "event_us_per_step": summary(event[n]),
                  "stream_seconds": round(total[n], 3), "episodes": int(last[n].reshape(-1, 5)[:, 0].sum())}
    for P in shapes:
        a, b = "a%d" % P, "b%d" % P
        if b in legs:                                                  # a and b: the same envs, ids and tables -- the same episodes
            res["a_equals_b_%d" % P] = bool(torch.equal(last[a], last[b]))
            res["b_over_a_%d" % P] = {"wall": summary([y / x for x, y in zip(wall[a], wall[b])]),
                                      "event": summary([y / x for x, y in zip(event[a], event[b])])}
        res["a_over_c_%d" % P] = {"wall": summary([x / y for x, y in zip(wall[a], wall["c"])]),
                                  "event": summary([x / y for x, y in zip(event[a], event["c"])])}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
