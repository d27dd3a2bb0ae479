#!/usr/bin/env python3
"""
Autoreset for a caller that chooses the actions: what env.step_autoreset / env.rollout_autoreset cost beside what a caller
writes without them (profiles/step_autoreset/README.md).

N envs x D senders, episodes of at most T steps (ended by done too), a seeded action stream of 64 rows used round and round.
Five legs, each on a handle of its own, in ONE process, alternated block by block so that clock and thermal drift hit all alike:
  a  env.step(action, out)                          no episodes at all: context
  b  env.step(), then what a caller writes today    age += 1, ret += reward, the end mask (done | age >= T), the episode count
                                                    and return sum, age / ret zeroed, env.reset(mask), torch.where for the
                                                    observation to act on next: the baseline
  c  env.step_autoreset(action, T, out=...)         the feature, one launch
  d  env.rollout() of 64 steps                      context
  e  env.rollout_autoreset() of 64 steps            the feature
Scored legs (profiles/autoreset_scored/README.md), behind names of their own -- `--legs s1,s0,s2,s3,r1,r0,r2,r3`; the score is one
point per delivered packet, make_score(D, reward=0, delivered=1):
  s1  env.step_autoreset(action, T, out=..., score=)   the scored one-step form, fused
  s0  env.step_autoreset(action, T, out=...)           the unscored parent call on the same box (leg c on a handle of its own)
  s2  s1 on a handle created with GW_ROLLOUT_CAP=0     the scored call's own per-step form
  s3  the composition available before                 gw_delivered, step_autoreset, gw_delivered, the difference and the score in
                                                       torch (it cannot reach {age, ret} or the tally: written inside the launch)
  r1 / r0 / r2 / r3                                    the same four for a rollout of 64: env.rollout_autoreset(score=); r3 is s3
                                                       per step with the packets and the score written into [64][N] rows
A block is `--block` steps (a multiple of 64) of one leg between two HIP events and two wall-clock reads (the second after a
synchronize); blocks are repeated until every leg has at least `--seconds` of stream time.  Reported per leg: the median and
the spread over blocks of the wall-clock and of the event microseconds per step.  b and c walk the same trajectory (checked
once, before the timing: the same rewards and the same episode count).  One JSON line; --out appends it to a file.
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
    ap.add_argument("--block", type=int, default=1024, help="steps per timed block (a multiple of 64)")
    ap.add_argument("--seconds", type=float, default=0.25, help="stream time per leg at least")
    ap.add_argument("--legs", default="a,b,c,d,e")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.block > 0 and args.block % 64 == 0

    import torch
    from gymwipe_amd import StepOutputs, VecCounterTrafficEnv, actions

    N, D, T, B = args.envs, args.devices, args.max_steps, args.block
    dev = torch.device("cuda:0")
    K = 64
    a_dev, a_dur = actions.actions_torch(3, 0, N, 0, K, D, 20, device=dev)
    acts = [{"device": a_dev[k], "duration": a_dur[k]} for k in range(K)]     # the same tensor objects every round: cached

    def new_env():
        env = VecCounterTrafficEnv(N, num_devices=D, device=dev)
        env.reset()
        return env

    def outputs(ended=False):
        return StepOutputs(torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.float32, device=dev),
                           torch.empty(N, dtype=torch.uint8, device=dev),
                           ended=torch.empty(N, dtype=torch.uint8, device=dev) if ended else None)

    envs = {leg: new_env() for leg in "abcde"}                          # (the scored legs' handles: below, where they are named)
    center = int(envs["a"].config.counter_bound)
    out_a, out_b, out_c = outputs(), outputs(), outputs(ended=True)
    out3 = (torch.empty((K, N), dtype=torch.int32, device=dev), torch.empty((K, N), dtype=torch.float32, device=dev),
            torch.empty((K, N), dtype=torch.uint8, device=dev))
    out4 = tuple(torch.empty_like(t) for t in out3) + (torch.empty((K, N), dtype=torch.uint8, device=dev),)
    age = torch.zeros(N, dtype=torch.int32, device=dev)
    ret = torch.zeros(N, dtype=torch.float32, device=dev)
    tally_b = torch.zeros(2, dtype=torch.float64, device=dev)          # episodes, return sum
    centre_row = torch.full((N,), center, dtype=torch.int32, device=dev)
    state = {"next_b": None}

    def leg_a(steps):
        env = envs["a"]
        for s in range(steps):
            env.step(acts[s % K], out_a)

    def leg_b(steps):
        env = envs["b"]
        for s in range(steps):
            obs, rew, done, _ = env.step(acts[s % K], out_b)
            age.add_(1)
            ret.add_(rew)
            end = (done != 0) | (age >= T)
            tally_b[0] += end.sum()
            tally_b[1] += (ret * end).sum()
            age.masked_fill_(end, 0)
            ret.masked_fill_(end, 0.0)
            env.reset(end)
            state["next_b"] = torch.where(end, centre_row, obs)

    def leg_c(steps):
        env = envs["c"]
        for s in range(steps):
            env.step_autoreset(acts[s % K], T, True, out_c)

    def leg_d(steps):
        env = envs["d"]
        for _ in range(steps // K):
            env.rollout(a_dev, a_dur, out=out3)

    def leg_e(steps):
        env = envs["e"]
        for _ in range(steps // K):
            env.rollout_autoreset(a_dev, a_dur, T, True, out=out4)

    legs = {"a": leg_a, "b": leg_b, "c": leg_c, "d": leg_d, "e": leg_e}
    names = [x for x in args.legs.split(",") if x]

    # ---- the scored legs: handles and buffers only for the legs asked for ----
    scored = [n for n in names if n in ("s0", "s1", "s2", "s3", "r0", "r1", "r2", "r3")]
    if scored:
        from gymwipe_amd import _native as nat
        score = actions.make_score(D, reward=0, delivered=1)
        w = torch.from_numpy(score.astype(np.int64)).to(dev)

        def outputs_scored():
            o = outputs(ended=True)
            return StepOutputs(o.obs, o.reward, o.done, ended=o.ended, delivered=torch.empty(N, dtype=torch.int32, device=dev))

        for n in scored:
            if n.endswith("2"):
                os.environ["GW_ROLLOUT_CAP"] = "0"                     # read when the handle is created: no fused rollout
            envs[n] = new_env()
            os.environ.pop("GW_ROLLOUT_CAP", None)
        so = {n: (outputs_scored() if n in ("s1", "s2") else outputs(ended=True)) for n in scored if n[0] == "s" or n == "r3"}
        rows5 = {n: out4 + (torch.empty((K, N), dtype=torch.int32, device=dev),) for n in scored if n in ("r1", "r2", "r3")}
        rows5 = {n: tuple(torch.empty_like(t) for t in r) for n, r in rows5.items()}
        deliv = {n: (torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev))
                 for n in scored if n.endswith("3")}

        def one_step(n, with_score):
            env, out = envs[n], so[n]
            kw = {"score": score} if with_score else {}

            def run(steps):
                for s in range(steps):
                    env.step_autoreset(acts[s % K], T, True, out, **kw)
            return run

        def rollout64(n, with_score):
            env = envs[n]
            kw = {"score": score, "out": rows5[n]} if with_score else {"out": out4}

            def run(steps):
                for _ in range(steps // K):
                    env.rollout_autoreset(a_dev, a_dur, T, True, **kw)
            return run

        def composition(n, keep_rows):
            env, out, (before, after) = envs[n], so[n], deliv[n]
            L, h = env._L, env._h

            def run(steps):
                for s in range(steps):
                    k = s % K
                    nat.check(L.gw_delivered(h, before.data_ptr(), env._stream()))
                    obs, rew, done, ended, nxt = env.step_autoreset(acts[k], T, True, out)
                    nat.check(L.gw_delivered(h, after.data_ptr(), env._stream()))
                    dl = after - before
                    sc = w[0] * rew.to(torch.int64) + w[1 + a_dev[k].to(torch.int64)] * dl
                    if keep_rows:
                        r = rows5[n]
                        r[0][k].copy_(obs); r[1][k].copy_(sc); r[2][k].copy_(done); r[3][k].copy_(ended); r[4][k].copy_(dl)
                    else:
                        rew.copy_(sc)
            return run

        legs.update({"s1": lambda: one_step("s1", True), "s0": lambda: one_step("s0", False), "s2": lambda: one_step("s2", True),
                     "s3": lambda: composition("s3", False), "r1": lambda: rollout64("r1", True), "r0": lambda: rollout64("r0", False),
                     "r2": lambda: rollout64("r2", True), "r3": lambda: composition("r3", True)})
        for n in scored:
            legs[n] = legs[n]()
        # the fused, the per-step and the composed form score the same steps: one round of the stream from fresh handles
        sums = {}
        for n in [x for x in ("s1", "s2", "s3") if x in scored]:
            total_sc = 0.0
            for s in range(K):
                if n == "s3":                                           # (one point per packet: the score is the difference)
                    nat.check(envs[n]._L.gw_delivered(envs[n]._h, deliv[n][0].data_ptr(), envs[n]._stream()))
                    envs[n].step_autoreset(acts[s], T, True, so[n])
                    nat.check(envs[n]._L.gw_delivered(envs[n]._h, deliv[n][1].data_ptr(), envs[n]._stream()))
                    total_sc += float((deliv[n][1] - deliv[n][0]).double().sum())
                else:
                    total_sc += float(envs[n].step_autoreset(acts[s], T, True, so[n], score=score)[1].double().sum())
            sums[n] = total_sc
            envs[n].reset()
        assert len(set(sums.values())) <= 1 and all(v > 0 for v in sums.values()), "the scored legs walk different steps: %r" % sums

    # b and c walk the same steps: rewards and episode count over one round of the stream, from fresh handles
    if "b" in names and "c" in names:
        rew_b = rew_c = 0.0
        for s in range(K):
            leg_b_env, leg_c_env = envs["b"], envs["c"]
            obs, rew, done, _ = leg_b_env.step(acts[s], out_b)
            age.add_(1)
            end = (done != 0) | (age >= T)
            age.masked_fill_(end, 0)
            leg_b_env.reset(end)
            rew_b += float(rew.double().sum())
            rew_c += float(leg_c_env.step_autoreset(acts[s], T, True, out_c)[1].double().sum())
        assert rew_b == rew_c, "b and c walk different steps"
        assert envs["c"].episode_stats()["episodes"] == N * (K // T), "c ended other episodes than every T-th step"
        age.zero_()
        envs["b"].reset()
        envs["c"].reset()

    for n in names:                                                    # warm-up: first launches, allocator, caches
        legs[n](256)
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
            legs[n](B)
            e1.record()
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            ms = e0.elapsed_time(e1)
            wall[n].append((t1 - t0) / B * 1e6)
            event[n].append(ms * 1e3 / B)
            total[n] += ms * 1e-3
    for env in envs.values():
        env.check()

    def summary(xs):
        return {"median": round(float(np.median(xs)), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}

    res = {"label": args.label, "gpu": torch.cuda.get_device_name(dev), "envs": N, "devices": D, "max_steps": T, "block": B,
           "blocks": {n: len(wall[n]) for n in names}}
    for n in names:
        res[n] = {"wall_us_per_step": summary(wall[n]), "event_us_per_step": summary(event[n]),
                  "stream_seconds": round(total[n], 3)}
    if "b" in names:
        res["b"]["episodes_counted"] = int(tally_b[0])
    if "c" in names:
        res["c"]["episodes"] = envs["c"].episode_stats()["episodes"]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
