#!/usr/bin/env python3
"""
Closed-loop rollout: what the policy inside the launch buys (profiles/rollout_policy/README.md).

Windows of K steps at N envs x D senders, a reset between windows, three forms of the same work:
  a  env.rollout             pre-staged actions, one persistent launch per window (no policy at all: the ceiling)
  b  per-step closed loop    what a caller does without gw_rollout_policy: per step, the observation's class, a draw,
                             torch.searchsorted on the same table, the flat action split, env.step()
  c  env.rollout_policy      the draw inside the launch; with GW_ROLLOUT_POLICY_UNFUSED=1 its unfused form
The stats leg (profiles/rollout_stats/README.md) -- the same closed loop for a caller that wants the table over (observation
class, action), not the transitions:
  t  rollout_policy + torch  c, then the table built with torch (bincount per column): what a caller without
                             gw_rollout_policy_stats writes
  r  rollout_policy + env.transition_stats   c, then the table by gw_transition_stats
  s  env.rollout_policy_stats                the tally inside the launch, no [K][N] array at all
The episodes leg (--episodes T; profiles/rollout_episodes/README.md) -- episodes of T steps inside the launch against the only
way to get the same trajectory without gw_rollout_episodes, a launch per T steps and a reset() in between:
  e0 env.rollout_episodes, both limits off   against c: what the hook at the end of a step costs when it never fires
  p  rollout_policy(T) + reset()             K / T calls of each per window
  e  env.rollout_episodes(max_steps=T)       one call per window
  q  rollout_policy_stats(T) + reset()       the same two for the tally
  f  env.rollout_episodes_stats(max_steps=T)
p/e and q/f walk the same steps (checked once, before the timing: the same reward sum, the same table).  Every leg reports the
share of its env-steps with a non-zero reward beside its rate: what the steps are worth.
Each of t, r and s must count every transition (checked once, before the timing; that they produce the same table from the
same steps is tests/test_rollout_stats.py's business).
The scored legs (--scored; profiles/rollout_scored/README.md) -- episodes of T steps (--episodes, default 8) ranked by what they
delivered, score = packets of the assigned sender the RRM decoded; the legs alternate in one process, --repeats rounds each,
median wall time per step over --windows calls of K steps:
  P1 env.rollout_population(score=...)       the fused scored form, P = --policies tables
  P0 env.rollout_population()                unscored on the same box: the cost of scoring
  P2 P1 under GW_ROLLOUT_POLICY_UNFUSED      its own per-step form
  P3 the composition available without it    per step: rollout_episodes(1 step), gw_delivered, the difference, the score and
                                             the per-env return in torch (one table for all envs: rollout_episodes has no
                                             population; the per-policy tally is left out, which favours this leg)
  R1 / R0 / R2 / R3                          the same four for the records form, env.rollout_episodes(score=...)
The delivered-tally legs (--packets; profiles/rollout_stats_delivered/README.md): D1 / D0 / D2, see packets_legs().
Each form is timed `--repeats` times over `--windows` windows (wall clock around a device synchronize); one JSON line with the
best, the median and the spread.  GW_TREE names the checkout whose gymwipe_amd package (and built library) is measured --
default: this file's own -- so one job can run a and b on the parent commit's build and c on this one's; a form the measured
checkout lacks is reported as null.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.environ.get("GW_TREE") or os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def scored_legs(args):
    import ctypes as C
    import torch
    from gymwipe_amd import VecCounterTrafficEnv, actions
    from gymwipe_amd import _native as nat

    N, D, K, T, P, W = args.envs, args.devices, args.steps, args.episodes or 8, args.policies, args.windows
    dev = torch.device("cuda:0")
    md = 20
    A = D * md
    rng = np.random.default_rng(7)
    cdf = actions.policy_cdf(rng.dirichlet(np.full(A, 0.3), size=3))
    cdfs = actions.policy_cdf(rng.dirichlet(np.full(A, 0.3), size=(P, 3)))
    score = actions.make_score(D, reward=0, delivered=1)
    w = torch.from_numpy(score.astype(np.int64)).to(dev)
    kinds = (torch.int32, torch.int32, torch.int32, torch.float32, torch.uint8, torch.uint8, torch.int32)
    envs, step0 = {}, {}

    def env_of(leg):                                           # a handle per leg: each continues its own episodes and stream
        if leg not in envs:
            e = envs[leg] = VecCounterTrafficEnv(N, num_devices=D, device=dev)
            e.reset()
            e.bench = {"table": e._policy_table(cdf), "tables": e._policy_table(cdfs, population=True),
                       "tally": torch.zeros((P, 5), dtype=torch.int64, device=dev),
                       "rows": tuple(torch.empty((K, N), dtype=t, device=dev) for t in kinds),
                       "deliv": torch.zeros((2, N), dtype=torch.int32, device=dev),
                       "ret": torch.zeros(N, dtype=torch.int64, device=dev)}
            step0[leg] = 0
        return envs[leg]

    def population(leg, scored):
        e = env_of(leg)
        e.rollout_population(e.bench["tables"], K, 5, max_steps=T, step0=step0[leg], tally=e.bench["tally"],
                             **({"score": score} if scored else {}))

    def records(leg, scored):
        e = env_of(leg)
        e.rollout_episodes(e.bench["table"], K, 5, max_steps=T, step0=step0[leg],
                           out=e.bench["rows"][:7 if scored else 6], **({"score": score} if scored else {}))

    def composed(leg, keep_rows):
        e = env_of(leg)
        b = e.bench
        L, h = nat.lib(), e._h
        for k in range(K):
            nat.check(L.gw_delivered(h, b["deliv"][0].data_ptr(), e._stream()))
            out = tuple(r[k:k + 1] for r in b["rows"][:6])
            e.rollout_episodes(b["table"], 1, 5, max_steps=T, step0=step0[leg] + k, out=out)
            nat.check(L.gw_delivered(h, b["deliv"][1].data_ptr(), e._stream()))
            dl = b["deliv"][1] - b["deliv"][0]
            sc = w[0] * out[3][0].to(torch.int64) + w[1 + out[0][0].to(torch.int64)] * dl
            b["ret"] = torch.where(out[5][0] != 0, torch.zeros_like(sc), b["ret"] + sc)
            if keep_rows:
                b["rows"][6][k] = dl
                out[3][0].copy_(sc)

    def unfused(fn):
        def run():
            os.environ["GW_ROLLOUT_POLICY_UNFUSED"] = "1"
            try:
                fn()
            finally:
                del os.environ["GW_ROLLOUT_POLICY_UNFUSED"]
        return run

    legs = {"P1": lambda: population("P1", True), "P0": lambda: population("P0", False), "P2": unfused(lambda: population("P2", True)),
            "P3": lambda: composed("P3", False),
            "R1": lambda: records("R1", True), "R0": lambda: records("R0", False), "R2": unfused(lambda: records("R2", True)),
            "R3": lambda: composed("R3", True)}
    times = {name: [] for name in legs}
    for rnd in range(args.repeats + 1):                        # round 0: warm-up (first launches, allocator)
        for name, fn in legs.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(W):                                 # W calls of K steps per timing
                fn()
                step0[name] += K
            torch.cuda.synchronize(dev)
            if rnd:
                times[name].append((time.perf_counter() - t0) / (K * W) * 1e6)
    for e in envs.values():
        e.check()
    res = {"label": args.label, "envs": N, "devices": D, "steps": K, "windows": W, "episodes": T, "policies": P, "rounds": args.repeats,
           "device": torch.cuda.get_device_name(0)}
    for name, t in times.items():
        res[name] = {"us_per_step_median": round(float(np.median(t)), 3), "min": round(min(t), 3), "max": round(max(t), 3)}
    med = {k: v["us_per_step_median"] for k, v in res.items() if isinstance(v, dict)}
    res["ratios"] = {"P1/P0": round(med["P1"] / med["P0"], 3), "P2/P1": round(med["P2"] / med["P1"], 3), "P3/P1": round(med["P3"] / med["P1"], 3),
                     "R1/R0": round(med["R1"] / med["R0"], 3), "R2/R1": round(med["R2"] / med["R1"], 3), "R3/R1": round(med["R3"] / med["R1"], 3)}
    print(json.dumps(res))


def packets_legs(args):
    """--packets (profiles/rollout_stats_delivered/README.md): episodes of T steps (--episodes, default 8), the tally with the
    packets a step delivered; the legs alternate in one process, --repeats rounds each, wall time per step over --windows calls
    of K steps:
      D1 env.rollout_episodes_stats(packets=True)   the eight-column table inside the launch
      D0 env.rollout_episodes_stats()               its parent on the same build: what the eighth column costs
      D2 the composition a caller has without it    rollout_episodes(score=neutral) into [K][N] rows, then the eight columns
                                                    with torch index_add_ (scatter-add) on the same stream
    D1 and D2 must build the same table from the same steps (checked once, before the timing, on two fresh handles)."""
    import torch
    from gymwipe_amd import VecCounterTrafficEnv, actions

    N, D, K, T, W = args.envs, args.devices, args.steps, args.episodes or 8, args.windows
    dev = torch.device("cuda:0")
    md = 20
    A = D * md
    rng = np.random.default_rng(7)
    p = rng.dirichlet(np.full(A, 0.3), size=3)
    if args.onehot:                                            # three non-empty bins instead of 3 * A: next to no flush
        p = np.zeros((3, A))
        p[:, 1 * md + md - 1] = 1.0
    cdf = actions.policy_cdf(p)
    neutral = actions.make_score(D)
    kinds = (torch.int32, torch.int32, torch.int32, torch.float32, torch.uint8, torch.uint8, torch.int32)
    center = 65536

    def new_env(cols):
        e = VecCounterTrafficEnv(N, num_devices=D, device=dev)
        e.reset()
        e.bench = {"cdf": e._policy_table(cdf), "table": torch.zeros((3, A, cols), dtype=torch.int64, device=dev), "step0": 0,
                   "rows": tuple(torch.empty((K, N), dtype=t, device=dev) for t in kinds)}
        return e

    def fused(e, packets):
        b = e.bench
        e.rollout_episodes_stats(b["cdf"], K, 5, max_steps=T, step0=b["step0"], table=b["table"], **({"packets": True} if packets else {}))
        b["step0"] += K

    def composed(e):
        b = e.bench
        first = e._last[0].clone()
        d, u, obs, rew, done, ended, dl = e.rollout_episodes(b["cdf"], K, 5, max_steps=T, step0=b["step0"], out=b["rows"], score=neutral)
        b["step0"] += K
        seen = torch.cat([first.unsqueeze(0), torch.where(ended[:-1] != 0, torch.full_like(obs[:-1], center), obs[:-1])])
        row = ((torch.sign(seen - center) + 1).to(torch.int64) * A + d.to(torch.int64) * md + u.to(torch.int64)).reshape(-1)
        r = rew.reshape(-1).to(torch.int64)
        col = (torch.sign(obs - center) + 1).reshape(-1).to(torch.int64)
        flat = b["table"].view(3 * A, 8)
        flat[:, 0].index_add_(0, row, torch.ones_like(row))
        flat[:, 1].index_add_(0, row, r)
        flat[:, 2].index_add_(0, row, r * r)
        flat.view(-1).index_add_(0, row * 8 + 3 + col, torch.ones_like(row))
        flat[:, 6].index_add_(0, row, (done.reshape(-1) != 0).to(torch.int64))
        flat[:, 7].index_add_(0, row, dl.reshape(-1).to(torch.int64).clamp(0, 65535))

    a, b = new_env(8), new_env(8)
    for _ in range(2):
        fused(a, True)
        composed(b)
    assert torch.equal(a.bench["table"], b.bench["table"]) and int(a.bench["table"][..., 0].sum()) == 2 * N * K, "D1 and D2 differ"
    assert int(a.bench["table"][..., 7].sum()) > 0
    del a, b
    envs = {"D1": new_env(8), "D0": new_env(7), "D2": new_env(8)}
    legs = {"D1": lambda: fused(envs["D1"], True), "D0": lambda: fused(envs["D0"], False), "D2": lambda: composed(envs["D2"])}
    times = {name: [] for name in legs}
    for rnd in range(args.repeats + 1):                        # round 0: warm-up (first launches, allocator)
        for name in (list(legs) if rnd % 2 else list(reversed(legs))):      # (a leg's place in the round alternates)
            fn = legs[name]
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(W):
                fn()
            torch.cuda.synchronize(dev)
            if rnd:
                times[name].append((time.perf_counter() - t0) / (K * W) * 1e6)
    for e in envs.values():
        e.check()
    res = {"label": args.label, "envs": N, "devices": D, "steps": K, "windows": W, "episodes": T, "rounds": args.repeats,
           "onehot": bool(args.onehot), "device": torch.cuda.get_device_name(0)}
    for name, t in times.items():
        res[name] = {"us_per_step_median": round(float(np.median(t)), 3), "min": round(min(t), 3), "max": round(max(t), 3)}
    res["ratios"] = {"D1/D0": round(res["D1"]["us_per_step_median"] / res["D0"]["us_per_step_median"], 3),
                     "D2/D1": round(res["D2"]["us_per_step_median"] / res["D1"]["us_per_step_median"], 3)}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--devices", type=int, default=4)
    ap.add_argument("--steps", type=int, default=64, help="steps per window (K)")
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--forms", default="a,b,c")
    ap.add_argument("--label", default="")
    ap.add_argument("--episodes", type=int, default=0, help="episode length T of the forms p, e, q, f (must divide --steps)")
    ap.add_argument("--scored", action="store_true", help="run the scored legs instead of --forms")
    ap.add_argument("--policies", type=int, default=64, help="P of the scored population legs")
    ap.add_argument("--packets", action="store_true", help="run the delivered-tally legs instead of --forms")
    ap.add_argument("--onehot", action="store_true",
                    help="--packets: a policy that always takes one action, so that a block's histogram has one bin per class to flush")
    args = ap.parse_args()
    if args.scored:
        return scored_legs(args)
    if args.packets:
        return packets_legs(args)

    import torch
    from gymwipe_amd import VecCounterTrafficEnv, actions
    from gymwipe_amd import _native as nat

    N, D, K, W = args.envs, args.devices, args.steps, args.windows
    dev = torch.device("cuda:0")
    env = VecCounterTrafficEnv(N, num_devices=D, device=dev)
    md = int(env.config.max_duration)
    A = D * md
    center = int(env.config.counter_bound)
    rng = np.random.default_rng(7)
    p = rng.dirichlet(np.full(A, 0.3), size=3)
    cdf = actions.policy_cdf(p) if hasattr(actions, "policy_cdf") else \
        np.minimum(np.floor(np.cumsum(p, axis=1) * 2.0 ** 32), 2.0 ** 32 - 1).astype(np.uint32)
    cdf[:, -1] = 0xffffffff
    table32 = torch.from_numpy(cdf.view(np.int32)).to(dev)
    # form b's table: the three rows as one sorted int64 vector (row r offset by r << 32), one searchsorted per step
    flat = (torch.from_numpy(cdf.astype(np.int64)).to(dev) + (torch.arange(3, device=dev)[:, None] << 32)).reshape(-1).contiguous()
    a_dev, a_dur = actions.actions_torch(3, 0, N, 0, K, D, md, device=dev)
    out3 = (torch.empty((K, N), dtype=torch.int32, device=dev), torch.empty((K, N), dtype=torch.float32, device=dev),
            torch.empty((K, N), dtype=torch.uint8, device=dev))
    out5 = (torch.empty((K, N), dtype=torch.int32, device=dev), torch.empty((K, N), dtype=torch.int32, device=dev)) + out3
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)

    def form_a():
        for _ in range(W):
            env.reset()
            env.rollout(a_dev, a_dur, out=out3)

    def form_b():
        for _ in range(W):
            obs = env.reset()
            for _k in range(K):
                cls = (torch.sign(obs - center) + 1).to(torch.int64)
                u = torch.randint(0, 0xffffffff, (N,), device=dev, generator=gen)
                a = torch.searchsorted(flat, u + (cls << 32), right=True) - cls * A
                a = torch.clamp(a, max=A - 1)
                d = torch.div(a, md, rounding_mode="floor")
                obs, _, _, _ = env.step({"device": d.to(torch.int32), "duration": (a - d * md).to(torch.int32)})

    def form_c():
        s = 0
        for _ in range(W):
            env.reset()
            env.rollout_policy(table32, K, 5, step0=s, out=out5)
            s += K

    def torch_table(first, out, table):
        d, u, obs, rew, done = out
        seen = torch.cat([first.unsqueeze(0), obs[:-1]])
        row = ((torch.sign(seen - center) + 1).to(torch.int64) * A + d.to(torch.int64) * md + u.to(torch.int64)).reshape(-1)
        r = rew.reshape(-1).to(torch.int64)
        col = (torch.sign(obs - center) + 1).reshape(-1).to(torch.int64)
        flat = table.view(3 * A, 7)
        flat[:, 0] += torch.bincount(row, minlength=3 * A)
        flat[:, 1].index_add_(0, row, r)
        flat[:, 2].index_add_(0, row, r * r)
        flat.view(-1).index_add_(0, row * 7 + 3 + col, torch.ones_like(row))
        flat[:, 6].index_add_(0, row, (done.reshape(-1) != 0).to(torch.int64))

    stats = torch.zeros((3, A, 7), dtype=torch.int64, device=dev)

    def form_t(table=stats):
        s = 0
        for _ in range(W):
            first = env.reset().clone()
            torch_table(first, env.rollout_policy(table32, K, 5, step0=s, out=out5), table)
            s += K

    def form_r(table=stats):
        s = 0
        for _ in range(W):
            first = env.reset().clone()
            env.transition_stats(first, *env.rollout_policy(table32, K, 5, step0=s, out=out5), table=table)
            s += K

    def form_s(table=stats):
        s = 0
        for _ in range(W):
            env.reset()
            env.rollout_policy_stats(table32, K, 5, step0=s, table=table)
            s += K

    T = args.episodes
    out6 = out5 + (torch.empty((K, N), dtype=torch.uint8, device=dev),)
    rewards_of = {"c": out5[3], "p": out5[3], "e0": out6[3], "e": out6[3]}    # form -> the rewards its last window stored

    def form_e0():
        s = 0
        for _ in range(W):
            env.reset()
            env.rollout_episodes(table32, K, 5, max_steps=0, on_done=False, step0=s, out=out6)
            s += K

    def form_p():                                              # T steps, reset, T steps, ...: the parent's only way
        s = 0
        for _ in range(W):
            for k in range(0, K, T):
                env.reset()
                env.rollout_policy(table32, T, 5, step0=s, out=tuple(t[k:k + T] for t in out5))
                s += T

    def form_e():
        s = 0
        env.reset()
        for _ in range(W):
            env.rollout_episodes(table32, K, 5, max_steps=T, on_done=True, step0=s, out=out6)
            s += K

    def form_q(table=stats):
        s = 0
        for _ in range(W):
            for k in range(0, K, T):
                env.reset()
                env.rollout_policy_stats(table32, T, 5, step0=s, table=table)
                s += T

    def form_f(table=stats):
        s = 0
        env.reset()
        for _ in range(W):
            env.rollout_episodes_stats(table32, K, 5, max_steps=T, on_done=True, step0=s, table=table)
            s += K

    have_e = hasattr(nat.lib(), "gw_rollout_episodes") and hasattr(env, "rollout_episodes")
    if T:
        assert T > 0 and K % T == 0, "--episodes must divide --steps"
    if T and have_e and any(f in args.forms.split(",") for f in "peqf"):
        # the same trajectory both ways, each from a fresh handle (an env's clock and queues outlive reset()): the rewards of p
        # and e, the tables of q and f.  (Default configuration: done never fires, every episode ends by the step limit.)
        def fresh():
            return VecCounterTrafficEnv(N, num_devices=D, device=dev)
        env = fresh()
        form_p()
        rew_p = out5[3].double().sum().item()
        env = fresh()
        form_e()
        assert out6[3].double().sum().item() == rew_p and int((out6[5] != 0).sum()) == N * K // T, "p and e walk different steps"
        tq, tf = torch.zeros_like(stats), torch.zeros_like(stats)
        env = fresh()
        form_q(tq)
        env = fresh()
        form_f(tf)
        assert bool((tq == tf).all()) and int(tq[..., 0].sum()) == N * K * W, "q and f build different tables"
        env = fresh()
    have_c = hasattr(nat.lib(), "gw_rollout_policy") and hasattr(env, "rollout_policy")
    have_s = hasattr(nat.lib(), "gw_rollout_policy_stats") and hasattr(env, "rollout_policy_stats")
    forms = {"a": form_a, "b": form_b, "c": form_c if have_c else None, "t": form_t if have_c else None,
             "r": form_r if have_s else None, "s": form_s if have_s else None,
             "e0": form_e0 if have_e else None, "p": form_p if T and have_c else None, "e": form_e if T and have_e else None,
             "q": form_q if T and have_s else None, "f": form_f if T and have_e else None}
    for f in args.forms.split(","):                            # every stats form counts every transition (the forms do not walk
        if f in ("t", "r", "s") and forms[f] is not None:                #  the same steps: an env's clock and queues outlive reset())
            check = torch.zeros_like(stats)
            forms[f](check)
            assert int(check[..., 0].sum()) == int(check[..., 3:6].sum()) == N * K * W, f
    res = {"label": args.label, "tree": "GW_TREE" if os.environ.get("GW_TREE") else "own", "envs": N, "devices": D, "steps": K, "windows": W,
           "episodes": T,
           "repeats": args.repeats, "unfused_switch": bool(os.environ.get("GW_ROLLOUT_POLICY_UNFUSED")),
           "lib": os.path.basename(os.environ.get("GW_LIB") or "")}
    for name in args.forms.split(","):
        fn = forms[name]
        if fn is None:
            res[name] = None
            continue
        fn()                                                   # warm-up (first launches, allocator)
        torch.cuda.synchronize(dev)
        times = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            times.append(time.perf_counter() - t0)
        env.check()
        rate = [N * K * W / t / 1e9 for t in times]
        res[name] = {"G_env_steps_per_s_best": round(max(rate), 3), "median": round(float(np.median(rate)), 3),
                     "min": round(min(rate), 3), "us_per_step_best": round(min(times) / (K * W) * 1e6, 3)}
        if name in rewards_of:                                 # what the steps are worth: the share with a non-zero reward
            res[name]["nonzero_reward_share"] = round(float((rewards_of[name] != 0).float().mean()), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
