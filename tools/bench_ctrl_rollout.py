#!/usr/bin/env python3
"""
The control loop's fused rollout beside what it replaces (profiles/ctrl_rollout/README.md).

VecControlLoopEnv, N envs, calls of K = 64 steps, every env with an initial angle of its own.  Up to twenty-five legs in ONE process,
alternated call by call so that clock and thermal drift hit all alike, each leg on a handle of its own:
  a   K x env.step                                      the only form there was; ctrl_step_kernel is unchanged
  b   env.rollout, no episodes                          the same actions in one launch
  c   env.rollout with episodes                         max_steps / fail_deg, ended rows written
  cs  per step: env.step, the rule in torch,            what c replaces: the bookkeeping on the device, one host read per step
      env.reset_envs(mask)                              (does any env end?) as a caller would write it
  cn  the same without the host read                    reset_envs(mask) issued every step, no synchronise
  d   env.reset_envs + env.rollout_schedules            P schedules, no [K][N] array at all, a per-env tally
  dc  env.reset_envs + env.rollout with episodes        fed d's schedules expanded to [K][N] actions along every env's own ages
                                                        (found once, before the timing, by a per-step composition): the same
                                                        trajectory, which is why both legs restart their envs in every call
  f   env.rollout_feedback, no rows                     P angle-feedback policies of --bins bins (profiles/ctrl_feedback/README.md)
  fn  per step: torch searchsorted (bucketize per       what f replaces, without a host read: the bin from the observation, the
      policy) + gather, env.step, the rule in torch,    action gathered from the policies, reset_envs(mask) issued every step
      env.reset_envs(mask)
  f1  env.reset_envs + env.rollout_feedback, no rows    fed d's schedules as policies of ONE bin: d's trajectory, so f1/d is what
                                                        the feedback kernel costs beyond the schedule kernel when it has nothing to decide
  cg, dg, fg   legs c, d and f on a handle on which      what the switch to the PID instantiations of the kernels costs
      env.set_gains((1, 0, 0)) has been called          (profiles/ctrl_gains/README.md): the same trajectory, per-env gains read
  cz, dz, fz   legs cg, dg and fg on a handle on which     what the switch to the disturbance instantiations costs
      env.set_disturbance(0) has been called as well    (profiles/ctrl_disturbance/README.md): the same trajectory, one draw per substep
  cw, dw, fw   the same with weights --noise on x[3]     a trajectory of their own: the disturbed plant, every env its own key
  cl, dl, fl   legs cz, dz and fz on a handle on which     what the switch to the loss instantiations costs
      env.set_loss(0) has been called as well           (profiles/ctrl_loss/README.md): the same trajectory, one draw per transmission
  cp, dp, fp   the same with probability --loss on all    a trajectory of their own: packets and announcements erased, every env
      four links                                        its own key
A timed unit is one call of K steps between two HIP events and two wall-clock reads, the second after a synchronise; units are
repeated until every leg has at least `--seconds` of stream time and at least `--min-repeats` units.  Before the timing, b's
outputs are checked against a's, c's `ended` against cs's, d's tally against dc's `ended`, f's state against fn's, f1's
tally against d's, cg's, dg's and fg's state against c's, d's and f's, cz's, dz's and fz's against cg's, dg's and fg's, and cl's,
dl's and fl's against cz's, dz's and fz's, each pair from one state.
Reported per leg: median, min and max of the wall-clock and event microseconds per step; the ratios of the wall-clock medians;
and the run-to-run spread of leg a ((max - min) / median), against which b/a is to be read.  One JSON line; --out appends it to
a file.
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
    ap.add_argument("--envs", type=int, default=32768)
    ap.add_argument("--steps", type=int, default=64, help="K: steps per call")
    ap.add_argument("--schedules", type=int, default=64, help="P of legs d and dc")
    ap.add_argument("--length", type=int, default=8, help="L of the schedules")
    ap.add_argument("--max-steps", type=int, default=25)
    ap.add_argument("--fail-deg", type=float, default=90.0)
    ap.add_argument("--seconds", type=float, default=0.25, help="stream time per leg at least")
    ap.add_argument("--min-repeats", type=int, default=5)
    ap.add_argument("--bins", type=int, default=3, help="B of legs f and fn")
    ap.add_argument("--noise", type=float, default=0.01, help="the weight on x[3] of legs cw, dw and fw")
    ap.add_argument("--loss", type=float, default=0.25, help="the loss probability on every link of legs cp, dp and fp")
    ap.add_argument("--legs", default="a,b,c,cs,cn,d,dc,f,fn,f1,cg,dg,fg,cz,dz,fz,cw,dw,fw,cl,dl,fl,cp,dp,fp")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    from gymwipe_amd import VecControlLoopEnv, actions

    if not torch.cuda.is_available():
        sys.exit("bench_ctrl_rollout needs a GPU: a timing taken anywhere else says nothing")
    N, K, P, L = args.envs, args.steps, args.schedules, args.length
    dev = torch.device("cuda:0")
    episodes = (args.max_steps, args.fail_deg)
    rng = np.random.default_rng(0)
    a_dev = torch.from_numpy(rng.integers(0, 2, (K, N)).astype(np.int32)).to(dev)
    a_dur = torch.from_numpy(rng.integers(0, 20, (K, N)).astype(np.int32)).to(dev)
    x0 = np.zeros((N, 4))
    x0[:, 2] = rng.uniform(-1.5, 1.5, N)                                # an initial angle of its own for every env
    x0[:, 3] = rng.uniform(-1.0, 1.0, N)
    sched_np = actions.make_ctrl_schedules([list(zip(rng.integers(0, 2, L).tolist(), rng.integers(0, 20, L).tolist()))
                                            for _ in range(P)], L)
    sched = torch.from_numpy(sched_np).to(dev)
    p_of = torch.arange(N, device=dev) // (N // P)
    B = args.bins
    fb_np = actions.make_ctrl_feedback([[list(zip(rng.integers(0, 2, L).tolist(), rng.integers(0, 20, L).tolist())) for _ in range(B)]
                                        for _ in range(P)], [sorted(rng.choice(90, B - 1, replace=False).tolist()) for _ in range(P)], L)
    fb_sched, fb_edges = torch.from_numpy(fb_np[0]).to(dev), torch.from_numpy(fb_np[1]).to(dev)     # keys |o|, sorted edges in [0, 90)
    one_bin, no_edges = sched[:, None].contiguous(), torch.empty((P, 0), dtype=torch.int32, device=dev)
    x_dev = torch.empty((K, N), dtype=torch.int32, device=dev)         # d's schedules expanded: filled in below
    x_dur = torch.empty((K, N), dtype=torch.int32, device=dev)

    def new_env(gains=None, noise=None, loss=None):
        env = VecControlLoopEnv(N, device=dev, gains=gains)
        env.set_initial_state(torch.from_numpy(x0))
        env.reset_envs()
        if noise is not None:
            env.set_disturbance((0.0, 0.0, 0.0, noise))                 # default keys: a sequence of its own for every env
        if loss is not None:
            env.set_loss((loss,) * 4)                                   # default keys, as above
        return env

    names = [x for x in args.legs.split(",") if x]
    SWITCHED = {"cg": None, "dg": None, "fg": None, "cz": 0.0, "dz": 0.0, "fz": 0.0, "cw": args.noise, "dw": args.noise, "fw": args.noise}
    LOSSY = {"cl": 0.0, "dl": 0.0, "fl": 0.0, "cp": args.loss, "dp": args.loss, "fp": args.loss}     # on a handle as cz's, dz's, fz's
    envs = {n: new_env((1.0, 0.0, 0.0), 0.0, LOSSY[n]) if n in LOSSY else new_env((1.0, 0.0, 0.0), SWITCHED[n]) if n in SWITCHED else new_env()
            for n in names}
    out = (torch.empty((K, N), dtype=torch.int32, device=dev), torch.empty((K, N), dtype=torch.float32, device=dev),
           torch.empty((K, N), dtype=torch.uint8, device=dev), torch.empty((K, N), dtype=torch.float64, device=dev))
    age = {n: torch.zeros(N, dtype=torch.int32, device=dev) for n in ("cs", "cn")}
    cost = {n: torch.zeros(N, dtype=torch.float64, device=dev) for n in ("cs", "cn")}
    ended_rows = torch.empty((K, N), dtype=torch.uint8, device=dev)

    def leg_a(env):
        for k in range(K):
            env.step({"device": a_dev[k], "duration": a_dur[k]})

    def leg_b(env):
        env.rollout(a_dev, a_dur, out=out)

    def leg_c(env):
        env.rollout(a_dev, a_dur, episodes=episodes, out=out)

    def composed(n, read):
        def leg(env):
            ag, co = age[n], cost[n]
            for k in range(K):
                _, _, _, info = env.step({"device": a_dev[k], "duration": a_dur[k]})
                mag = info["Sensor angle"].abs()
                ag += 1
                co += mag
                cause = (ag == args.max_steps).to(torch.uint8) | ((mag > args.fail_deg).to(torch.uint8) << 1)
                ended_rows[k] = cause
                if not read or bool(cause.any()):
                    env.reset_envs(cause)
                    gone = cause != 0
                    ag.masked_fill_(gone, 0)
                    co.masked_fill_(gone, 0.0)
        return leg

    tally = {}

    def leg_d(env):
        env.reset_envs()
        tally["d"] = env.rollout_schedules(sched, episodes, K)[0]

    def leg_dc(env):
        env.reset_envs()
        env.rollout(x_dev, x_dur, episodes=episodes, out=out)

    def expand_schedules():
        """x_dev / x_dur <- the action every env takes at each of K steps from a reset, under its schedule and the episode rule."""
        env = new_env()
        ag = torch.zeros(N, dtype=torch.int64, device=dev)
        for k in range(K):
            row = sched[p_of, ag % L].to(torch.int32)
            x_dev[k], x_dur[k] = row[:, 0].clamp(max=1), row[:, 1].clamp(max=19)
            _, _, _, info = env.step({"device": x_dev[k], "duration": x_dur[k]})
            mag = info["Sensor angle"].abs()
            ag += 1
            gone = (ag == args.max_steps) | (mag > args.fail_deg)
            env.reset_envs(gone)
            ag.masked_fill_(gone, 0)
        env.close()

    def leg_f(env):
        tally["f"] = env.rollout_feedback(fb_sched, fb_edges, episodes, K)[0]

    fn_age = torch.zeros(N, dtype=torch.int64, device=dev)
    fn_obs = []

    def leg_fn(env):
        if not fn_obs:
            fn_obs.append(env.reset_envs(torch.zeros(N, dtype=torch.uint8, device=dev)))    # resets nothing: the observations
        obs, ag = fn_obs[0], fn_age
        for k in range(K):
            key = obs.abs()
            b = torch.searchsorted(fb_edges[p_of], key[:, None], right=True)[:, 0] if B > 1 else torch.zeros_like(ag)
            row = fb_sched[p_of, b, ag % L].to(torch.int32)
            _, _, _, info = env.step({"device": row[:, 0].clamp(max=1), "duration": row[:, 1].clamp(max=19)})
            mag = info["Sensor angle"].abs()
            ag += 1
            cause = (ag == args.max_steps).to(torch.uint8) | ((mag > args.fail_deg).to(torch.uint8) << 1)
            obs = env.reset_envs(cause)
            ag.masked_fill_(cause != 0, 0)

    def leg_f1(env):
        env.reset_envs()
        tally["f1"] = env.rollout_feedback(one_bin, no_edges, episodes, K)[0]

    def leg_dg(env):
        env.reset_envs()
        tally["dg"] = env.rollout_schedules(sched, episodes, K)[0]

    def leg_fg(env):
        tally["fg"] = env.rollout_feedback(fb_sched, fb_edges, episodes, K)[0]

    def tallied(n, leg):                                                # legs dg and fg under another name
        def run(env):
            leg(env)
            tally[n] = tally.pop(leg.__name__[4:])
        return run

    legs = {"cl": leg_c, "cp": leg_c, "dl": tallied("dl", leg_dg), "dp": tallied("dp", leg_dg), "fl": tallied("fl", leg_fg),
            "fp": tallied("fp", leg_fg), "cz": leg_c, "cw": leg_c, "dz": tallied("dz", leg_dg), "dw": tallied("dw", leg_dg), "fz": tallied("fz", leg_fg),
            "fw": tallied("fw", leg_fg), "cg": leg_c, "dg": leg_dg, "fg": leg_fg, "f": leg_f, "fn": leg_fn, "f1": leg_f1, "a": leg_a, "b": leg_b, "c": leg_c, "cs": composed("cs", True), "cn": composed("cn", False), "d": leg_d, "dc": leg_dc}

    # the legs mean what they say: from one state b gives a's last rows, and c ends the envs its composition ends
    if "a" in names and "b" in names:
        leg_a(envs["a"])
        leg_b(envs["b"])
        assert torch.equal(envs["a"]._obs, out[0][-1]) and torch.equal(envs["a"]._angle, out[3][-1]), "rollout differs from K steps"
    if "c" in names and "cs" in names:
        leg_c(envs["c"])
        want = out[2].clone()
        legs["cs"](envs["cs"])
        assert torch.equal(want, ended_rows) and bool(want.any()), "the composition ends other envs than the fused call"
    if "dc" in names:
        expand_schedules()
    if "d" in names and "dc" in names:
        leg_d(envs["d"])
        leg_dc(envs["dc"])
        ends = (out[2] != 0).sum(0).to(torch.float64)
        assert torch.equal(tally["d"][:, 0], ends) and bool(ends.any()), "the expanded actions end other envs than the schedules"
    if "f" in names and "fn" in names:
        leg_f(envs["f"])
        leg_fn(envs["fn"])
        for field in ("x", "now", "u", "n_tx"):
            assert (envs["f"].get_state(field) == envs["fn"].get_state(field)).all(), "the composition leaves another %s than the feedback call" % field
        assert (envs["f"].get_state("age") == fn_age.cpu().numpy()).all(), "the composition's episodes are not the feedback call's"
        assert bool((tally["f"][:, 0] > 0).any()) and bool((tally["f"][:, 7] > 0).any()) and bool((tally["f"][:, 7] < K).any())
    if "f1" in names and "d" in names:
        leg_d(envs["d"])
        leg_f1(envs["f1"])
        assert torch.equal(tally["f1"][:, :4], tally["d"]), "one bin does not give the schedule call's tally"
    for x, y in (("cg", "c"), ("dg", "d"), ("fg", "f")):                # the handle with gains (1, 0, 0) set walks the other's trajectory
        if x in names and y in names:
            for n in (x, y):
                envs[n].reset_envs()
                legs[n](envs[n])
            for field in ("x", "now", "u", "angle_deg", "n_tx", "commands", "age", "cost"):
                assert (envs[x].get_state(field) == envs[y].get_state(field)).all(), "leg %s leaves another %s than leg %s" % (x, field, y)
            assert (envs[x].get_state("last_error") != 0).any() and (envs[y].get_state("last_error") == 0).all()
            if x != "cg":
                assert torch.equal(tally[x], tally[y]), "leg %s tallies other episodes than leg %s" % (x, y)
    for x, y in (("cz", "cg"), ("dz", "dg"), ("fz", "fg")):             # zero weights on a switched handle walk the gains' trajectory
        if x in names and y in names:
            for n in (x, y):
                envs[n].reset_envs()
                legs[n](envs[n])
            for field in ("x", "now", "u", "angle_deg", "n_tx", "commands", "age", "cost", "last_error"):
                assert (envs[x].get_state(field) == envs[y].get_state(field)).all(), "leg %s leaves another %s than leg %s" % (x, field, y)
            assert (envs[x].get_state("noise_count") != 0).all() and (envs[y].get_state("noise_count") == 0).all()
            if x != "cz":
                assert torch.equal(tally[x], tally[y]), "leg %s tallies other episodes than leg %s" % (x, y)
    for x, y in (("cw", "cg"), ("dw", "dg"), ("fw", "fg")):             # ... and weights that are not zero leave it
        if x in names and y in names:
            for n in (x, y):
                envs[n].reset_envs()
                legs[n](envs[n])
            assert (envs[x].get_state("x") != envs[y].get_state("x")).any(), "leg %s is not disturbed" % x
    for x, y in (("cl", "cz"), ("dl", "dz"), ("fl", "fz")):             # zero thresholds on a switched handle walk the disturbance's trajectory
        if x in names and y in names:
            for n in (x, y):
                envs[n].reset_envs()
                legs[n](envs[n])
            for field in ("x", "now", "u", "angle_deg", "n_tx", "commands", "age", "cost", "last_error"):       # (the counts of draws
                # survive reset_envs and the legs have run different numbers of calls by now: they are not compared)
                assert (envs[x].get_state(field) == envs[y].get_state(field)).all(), "leg %s leaves another %s than leg %s" % (x, field, y)
            assert (envs[x].get_state("loss_count") != 0).all() and (envs[y].get_state("loss_count") == 0).all()
            assert (envs[x].get_state("lost") == 0).all()
            if x != "cl":
                assert torch.equal(tally[x], tally[y]), "leg %s tallies other episodes than leg %s" % (x, y)
    for x, y in (("cp", "cz"), ("dp", "dz"), ("fp", "fz")):             # ... and thresholds that are not zero leave it
        if x in names and y in names:
            for n in (x, y):
                envs[n].reset_envs()
                legs[n](envs[n])
            assert (envs[x].get_state("lost") != 0).any() and (envs[x].get_state("x") != envs[y].get_state("x")).any(), "leg %s loses nothing" % x
    for n in names:                                                     # warm-up: first launches, allocator, caches
        legs[n](envs[n])
    torch.cuda.synchronize(dev)
    wall = {n: [] for n in names}
    event = {n: [] for n in names}
    total = {n: 0.0 for n in names}
    while min(total.values()) < args.seconds or min(len(v) for v in wall.values()) < args.min_repeats:
        for n in names:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            e0.record()
            legs[n](envs[n])
            e1.record()
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            ms = e0.elapsed_time(e1)
            wall[n].append((t1 - t0) / K * 1e6)
            event[n].append(ms * 1e3 / K)
            total[n] += ms * 1e-3

    def summary(xs):
        return {"median": round(float(np.median(xs)), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}

    res = {"label": args.label, "gpu": torch.cuda.get_device_name(dev), "envs": N, "steps": K, "schedules": P, "length": L, "bins": B,
           "max_steps": args.max_steps, "fail_deg": args.fail_deg, "repeats": {n: len(wall[n]) for n in names}}
    for n in names:
        res[n] = {"wall_us_per_step": summary(wall[n]), "event_us_per_step": summary(event[n]), "stream_seconds": round(total[n], 3)}
    med = {n: res[n]["wall_us_per_step"]["median"] for n in names}
    res["ratios"] = {"%s/%s" % (x, y): round(med[x] / med[y], 3)
                     for x, y in (("b", "a"), ("c", "cs"), ("c", "cn"), ("c", "b"), ("d", "dc"), ("d", "c"), ("f", "fn"), ("f1", "d"), ("f", "c"), ("cg", "c"), ("dg", "d"), ("fg", "f"),
                                  ("cz", "cg"), ("dz", "dg"), ("fz", "fg"), ("cw", "cg"), ("dw", "dg"), ("fw", "fg"),
                                  ("cl", "cz"), ("dl", "dz"), ("fl", "fz"), ("cp", "cz"), ("dp", "dz"), ("fp", "fz")) if x in med and y in med}
    if "a" in names:
        w = res["a"]["wall_us_per_step"]
        res["spread_a"] = round((w["max"] - w["min"]) / w["median"], 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    for env in envs.values():
        env.close()


if __name__ == "__main__":
    main()
