#!/usr/bin/env python3
"""What a population of TD3 learners (learner.TD3Population: P members, six launches per update whatever P is) costs next to what the same P
learners cost as separate learner.TD3Learner objects driven one after another (6 P launches per update) -- scripts/pop_bench.py for TD3, at the
default TD3Config (policy_delay 2).  At N environments and minibatch B, for each P:
  (a) one update of all P members: population vs the P separate learners updated in turn
  (b) one step of the whole loop (act -> env.step -> push -> update): population vs the P separate learners on their slices of the same env
  (c) P = 1: the population against a single TD3Learner, with the single learner's own round-to-round spread
Both sides are timed in windows of 20 calls with a synchronisation at both ends, in three interleaved rounds in one process; medians are reported.
Writes profiles/learner/td3_pop_bench.json and prints it as one JSON line.
   usage: python scripts/td3_pop_bench.py [--n 4096] [--batch 100] [--pop 1 4 16] [--steps 200] [--warmup 20] [--trace-updates P]
--trace-updates P fills the replay and runs 20 updates of a population of P and nothing else (for a kernel trace run of its own, without counters: rocprofv3 --kernel-trace --stats -- python ...)."""
import argparse
import gc
import json
import os
import sys

from _timing import timed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
CAPACITY = 1 << 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--pop", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--trace-updates", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "learner", "td3_pop_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import rl_mpc_lanemerging_amd as pkg
    if pkg.build.needs_build():
        raise SystemExit("build the library first (__graft_entry__.build())")
    from rl_mpc_lanemerging_amd import _capi, learner, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    ctx = _capi.default_context()
    env = vec_env.MergeVecEnv(args.n, seed=1, ctx=ctx)
    cfg = learner.TD3Config(n_obs=env.obs_dim, batch=args.batch, capacity=CAPACITY, replay_start=0)
    result = {"learner": "TD3", "policy_delay": cfg.policy_delay, "n": args.n, "batch": args.batch, "steps": args.steps, "capacity": CAPACITY, "backend": _capi.backend_info(), "populations": {}}
    for P in ([args.trace_updates] if args.trace_updates else args.pop):
        n = args.n // P
        assert n * P == args.n, "--n must be a multiple of every --pop"
        sl = [slice(m * n, (m + 1) * n) for m in range(P)]
        pop = learner.TD3Population(env, (cfg, P), seeds=list(range(1, P + 1)))
        lone = [] if args.trace_updates else [learner.TD3Learner(env, cfg, seed=m + 1) for m in range(P)]
        state = {"obs": env.reset()}

        def step_pop(update=True):
            obs = state["obs"]
            ticks = env.episode_ticks.clone()
            a = pop.act(obs, ticks, noise=True)
            nobs, r, term, trunc, info = env.step(a)
            pop.push(obs, ticks, a, r, nobs, term, trunc, final_obs=info["final_observation"])
            if update:
                pop.update(1)
            state["obs"] = nobs

        def step_lone(update=True):
            obs = state["obs"]
            ticks = env.episode_ticks.clone()
            a = torch.cat([L.act(obs[s], ticks[s], noise=True) for L, s in zip(lone, sl)])
            nobs, r, term, trunc, info = env.step(a)
            fin = info["final_observation"]
            for L, s in zip(lone, sl):
                L.push(obs[s], ticks[s], a[s], r[s], nobs[s], term[s], trunc[s], final_obs=fin[s])
                if update:
                    L.update(1)
            state["obs"] = nobs

        def update_lone():
            for L in lone:
                L.update(1)
        for _ in range(10):                                         # fill: 10 n transitions per member, both sides
            step_pop(update=False)
            if lone:
                step_lone(update=False)
        torch.cuda.synchronize()
        if args.trace_updates:
            pop.update(20)
            torch.cuda.synchronize()
            print(json.dumps({"trace_updates": 20, "P": P, "updates": pop.stats()["updates"].tolist()}))
            return
        rounds = {"pop_update": [], "lone_update": [], "pop_loop": [], "lone_loop": []}
        for _ in range(3):                                          # interleaved rounds in one process
            rounds["pop_update"].append(timed(lambda: pop.update(1), args.steps, args.warmup, torch))
            rounds["lone_update"].append(timed(update_lone, args.steps, args.warmup, torch))
            rounds["pop_loop"].append(timed(step_pop, args.steps, args.warmup, torch))
            rounds["lone_loop"].append(timed(step_lone, args.steps, args.warmup, torch))
        env.drain_episode_stats()
        env.check_error()
        med = {k: float(np.median(v)) for k, v in rounds.items()}
        result["populations"][str(P)] = {
            "n_per_member": n,
            "pop_update_us": med["pop_update"] * 1e6, "separate_updates_us": med["lone_update"] * 1e6, "update_speedup": med["lone_update"] / med["pop_update"],
            "pop_update_us_per_member": med["pop_update"] * 1e6 / P,
            "pop_loop_step_us": med["pop_loop"] * 1e6, "separate_loop_step_us": med["lone_loop"] * 1e6, "loop_speedup": med["lone_loop"] / med["pop_loop"],
            "pop_loop_frames_per_s": args.n / med["pop_loop"], "separate_loop_frames_per_s": args.n / med["lone_loop"],
            "rounds_us": {k: [x * 1e6 for x in v] for k, v in rounds.items()},
            "updates_done": {"population": pop.stats()["updates"].tolist(), "separate": [L.stats()["updates"] for L in lone]}}
        if P == 1:                                                  # (c): the difference next to the single learner's own spread
            lo, hi = min(rounds["lone_update"]), max(rounds["lone_update"])
            result["p1_vs_single"] = {"pop_update_us": med["pop_update"] * 1e6, "single_update_us": med["lone_update"] * 1e6,
                                      "difference_us": (med["pop_update"] - med["lone_update"]) * 1e6, "single_round_spread_us": (hi - lo) * 1e6,
                                      "single_rounds_us": [x * 1e6 for x in rounds["lone_update"]], "pop_rounds_us": [x * 1e6 for x in rounds["pop_update"]],
                                      "pop_loop_step_us": med["pop_loop"] * 1e6, "single_loop_step_us": med["lone_loop"] * 1e6}
        del pop, lone
        gc.collect()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
