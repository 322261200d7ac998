#!/usr/bin/env python3
"""What a population of C51 learners (learner.C51Population: P members, three launches per update whatever P is) costs next to what the same P
learners cost as separate learner.C51Learner objects driven one after another (3 P launches per update) -- scripts/dqn_pop_bench.py for the
categorical head, on sumo-jerk-v0 at the shipped network (20-256-5 x 51 atoms) and minibatch (B = 50).  At N environments, for each P:
  (a) one update of all P members: population vs the P separate learners updated in turn, as updates per second (member updates: P per call)
  (b) P = 1: the population against a single C51Learner, with the single learner's own round-to-round spread
Both sides live in one process and are filled from the same env steps (each lone learner gets its member's slice), so their rings hold the same
rows.  Both are timed in windows of 20 calls with a synchronisation at both ends, in three interleaved rounds; medians are reported.  No ratio is
asserted anywhere: the file says what was measured.
Writes profiles/learner/c51_pop_bench.json and prints it as one JSON line.
   usage: python scripts/c51_pop_bench.py [--n 4096] [--batch 50] [--pop 1 4 16] [--steps 200] [--warmup 20]"""
import argparse
import gc
import json
import os
import sys

from _timing import timed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
CAPACITY = 1 << 16
EPS = 0.1                                                           # the reference's EPS_END: every acting call explores


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--pop", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "learner", "c51_pop_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import rl_mpc_lanemerging_amd as pkg
    if pkg.build.needs_build():
        raise SystemExit("build the library first (__graft_entry__.build())")
    from rl_mpc_lanemerging_amd import _capi, learner, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    ctx = _capi.default_context()
    env = vec_env.MergeVecEnv(args.n, env_id="sumo-jerk-v0", seed=1, ctx=ctx)
    cfg = learner.C51Config(n_obs=env.obs_dim, batch=args.batch, capacity=CAPACITY, replay_start=0)
    result = {"learner": "C51", "env_id": "sumo-jerk-v0", "net": [cfg.n_obs, cfg.h1, int(env.action_space["n"])], "n_atoms": cfg.n_atoms,
              "support": [cfg.v_min, cfg.v_max], "eps": EPS, "n": args.n, "batch": args.batch, "steps": args.steps, "capacity": CAPACITY,
              "launches_per_update": {"population": 3, "separate": "3 P"}, "backend": _capi.backend_info(), "populations": {}}
    for P in args.pop:
        n = args.n // P
        assert n * P == args.n, "--n must be a multiple of every --pop"
        sl = [slice(m * n, (m + 1) * n) for m in range(P)]
        pop = learner.C51Population(env, (cfg, P), seeds=list(range(1, P + 1)))
        lone = [learner.C51Learner(env, cfg, seed=m + 1) for m in range(P)]
        obs = env.reset()
        for _ in range(10):                                         # fill: 10 n transitions per member, the same rows on both sides
            a = pop.act(obs, None, eps=EPS)
            nobs, r, term, trunc, info = env.step(a)
            fin = info["final_observation"]
            pop.push(obs, None, a, r, nobs, term, trunc, final_obs=fin)
            for L, s in zip(lone, sl):
                L.push(obs[s], None, a[s], r[s], nobs[s], term[s], trunc[s], final_obs=fin[s])
            obs = nobs
        torch.cuda.synchronize()

        def update_lone():
            for L in lone:
                L.update(1)
        rounds = {"pop_update": [], "lone_update": []}
        for _ in range(3):                                          # interleaved rounds in one process
            rounds["pop_update"].append(timed(lambda: pop.update(1), args.steps, args.warmup, torch))
            rounds["lone_update"].append(timed(update_lone, args.steps, args.warmup, torch))
        env.drain_episode_stats()
        env.check_error()
        ctx.check_error()
        med = {k: float(np.median(v)) for k, v in rounds.items()}
        result["populations"][str(P)] = {
            "n_per_member": n,
            "pop_update_us": med["pop_update"] * 1e6, "separate_updates_us": med["lone_update"] * 1e6, "update_speedup": med["lone_update"] / med["pop_update"],
            "pop_update_us_per_member": med["pop_update"] * 1e6 / P, "separate_update_us_per_member": med["lone_update"] * 1e6 / P,
            "pop_member_updates_per_s": P / med["pop_update"], "separate_member_updates_per_s": P / med["lone_update"],
            "rounds_us": {k: [x * 1e6 for x in v] for k, v in rounds.items()},
            "updates_done": {"population": pop.stats()["updates"].tolist(), "separate": [L.stats()["updates"] for L in lone]}}
        if P == 1:                                                  # (b): the difference next to the single learner's own spread
            lo, hi = min(rounds["lone_update"]), max(rounds["lone_update"])
            result["p1_vs_single"] = {"pop_update_us": med["pop_update"] * 1e6, "single_update_us": med["lone_update"] * 1e6,
                                      "difference_us": (med["pop_update"] - med["lone_update"]) * 1e6, "single_round_spread_us": (hi - lo) * 1e6,
                                      "within_single_spread": bool(abs(med["pop_update"] - med["lone_update"]) <= hi - lo),
                                      "single_rounds_us": [x * 1e6 for x in rounds["lone_update"]], "pop_rounds_us": [x * 1e6 for x in rounds["pop_update"]]}
        del pop, lone
        gc.collect()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
