#!/usr/bin/env python3
"""What a population of DQN learners (learner.DQNPopulation: P members, three launches per update whatever P is) costs next to what the same P
learners cost as separate learner.DQNLearner objects driven one after another (3 P launches per update) -- scripts/td3_pop_bench.py for DQN, on
sumo-jerk-v0 at the reference's own network (20-256-5) and minibatch (B = 50).  At N environments, for each P:
  (a) one update of all P members: population vs the P separate learners updated in turn
  (b) one step of the whole loop (act -> env.step -> push -> update): population vs the P separate learners on their slices of the same env
  (c) P = 1: the population against a single DQNLearner, with the single learner's own round-to-round spread
Both sides are timed in windows of 20 calls with a synchronisation at both ends, in three interleaved rounds in one process; medians are reported.
Writes profiles/learner/dqn_pop_bench.json and prints it as one JSON line.
   usage: python scripts/dqn_pop_bench.py [--n 4096] [--batch 50] [--pop 1 4 16] [--steps 200] [--warmup 20] [--trace-updates P]
          python scripts/dqn_pop_bench.py --summarize-trace DIR [DIR ...]
--trace-updates P fills the replay and runs 20 updates of a population of P and nothing else (for a kernel trace run of its own, without counters:
rocprofv3 --kernel-trace --stats -f csv -d DIR -o t -- python scripts/dqn_pop_bench.py --trace-updates P); --summarize-trace turns the kernel-stats
CSVs of such runs into the rows of profiles/learner/dqn_pop_kernel_stats.txt (no GPU needed)."""
import argparse
import csv
import gc
import glob
import json
import os
import sys

from _timing import timed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
CAPACITY = 1 << 16
EPS = 0.1                                                           # the reference's EPS_END: every acting call explores


def summarize_trace(directories, out):
    """One line per (run, kernel): calls, average, minimum and maximum duration in us.  The run's name is its directory's."""
    lines = ["# rocprofv3 --kernel-trace --stats -f csv -d <run> -o t -- python scripts/dqn_pop_bench.py --trace-updates P   (B = 50, 20-256-5, 10 fill steps, "
             "20 updates; no counters in these runs)", "%-10s %-24s %6s %10s %10s %10s" % ("run", "kernel", "calls", "avg_us", "min_us", "max_us")]
    for d in directories:
        paths = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not paths:
            raise SystemExit("no *kernel_stats.csv under %s" % d)
        rows = [r for r in csv.DictReader(open(paths[0])) if "stmpc::k_dqn" in r["Name"] or "stmpc::k_per" in r["Name"] or "stmpc::k_ddpg_stats" in r["Name"]]
        for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
            name = r["Name"].split("(")[0].replace("stmpc::", "").replace("void ", "")
            lines.append("%-10s %-24s %6d %10.1f %10.1f %10.1f" % (os.path.basename(os.path.normpath(d)), name, int(r["Calls"]), float(r["AverageNs"]) / 1e3,
                                                                   float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3))
    text = "\n".join(lines) + "\n"
    if out:
        with open(out, "w") as fh:
            fh.write(text)
    sys.stdout.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--pop", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--trace-updates", type=int, default=0)
    ap.add_argument("--summarize-trace", nargs="+", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "learner", "dqn_pop_bench.json"))
    ap.add_argument("--stats-out", default=os.path.join(REPO, "profiles", "learner", "dqn_pop_kernel_stats.txt"))
    args = ap.parse_args()
    if args.summarize_trace:
        return summarize_trace(args.summarize_trace, args.stats_out)
    import numpy as np
    import torch
    import rl_mpc_lanemerging_amd as pkg
    if pkg.build.needs_build():
        raise SystemExit("build the library first (__graft_entry__.build())")
    from rl_mpc_lanemerging_amd import _capi, learner, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    ctx = _capi.default_context()
    env = vec_env.MergeVecEnv(args.n, env_id="sumo-jerk-v0", seed=1, ctx=ctx)
    cfg = learner.DQNConfig(n_obs=env.obs_dim, batch=args.batch, capacity=CAPACITY, replay_start=0)
    result = {"learner": "DQN", "env_id": "sumo-jerk-v0", "net": [cfg.n_obs, cfg.h1, int(env.action_space["n"])], "eps": EPS, "n": args.n, "batch": args.batch,
              "steps": args.steps, "capacity": CAPACITY, "launches_per_update": {"population": 3, "separate": "3 P"}, "backend": _capi.backend_info(), "populations": {}}
    for P in ([args.trace_updates] if args.trace_updates else args.pop):
        n = args.n // P
        assert n * P == args.n, "--n must be a multiple of every --pop"
        sl = [slice(m * n, (m + 1) * n) for m in range(P)]
        pop = learner.DQNPopulation(env, (cfg, P), seeds=list(range(1, P + 1)))
        lone = [] if args.trace_updates else [learner.DQNLearner(env, cfg, seed=m + 1) for m in range(P)]
        state = {"obs": env.reset()}

        def step_pop(update=True):
            obs = state["obs"]
            a = pop.act(obs, None, eps=EPS)
            nobs, r, term, trunc, info = env.step(a)
            pop.push(obs, None, a, r, nobs, term, trunc, final_obs=info["final_observation"])
            if update:
                pop.update(1)
            state["obs"] = nobs

        def step_lone(update=True):
            obs = state["obs"]
            a = torch.cat([L.act(obs[s], None, eps=EPS) for L, s in zip(lone, sl)])
            nobs, r, term, trunc, info = env.step(a)
            fin = info["final_observation"]
            for L, s in zip(lone, sl):
                L.push(obs[s], None, a[s], r[s], nobs[s], term[s], trunc[s], final_obs=fin[s])
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
                                      "within_single_spread": bool(abs(med["pop_update"] - med["lone_update"]) <= hi - lo),
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
