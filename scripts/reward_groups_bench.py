#!/usr/bin/env python3
"""What reward groups (R groups of N / R environments, each rewarded under its own settings, in one MergeVecEnv: csrc/stmpc_env_groups_kernels.hpp)
cost and gain next to the paths that existed before them, at N = 4096 and R = 4 (the four reward functions):
  (a) one grouped MergeVecEnv.step of N environments
  (b) the same N as R lone envs of N / R (R contexts) stepped one after another: what the feature replaces
  (c) the ungrouped MergeVecEnv.step of the same N and seed -- the same world bit for bit: what the table costs
The three sides are timed in the same process on live worlds (autoreset on, episodes of the default length), interleaved, in five rounds (windows
of 20 calls with a synchronisation at both ends); medians and the spread over rounds are reported.  Writes profiles/env/reward_groups_bench.json
and prints it as one JSON line.
   usage: python scripts/reward_groups_bench.py [--n 4096] [--steps 200] [--warmup 20] [--rounds 5]"""
import argparse
import json
import os
import sys

from _timing import timed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
REWARDS = [{"REWARD_FUNCTION": "Continuous"}, {"REWARD_FUNCTION": "Slotted"}, {"REWARD_FUNCTION": "Slotted Jerk", "ALT_J_WEIGHT": 0.1},
           {"REWARD_FUNCTION": "ST"}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "env", "reward_groups_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import rl_mpc_lanemerging_amd as pkg
    if pkg.build.needs_build():
        raise SystemExit("build the library first (__graft_entry__.build())")
    from rl_mpc_lanemerging_amd import _capi, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    S = pkg.Settings
    dev = torch.device("cuda", torch.cuda.current_device())
    N, R = args.n, len(REWARDS)
    env_id = "sumo-jerk-continuous-v0"
    grouped = vec_env.MergeVecEnv(N, env_id=env_id, seed=1, rewards=REWARDS)
    plain = vec_env.MergeVecEnv(N, env_id=env_id, seed=1)
    lone = []
    for r, group in enumerate(REWARDS):
        snap = S.snapshot()
        pkg.apply_overrides(group)                                  # a lone env of this reward, the way it was made before groups
        lone.append(vec_env.MergeVecEnv(N // R, env_id=env_id, seed=1 + r))
        S.restore(snap)
    zero, zero_r = torch.zeros(N, dtype=torch.float64, device=dev), torch.zeros(N // R, dtype=torch.float64, device=dev)
    for e in [grouped, plain] + lone:
        e.reset()

    def lone_steps():
        for e in lone:
            e.step(zero_r)
    rounds = {"grouped": [], "lone": [], "plain": []}
    for _ in range(args.rounds):
        rounds["grouped"].append(timed(lambda: grouped.step(zero), args.steps, args.warmup, torch))
        rounds["lone"].append(timed(lone_steps, args.steps, args.warmup, torch))
        rounds["plain"].append(timed(lambda: plain.step(zero), args.steps, args.warmup, torch))
    for e in [grouped, plain] + lone:
        e.check_error()
    med = lambda v: float(np.median(v))
    spread = lambda v: float((max(v) - min(v)) / np.median(v))
    a, b, c = med(rounds["grouped"]) * 1e6, med(rounds["lone"]) * 1e6, med(rounds["plain"]) * 1e6
    result = {"N": N, "R": R, "n_per_group": N // R, "steps": args.steps, "rounds": args.rounds, "backend": _capi.backend_info(),
              "a_grouped_step_us": a, "b_lone_steps_us": b, "c_plain_step_us": c, "b_over_a": b / a, "a_over_c": a / c,
              "a_spread": spread(rounds["grouped"]), "b_spread": spread(rounds["lone"]), "c_spread": spread(rounds["plain"]),
              "rounds_us": {k: [x * 1e6 for x in v] for k, v in rounds.items()}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
