#!/usr/bin/env python3
"""What one grouped shielded step (vec_env.GroupedShieldVecEnv with the five traffic types of episodes.TRAFFIC_TYPES as traffic groups:
csrc/stmpc_shield_groups_kernels.hpp around the body of stmpc_first_step_device) costs next to the paths that existed before it, at N = 4096 and 65536
(each rounded up to a multiple of the five groups: 4100 and 65540):
  (g) the grouped shielded step: five groups of N / 5 environments, one launch sequence
  (a) the lone shielded step of the same N (MergeVecEnv(shield="first_step"), "default" traffic): the same number of launches
  (b) five lone shielded envs of N / 5 environments, one per traffic type, stepped one after another: what a caller had to do before
(a) and (b) run code this feature does not touch.  All arms are timed in the same process on live worlds (autoreset on, episodes of the default
length, seeded uniform jerks in the Box, dense controller: no host synchronisation), interleaved, in three rounds (windows of 20 calls with a
synchronisation at both ends); medians, the spread over rounds and the ratios g / a and b / g are reported.  Writes
profiles/env/shield_groups_bench.json and prints it as one JSON line.
   usage: python scripts/shield_groups_env_bench.py [--n 4096 65536] [--steps 60] [--warmup 20] [--rounds 3]"""
import argparse
import json
import os
import sys

from _timing import timed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
KMAX = 32
TYPES = ("low", "medium", "default", "moderate", "fast")


def bench(N, args, np, torch, pkg, _capi, episodes, vec_env):
    assert N % len(TYPES) == 0, "N must divide into the five traffic groups"
    npg = N // len(TYPES)
    dev = torch.device("cuda", torch.cuda.current_device())
    kw = dict(seed=1, reward="Continuous", shield_kmax=KMAX)
    grouped = vec_env.GroupedShieldVecEnv(N, ctx=_capi.Context(-1), traffic=list(TYPES), **kw)
    snap = pkg.Settings.snapshot()
    pkg.apply_overrides(episodes.TRAFFIC_TYPES["default"])
    lone = vec_env.MergeVecEnv(N, ctx=_capi.Context(-1), shield="first_step", **kw)
    five = []
    for t in TYPES:
        pkg.Settings.restore(snap)
        pkg.apply_overrides(episodes.TRAFFIC_TYPES[t])
        five.append(vec_env.MergeVecEnv(npg, ctx=_capi.Context(-1), shield="first_step", **kw))
    pkg.Settings.restore(snap)
    for e in [grouped, lone] + five:
        e.reset()
    rng = np.random.default_rng(3)
    acts = [torch.as_tensor(rng.uniform(lone.action_space["low"], lone.action_space["high"], N), device=dev) for _ in range(16)]
    parts = [[a[g * npg:(g + 1) * npg].contiguous() for g in range(len(TYPES))] for a in acts]
    cursor = [0]

    def nxt():
        cursor[0] += 1
        return cursor[0] % len(acts)

    def five_step():
        i = nxt()
        for g, e in enumerate(five):
            e.step(parts[i][g])
    rounds = {"g_grouped": [], "a_lone": [], "b_five_lone": []}
    for _ in range(args.rounds):
        rounds["g_grouped"].append(timed(lambda: grouped.step(acts[nxt()]), args.steps, args.warmup, torch))
        rounds["a_lone"].append(timed(lambda: lone.step(acts[nxt()]), args.steps, args.warmup, torch))
        rounds["b_five_lone"].append(timed(five_step, args.steps, args.warmup, torch))
    for e in [grouped, lone] + five:
        e.check_error()
    med = lambda v: float(np.median(v))
    out = {"N": N, "n_per_group": npg, "rounds_us": {k: [x * 1e6 for x in v] for k, v in rounds.items()},
           "takeover_share_by_group": grouped.takeover_share(), "shield_counts_grouped": grouped.shield_counts(), "shield_counts_lone": lone.shield_counts()}
    for k, v in rounds.items():
        out[k + "_us"] = med(v) * 1e6
        out[k + "_spread"] = float((max(v) - min(v)) / np.median(v))
    out["g_over_a"] = out["g_grouped_us"] / out["a_lone_us"]
    out["b_over_g"] = out["b_five_lone_us"] / out["g_grouped_us"]
    out["g_over_a_rounds"] = [g / a for g, a in zip(rounds["g_grouped"], rounds["a_lone"])]
    out["b_over_g_rounds"] = [b / g for b, g in zip(rounds["b_five_lone"], rounds["g_grouped"])]
    for e in [grouped, lone] + five:
        e.ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "env", "shield_groups_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import rl_mpc_lanemerging_amd as pkg
    if pkg.build.needs_build():
        raise SystemExit("build the library first (__graft_entry__.build())")
    from rl_mpc_lanemerging_amd import _capi, combined_bench, episodes, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    pkg.apply_overrides(combined_bench.COMBINED_MEDIUM_1)
    result = {"kmax": KMAX, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "traffic": list(TYPES), "backend": _capi.backend_info(),
              "sizes": [bench(-(-n // len(TYPES)) * len(TYPES), args, np, torch, pkg, _capi, episodes, vec_env) for n in args.n]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
