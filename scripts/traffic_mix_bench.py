#!/usr/bin/env python3
"""What the traffic mix (every episode of a MergeVecEnv draws its own traffic type on the device: csrc/stmpc_traffic_mix_kernels.hpp) costs next to the
plain env, at N = 4096 and T = 5 (the five reference traffic types, uniform weights):
  (a) one mixed MergeVecEnv.step of N environments
  (b) the plain MergeVecEnv.step of the same N and seed under "default" traffic
The expectation, to be measured and not a threshold: equal within the rounds' spread, as the reward groups' table read was -- the step is
launch-bound, and the mix adds one 24-byte table row per lane and launch.  Both sides are timed in the same process on live worlds (autoreset on,
episodes of the default length) under the same seeded uniform jerks from the Box, interleaved, in five rounds (windows of 20 calls with a
synchronisation at both ends); medians and the spread over rounds are reported.  Writes profiles/env/traffic_mix_bench.json and prints it as one JSON
line.
   usage: python scripts/traffic_mix_bench.py [--n 4096] [--steps 200] [--warmup 20] [--rounds 5]"""
import argparse
import json
import os
import sys

from _timing import WINDOW, timed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
MIX = ["low", "medium", "default", "moderate", "fast"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "env", "traffic_mix_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import rl_mpc_lanemerging_amd as pkg
    if pkg.build.needs_build():
        raise SystemExit("build the library first (__graft_entry__.build())")
    from rl_mpc_lanemerging_amd import _capi, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    dev = torch.device("cuda", torch.cuda.current_device())
    N = args.n
    env_id = "sumo-jerk-continuous-v0"
    mixed = vec_env.MergeVecEnv(N, env_id=env_id, seed=1, traffic_mix=MIX)
    plain = vec_env.MergeVecEnv(N, env_id=env_id, seed=1, traffic=["default"])
    box = mixed.action_space
    gen = torch.Generator(device="cpu").manual_seed(11)
    jerks = (box["low"] + (box["high"] - box["low"]) * torch.rand(WINDOW, N, dtype=torch.float64, generator=gen)).to(dev)
    for e in (mixed, plain):
        e.reset()
    turn = {"mixed": 0, "plain": 0}

    def step(env, name):
        env.step(jerks[turn[name] % WINDOW])
        turn[name] += 1
    rounds = {"mixed": [], "plain": []}
    for _ in range(args.rounds):
        rounds["mixed"].append(timed(lambda: step(mixed, "mixed"), args.steps, args.warmup, torch))
        rounds["plain"].append(timed(lambda: step(plain, "plain"), args.steps, args.warmup, torch))
    for e in (mixed, plain):
        e.check_error()
    log = mixed.drain_episode_stats()
    med = lambda v: float(np.median(v))
    spread = lambda v: float((max(v) - min(v)) / np.median(v))
    a, b = med(rounds["mixed"]) * 1e6, med(rounds["plain"]) * 1e6
    result = {"N": N, "T": len(MIX), "traffic_mix": MIX, "steps": args.steps, "rounds": args.rounds, "backend": _capi.backend_info(),
              "a_mixed_step_us": a, "b_plain_step_us": b, "a_over_b": a / b, "a_spread": spread(rounds["mixed"]), "b_spread": spread(rounds["plain"]),
              "episodes_by_type": [row["episodes"] for row in mixed.summary_by_traffic(log)],
              "rounds_us": {k: [x * 1e6 for x in v] for k, v in rounds.items()}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
