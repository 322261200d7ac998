#!/usr/bin/env python3
"""What the shielded env step (MergeVecEnv(shield="first_step"): csrc/stmpc_shield_env_kernels.hpp + the body of stmpc_first_step_device) costs next to
the paths that existed before it, at N = 4096, "default" traffic:
  (a) the shielded step, dense (the controller solved for every environment; no host synchronisation)
  (b) the shielded step, sparse (the controller solved for the taken-over environments; one integer crosses to the host)
  (c) the unshielded MergeVecEnv.step
  (d) the shield driven from Python out of the public pieces on a second context that holds the states of (c) -- a twin env of the same seed, stepped
      with (c)'s actions whenever (c) is stepped, outside (d)'s timed windows: sim_view + speed_from_jerk_device + FirstStepController.decide (dense)
      -- (c) + (d) is the work of (a) as a caller had to compose it before (timed together too, with the twin's own step standing in for (c)'s)
All arms are timed in the same process on live worlds (autoreset on, episodes of the default length, seeded uniform jerks in the Box), interleaved, in
five rounds (windows of 20 calls with a synchronisation at both ends); medians and the spread over rounds are reported.  Then the point of the
feature: the crashed share of the finished episodes and the takeover share of a shielded and an unshielded env under the same seed and actions
(n = 1024, 400 ticks: tests/test_shield_env.py's autoreset case).  Writes profiles/env/shield_bench.json and prints it as one JSON line.
   usage: python scripts/shield_env_bench.py [--n 4096] [--steps 100] [--warmup 20] [--rounds 5]"""
import argparse
import json
import os
import sys

from _timing import WINDOW, timed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
KMAX = 32


def crash_shares(vec_env, np, torch, n=1024, ticks=400, seed=7, act_seed=11):
    """Shielded and unshielded env under the same seed and actions: crashed episodes, finished episodes, takeover share."""
    out = {}
    for name, kw in (("shielded", dict(shield="first_step", shield_kmax=KMAX)), ("unshielded", {})):
        env = vec_env.MergeVecEnv(n, seed=seed, reward="Continuous", **kw)
        env.reset()
        rng = np.random.default_rng(act_seed)
        taken = torch.zeros((), dtype=torch.int64, device=env.device)
        for _ in range(ticks):
            info = env.step(torch.as_tensor(rng.uniform(env.action_space["low"], env.action_space["high"], n), device=env.device))[4]
            if kw:
                taken += info["takeover"].sum()
        d = env.drain_episode_stats()
        out[name] = {"episodes": int(len(d["env"])), "crashed": int(d["crashed"].sum()), "crash_share": float(d["crashed"].mean()) if len(d["env"]) else 0.0,
                     "takeover_share": int(taken.item()) / float(n * ticks)}
        env.ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "env", "shield_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import rl_mpc_lanemerging_amd as pkg
    if pkg.build.needs_build():
        raise SystemExit("build the library first (__graft_entry__.build())")
    from rl_mpc_lanemerging_amd import _capi, combined_bench, episodes, first_step, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    pkg.apply_overrides(combined_bench.COMBINED_MEDIUM_1)
    pkg.apply_overrides(episodes.TRAFFIC_TYPES["default"])
    S = pkg.Settings
    dev = torch.device("cuda", torch.cuda.current_device())
    N = args.n
    mk = lambda **kw: vec_env.MergeVecEnv(N, seed=1, reward="Continuous", ctx=_capi.Context(-1), **kw)
    dense, sparse, plain, twin = mk(shield="first_step", shield_kmax=KMAX), mk(shield="first_step", shield_sparse=True, shield_kmax=KMAX), mk(), mk()
    for e in (dense, sparse, plain, twin):
        e.reset()
    rng = np.random.default_rng(3)
    acts = [torch.as_tensor(rng.uniform(plain.action_space["low"], plain.action_space["high"], N), device=dev) for _ in range(16)]
    cursor = [0]

    def act():
        cursor[0] += 1
        return acts[cursor[0] % len(acts)]
    fs = first_step.FirstStepController(N, twin.ctx, twin.params, sparse_control=False)
    z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)
    ego5, k, ox, ov = z(N, 5), z(N, dtype=torch.int32), z(N, KMAX), z(N, KMAX)

    def both_step():                             # (c) and its twin see the same actions, so the twin's context holds (c)'s states
        a = act()
        plain.step(a)
        twin.step(a)

    def pieces():
        twin.ctx.sim_view(twin.sim_cfg, N, KMAX, ego5.data_ptr(), k.data_ptr(), ox.data_ptr(), ov.data_ptr())
        fs.decide_jerk(ego5, k, ox, ov, act())

    def step_and_pieces():                       # the composition as a caller runs it: the env step, then the shield's pieces on the new state
        both_step()
        pieces()

    def advance():                               # untimed, before each of (d)'s windows: a window of fresh states
        for _ in range(WINDOW):
            both_step()
    rounds = {"a_dense": [], "b_sparse": [], "c_plain": [], "d_pieces": [], "c_plus_d": []}
    for _ in range(args.rounds):
        rounds["a_dense"].append(timed(lambda: dense.step(act()), args.steps, args.warmup, torch))
        rounds["b_sparse"].append(timed(lambda: sparse.step(act()), args.steps, args.warmup, torch))
        rounds["c_plain"].append(timed(both_step, args.steps, args.warmup, torch) / 2)          # (two equal env steps per call)
        rounds["d_pieces"].append(timed(pieces, args.steps, args.warmup, torch, before_window=advance))
        rounds["c_plus_d"].append(timed(step_and_pieces, args.steps, args.warmup, torch))       # (holds a second env step: subtract c_plain)
    for e in (dense, sparse, plain, twin):
        e.check_error()
    med = lambda v: float(np.median(v))
    spread = lambda v: float((max(v) - min(v)) / np.median(v))
    result = {"N": N, "kmax": KMAX, "steps": args.steps, "rounds": args.rounds, "backend": _capi.backend_info(), "traffic": "default",
              "shield_counts_dense": dense.shield_counts(), "shield_counts_sparse": sparse.shield_counts(),
              "rounds_us": {k_: [x * 1e6 for x in v] for k_, v in rounds.items()}}
    for k_, v in rounds.items():
        result[k_ + "_us"] = med(v) * 1e6
        result[k_ + "_spread"] = spread(v)
    result["c_plus_d_us"] -= result["c_plain_us"]                   # one env step + the pieces, interleaved on advancing states
    result["a_minus_c_minus_d_us"] = result["a_dense_us"] - result["c_plain_us"] - result["d_pieces_us"]
    result["a_minus_c_plus_d_interleaved_us"] = result["a_dense_us"] - result["c_plus_d_us"]
    result["crash_shares"] = crash_shares(vec_env, np, torch)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
