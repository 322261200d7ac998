#!/usr/bin/env python3
"""What one evaluation of a categorical (C51) policy costs: the fused launch (actor.C51Actor: k_c51actor_eval -- state vector, logits network,
expected values, argmax, action table) against the composition it replaces, on the same N states at Kmax = 16 for the 20 -> 256 -> 5 x 51 network:
  stmpc_policy_features_device (time feature off), C51Learner.act (eps = 0), then the table gather and the cast to fp64 in torch.
Both sides are timed in the same process, interleaved, in five rounds (_timing.timed: windows of 20 calls with a synchronisation at both ends); the
medians are reported, as evaluations (states) per second, with their ratio.  Before anything is timed the two sides' jerks are compared bit for bit.
Writes profiles/actor/c51actor_bench.json and prints it as one JSON line.
   usage: python scripts/c51actor_bench.py [--n 4096] [--steps 400] [--warmup 40]
          python scripts/c51actor_bench.py --table     prints the JSON's figures as the line DESIGN section 38 quotes (no GPU needed)"""
import argparse
import json
import os
import sys

from _timing import timed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
KMAX, ROUNDS = 16, 5
NET = (20, 256, 5, 51)


def table(r):
    return ("N = %d, %d -> %d -> %d x %d, Kmax = %d: fused launch %.1f us per evaluation (%.1f M states/s); features + act + table gather %.1f us "
            "(%.1f M states/s); ratio %.2f x." % ((r["n"],) + tuple(r["net"]) + (r["kmax"], r["fused_us"], r["fused_states_per_s"] / 1e6, r["composed_us"],
                                                                                 r["composed_states_per_s"] / 1e6, r["speedup"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "actor", "c51actor_bench.json"))
    ap.add_argument("--table", action="store_true")
    args = ap.parse_args()
    if args.table:
        print(table(json.load(open(args.out))))
        return
    import numpy as np
    import torch
    import rl_mpc_lanemerging_amd as pkg
    if pkg.build.needs_build():
        raise SystemExit("build the library first (__graft_entry__.build())")
    from rl_mpc_lanemerging_amd import _capi, actor, combined_bench, learner
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    pkg.apply_overrides(combined_bench.COMBINED_MEDIUM_1)
    S = pkg.Settings
    dev = torch.device("cuda", torch.cuda.current_device())
    ctx = _capi.default_context()
    stream = torch.cuda.current_stream().cuda_stream
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    N = args.n
    n_obs, h1, A, K = NET
    ego, kc, ox, ov, _ = combined_bench.bench_states(N, 3000, S)
    pad = lambda a: np.concatenate([a, np.zeros((N, KMAX - a.shape[1]))], axis=1)
    d_ego5, d_k, d_ox, d_ov = t(ego), t(kc), t(pad(ox)), t(pad(ov))
    d_ego4, d_oa = d_ego5[:, :4].contiguous(), torch.zeros_like(d_ox)
    L = learner.C51Learner((n_obs, A), learner.C51Config(n_obs=n_obs, n_actions=A, h1=h1, n_atoms=K), seed=1, ctx=ctx)
    L.action_values = np.array([S.JERK_VALUES_DQN[i] for i in range(A)], dtype=np.float64)
    pol = actor.C51Actor.from_learner(L, N, ctx, S)
    fcfg = _capi.FeaturesCfg.from_settings(S, time_feature=False)
    feat = torch.empty(N, n_obs, dtype=torch.float32, device=dev)
    d_table = t(L.action_values)

    def fused():
        return pol(1, d_ego4, d_k, d_ox, d_ov, d_oa)

    def composed():
        ctx.policy_features_device(fcfg, N, KMAX, 1, d_ego4.data_ptr(), d_k.data_ptr(), d_ox.data_ptr(), d_ov.data_ptr(), d_oa.data_ptr(), 0, feat.data_ptr(), n_obs, stream)
        return d_table[L.act(feat, eps=0.0).long()].to(torch.float64)

    a, b = fused().cpu().numpy().copy(), composed().cpu().numpy()
    if not np.array_equal(a.view(np.uint64), b.view(np.uint64)):
        raise SystemExit("the fused launch and the composition disagree on %d of %d jerks" % (int((a != b).sum()), N))
    rounds = {"fused": [], "composed": []}
    for _ in range(ROUNDS):
        rounds["fused"].append(timed(fused, args.steps, args.warmup, torch))
        rounds["composed"].append(timed(composed, args.steps, args.warmup, torch))
    ctx.check_error()
    med = {q: float(np.median(v)) for q, v in rounds.items()}
    result = {"n": N, "net": list(NET), "kmax": KMAX, "steps": args.steps, "rounds": ROUNDS, "backend": _capi.backend_info(),
              "fused_us": med["fused"] * 1e6, "composed_us": med["composed"] * 1e6, "fused_states_per_s": N / med["fused"],
              "composed_states_per_s": N / med["composed"], "speedup": med["composed"] / med["fused"], "jerks_bit_identical": True,
              "distinct_actions": int(np.unique(a).size), "rounds_us": {q: [x * 1e6 for x in v] for q, v in rounds.items()}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
