#!/usr/bin/env python3
"""What a population of categorical (C51) policies (actor.C51ActorPopulation: P members on slices of one batch, ONE launch of
k_c51actor_eval_pop) costs next to the same P lone C51Actors evaluated one after another on their slices (P launches of k_c51actor_eval), at
Kmax = 16 for the 20 -> 256 -> 5 x 51 network, 4096 rows in total, P = 1, 4, 16.  The members are views of P learners with different seeds, supports
and tables.  Before anything is timed the two sides' jerk, action, expected values and input vectors are compared bit for bit.  The sides are timed
in the same process, interleaved, in three rounds (_timing.timed: windows of 20 calls with a synchronisation at both ends); medians are reported.
Writes profiles/actor/c51actor_pop_bench.json and prints it as one JSON line.
   usage: python scripts/c51actor_pop_bench.py [--pop 1 4 16] [--rows 4096] [--steps 400] [--warmup 40]
          python scripts/c51actor_pop_bench.py --only-pop --calls 50    the population's evaluations alone, `calls` per P, nothing timed or
                                                                       written: the program of a `rocprofv3 --kernel-trace --stats` run,
                                                                       whose k_c51actor_eval_pop count is then len(pop) * calls and whose
                                                                       k_c51actor_eval count is 0
          python scripts/c51actor_pop_bench.py --lone PARENT.json THIS.json   merges two runs of scripts/c51actor_bench.py (the parent commit's and
                                                                       this one's, same session, five rounds each) into the JSON with the
                                                                       check that the lone kernel did not get slower (no GPU needed)
          python scripts/c51actor_pop_bench.py --table                  prints the JSON's figures as the DESIGN section quotes them (no GPU needed)"""
import argparse
import json
import os
import sys

from _timing import timed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
KMAX, ROUNDS = 16, 3
NET = (20, 256, 5, 51)


def lone_check(parent, this):
    """The lone k_c51actor_eval before and after its text moved into a __device__ body: this commit's median against the parent's slowest round
    plus the parent's own min-max spread over its rounds as margin."""
    p, t = parent["rounds_us"]["fused"], this["rounds_us"]["fused"]
    spread = max(p) - min(p)
    return {"parent_rounds_us": p, "this_rounds_us": t, "parent_median_us": parent["fused_us"], "this_median_us": this["fused_us"],
            "parent_min_us": min(p), "parent_max_us": max(p), "parent_spread_us": spread, "bound_us": max(p) + spread,
            "not_slower": bool(this["fused_us"] <= max(p) + spread), "parent_backend": parent["backend"], "this_backend": this["backend"],
            "n": this["n"], "net": this["net"]}


def table(r):
    rows = ["| P | rows per member | population, one launch | P lone evaluations | ratio |", "|---|---|---|---|---|"]
    for s in sorted(r["shapes"].values(), key=lambda s: s["P"]):
        rows.append("| %d | %d | %.1f us | %.1f us | %.2f x |" % (s["P"], s["n_per_member"], s["pop_eval_us"], s["separate_evals_us"], s["speedup_vs_separate"]))
    c = r.get("lone_kernel")
    if c:
        rows += ["", "Lone `k_c51actor_eval`, N = %d: parent %.1f us (rounds %.1f ... %.1f, spread %.1f), this commit %.1f us; bound %.1f us: %s." % (
            c["n"], c["parent_median_us"], c["parent_min_us"], c["parent_max_us"], c["parent_spread_us"], c["this_median_us"], c["bound_us"],
            "not slower" if c["not_slower"] else "SLOWER")]
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pop", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--only-pop", action="store_true")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--lone", nargs=2, metavar=("PARENT", "THIS"))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "actor", "c51actor_pop_bench.json"))
    ap.add_argument("--table", action="store_true")
    args = ap.parse_args()
    if args.table:
        print(table(json.load(open(args.out))))
        return
    if args.lone:
        result = json.load(open(args.out)) if os.path.exists(args.out) else {}
        result["lone_kernel"] = lone_check(json.load(open(args.lone[0])), json.load(open(args.lone[1])))
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1, sort_keys=True)
        print(json.dumps(result["lone_kernel"], sort_keys=True))
        if not result["lone_kernel"]["not_slower"]:
            raise SystemExit("the lone k_c51actor_eval got slower: %.2f us against a bound of %.2f us" % (result["lone_kernel"]["this_median_us"], result["lone_kernel"]["bound_us"]))
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
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    n_obs, h1, A, K = NET
    N = args.rows
    ego, kc, ox, ov, _ = combined_bench.bench_states(N, 3000, S)
    pad = lambda a: np.concatenate([a, np.zeros((N, KMAX - a.shape[1]))], axis=1)
    d_ego5, d_k, d_ox, d_ov = t(ego), t(kc), t(pad(ox)), t(pad(ov))
    d_ego4, d_oa = d_ego5[:, :4].contiguous(), torch.zeros_like(d_ox)
    result = json.load(open(args.out)) if os.path.exists(args.out) and not args.only_pop else {}
    result.update({"kmax": KMAX, "net": list(NET), "rows": N, "steps": args.steps, "rounds": ROUNDS, "backend": _capi.backend_info(), "shapes": {}})
    for P in args.pop:
        if N % P:
            raise SystemExit("%d rows do not split into %d members" % (N, P))
        n = N // P
        learners = []
        for m in range(P):
            cfg = learner.C51Config(n_obs=n_obs, n_actions=A, h1=h1, n_atoms=K, v_min=-10.0 - 0.5 * m, v_max=10.0 + 0.25 * m, batch=16, capacity=64)
            L = learner.C51Learner((n_obs, A), cfg, seed=1 + m, ctx=ctx)
            L.action_values = np.array([S.JERK_VALUES_DQN[i] for i in range(A)], dtype=np.float64) + 0.125 * m
            learners.append(L)
        pop = actor.C51ActorPopulation(learners, n, ctx, S)
        sl = [slice(m * n, (m + 1) * n) for m in range(P)]
        views = {q: [x[s] for s in sl] for q, x in (("ego4", d_ego4), ("k", d_k), ("ox", d_ox), ("ov", d_ov), ("oa", d_oa))}

        def eval_pop():
            pop(1, d_ego4, d_k, d_ox, d_ov, d_oa)

        if args.only_pop:
            for _ in range(args.calls):
                eval_pop()
            torch.cuda.synchronize()
            ctx.check_error()
            print("P = %d: %d evaluations of the population" % (P, args.calls), flush=True)
            continue
        lone = [actor.C51Actor.from_learner(L, n, ctx, S) for L in learners]

        def eval_lone():
            for m, a in enumerate(lone):
                a(1, views["ego4"][m], views["k"][m], views["ox"][m], views["ov"][m], views["oa"][m])

        pop.keep_q = pop.keep_features = True
        for a in lone:
            a.keep_q = a.keep_features = True
        eval_pop(), eval_lone()
        torch.cuda.synchronize()
        for key in ("jerk", "action", "q", "feat"):
            got, want = getattr(pop, key).cpu().numpy(), np.concatenate([getattr(a, key).cpu().numpy() for a in lone])
            if got.tobytes() != want.tobytes():
                raise SystemExit("P = %d: the population and the lone actors disagree on %s" % (P, key))
        distinct = int(np.unique(pop.jerk.cpu().numpy()).size)
        pop.keep_q = pop.keep_features = False
        for a in lone:
            a.keep_q = a.keep_features = False
        rounds = {"pop": [], "lone": []}
        for _ in range(ROUNDS):
            rounds["pop"].append(timed(eval_pop, args.steps, args.warmup, torch))
            rounds["lone"].append(timed(eval_lone, args.steps, args.warmup, torch))
        ctx.check_error()
        med = {q: float(np.median(v)) for q, v in rounds.items()}
        result["shapes"]["P%d" % P] = {"P": P, "n_per_member": n, "rows": N, "pop_eval_us": med["pop"] * 1e6, "separate_evals_us": med["lone"] * 1e6,
                                       "speedup_vs_separate": med["lone"] / med["pop"], "pop_states_per_s": N / med["pop"], "outputs_bit_identical": True,
                                       "distinct_jerks": distinct, "launches_per_evaluation": {"population": 1, "separate": P},
                                       "rounds_us": {q: [x * 1e6 for x in v] for q, v in rounds.items()}}
        print("P%d" % P, json.dumps(result["shapes"]["P%d" % P], sort_keys=True), flush=True)
        del pop, lone
    if args.only_pop:
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
