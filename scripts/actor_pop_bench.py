#!/usr/bin/env python3
"""What a population of actors (actor.ActorPopulation: P members on slices of one batch, one launch) costs next to the paths that existed before
it, at Kmax = 16, for P members of n_per_member states each:
  (a) one policy evaluation: the population vs the same P actors evaluated one after another on their slices (P launches of k_actor_eval), and
      vs ONE single-actor launch over all P * n_per_member rows -- the floor: the same arithmetic with one set of weights
  (b) one tick of the combined controller (combined.decide_batch_device): P * n_per_member environments under the population vs P ticks of
      n_per_member environments, one per actor
  (c) P = 4: learner.evaluate_members from zero-copy views of a DDPGPopulation vs the chain it replaces, per member: synchronise, export_actor to a
      file, DDPGActor from that file, a runner of its own
The sides of a comparison are timed in the same process, interleaved, in three rounds (windows of 20 calls with a synchronisation at both ends);
medians are reported.  Writes profiles/actor/pop_bench.json and prints it as one JSON line.
   usage: python scripts/actor_pop_bench.py [--pop 1 4 16] [--n-per-member 256 4096] [--steps 200] [--warmup 20] [--tick-steps 20] [--tick-warmup 3]
          python scripts/actor_pop_bench.py --table     prints the JSON's figures as the tables DESIGN section 15 quotes (no GPU needed)"""
import argparse
import json
import os
import sys
import tempfile
import time

from _timing import timed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
KMAX = 16


def tables(result):
    rows = ["| P | n per member | population | P separate evaluations | one actor, all rows (floor) | vs separate | combined tick, population | P separate ticks | vs separate |",
            "|---|---|---|---|---|---|---|---|---|"]
    for r in sorted(result["shapes"].values(), key=lambda r: (r["n_per_member"], r["P"])):
        rows.append("| %d | %d | %.1f us | %.1f us | %.1f us | %.2f x | %.2f ms | %.2f ms | %.2f x |" % (
            r["P"], r["n_per_member"], r["pop_eval_us"], r["separate_evals_us"], r["single_actor_all_rows_us"], r["eval_speedup_vs_separate"],
            r["pop_tick_us"] / 1e3, r["separate_ticks_us"] / 1e3, r["tick_speedup"]))
    c = result.get("evaluate_members_P4")
    if c:
        rows += ["", "`evaluate_members` from views, P = %d x %d episodes of at most %.0f s: %.0f ms; export, file, load and a runner per member: %.0f ms (%.2f x)." % (
            c["P"], c["n_per_member"], c["max_episode_length_s"], c["from_views_ms"], c["export_file_load_run_ms"], c["speedup"])]
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pop", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--n-per-member", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--tick-steps", type=int, default=20)
    ap.add_argument("--tick-warmup", type=int, default=3)
    ap.add_argument("--skip-chain", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "actor", "pop_bench.json"))
    ap.add_argument("--table", action="store_true")
    args = ap.parse_args()
    if args.table:
        print(tables(json.load(open(args.out))))
        return
    import numpy as np
    import torch
    import rl_mpc_lanemerging_amd as pkg
    if pkg.build.needs_build():
        raise SystemExit("build the library first (__graft_entry__.build())")
    from rl_mpc_lanemerging_amd import _capi, actor, combined, combined_bench, episodes, learner, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    pkg.apply_overrides(combined_bench.COMBINED_MEDIUM_1)
    S = pkg.Settings
    dev = torch.device("cuda", torch.cuda.current_device())
    ctx = _capi.default_context()
    params = _capi.Params.from_settings(S)
    ccfg = _capi.CombinedCfg.from_settings(S, sparse_control=True)
    stream = torch.cuda.current_stream().cuda_stream
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    result = {"kmax": KMAX, "steps": args.steps, "tick_steps": args.tick_steps, "backend": _capi.backend_info(), "shapes": {}}
    for n in args.n_per_member:
        for P in args.pop:
            N = P * n
            ego, kc, ox, ov, evals0 = combined_bench.bench_states(N, 3000, S)
            pad = lambda a: np.concatenate([a, np.zeros((N, KMAX - a.shape[1]))], axis=1)
            d_ego5, d_k, d_ox, d_ov, d_e0 = t(ego), t(kc), t(pad(ox)), t(pad(ov)), t(evals0)
            d_ego4, d_oa = d_ego5[:, :4].contiguous(), torch.zeros_like(d_ox)
            sl = [slice(m * n, (m + 1) * n) for m in range(P)]
            names = [actor.PRETRAINED[m % len(actor.PRETRAINED)] for m in range(P)]
            pop = actor.ActorPopulation(names, n, ctx, S)
            lone = [actor.DDPGActor(name, n, ctx, S, dev) for name in names]
            whole = actor.DDPGActor(names[0], N, ctx, S, dev)
            views = {q: [x[s] for s in sl] for q, x in (("ego5", d_ego5), ("ego4", d_ego4), ("k", d_k), ("ox", d_ox), ("ov", d_ov), ("oa", d_oa), ("e0", d_e0))}

            def eval_pop():
                pop(1, d_ego4, d_k, d_ox, d_ov, d_oa)

            def eval_lone():
                for m, a in enumerate(lone):
                    a(1, views["ego4"][m], views["k"][m], views["ox"][m], views["ov"][m], views["oa"][m])

            def eval_whole():
                whole(1, d_ego4, d_k, d_ox, d_ov, d_oa)

            def tick_pop():
                pop.evals.copy_(d_e0)          # every timed tick is the same tick of the same episodes
                combined.decide_batch_device(ctx, params, ccfg, d_ego5, d_k, d_ox, d_ov, pop, None, stream, d_oa=d_oa)

            def tick_lone():
                for m, a in enumerate(lone):
                    a.evals.copy_(views["e0"][m])
                    combined.decide_batch_device(ctx, params, ccfg, views["ego5"][m], views["k"][m], views["ox"][m], views["ov"][m], a, None, stream, d_oa=views["oa"][m])

            rounds = {"eval_pop": [], "eval_lone": [], "eval_whole": [], "tick_pop": [], "tick_lone": []}
            for _ in range(3):
                rounds["eval_pop"].append(timed(eval_pop, args.steps, args.warmup, torch))
                rounds["eval_lone"].append(timed(eval_lone, args.steps, args.warmup, torch))
                rounds["eval_whole"].append(timed(eval_whole, args.steps, args.warmup, torch))
                rounds["tick_pop"].append(timed(tick_pop, args.tick_steps, args.tick_warmup, torch))
                rounds["tick_lone"].append(timed(tick_lone, args.tick_steps, args.tick_warmup, torch))
            ctx.check_error()
            med = {q: float(np.median(v)) for q, v in rounds.items()}
            result["shapes"]["P%d_n%d" % (P, n)] = {
                "P": P, "n_per_member": n, "rows": N,
                "pop_eval_us": med["eval_pop"] * 1e6, "separate_evals_us": med["eval_lone"] * 1e6, "single_actor_all_rows_us": med["eval_whole"] * 1e6,
                "eval_speedup_vs_separate": med["eval_lone"] / med["eval_pop"], "eval_over_floor": med["eval_pop"] / med["eval_whole"],
                "pop_tick_us": med["tick_pop"] * 1e6, "separate_ticks_us": med["tick_lone"] * 1e6, "tick_speedup": med["tick_lone"] / med["tick_pop"],
                "pop_ticks_per_s": N / med["tick_pop"], "separate_ticks_per_s": N / med["tick_lone"],
                "rounds_us": {q: [x * 1e6 for x in v] for q, v in rounds.items()}}
            print("P%d_n%d" % (P, n), json.dumps(result["shapes"]["P%d_n%d" % (P, n)], sort_keys=True), flush=True)
            del pop, lone, whole
    if not args.skip_chain:
        P, n, length = 4, 256, 10.0
        pkg.apply_overrides(combined_bench.COMBINED_MEDIUM_1_TRAFFIC)
        env = vec_env.MergeVecEnv(P * 64, seed=1, ctx=ctx)
        lpop = learner.DDPGPopulation(env, (learner.DDPGConfig(n_obs=env.obs_dim, batch=100, capacity=1 << 14, replay_start=0), P), seeds=[1, 2, 3, 4],
                                      init=list(actor.PRETRAINED[:P]))
        obs = env.reset()
        for _ in range(4):                                          # a few updates, so that the members are no longer the files they started from
            ticks = env.episode_ticks.clone()
            a = lpop.act(obs, ticks, noise=True)
            nobs, r, term, trunc, info = env.step(a)
            lpop.push(obs, ticks, a, r, nobs, term, trunc, final_obs=info["final_observation"])
            lpop.update(1)
            obs = nobs
        torch.cuda.synchronize()
        ectx = _capi.Context(-1)
        tmp = tempfile.mkdtemp()

        def from_views():
            return learner.evaluate_members(lpop, n, seed=3, kmax=KMAX, max_episode_length=length, ctx=ectx)["by_member"]

        def chain():
            rows = []
            for m in range(P):
                torch.cuda.synchronize()
                path = lpop.member(m).export_actor(os.path.join(tmp, "member%d.npz" % m))
                pol = actor.DDPGActor(path, n, ectx, S, dev)
                rows.append(episodes.summary(episodes.run_episodes(n, seed=3, controller="combined", policy=pol, ctx=ectx, kmax=KMAX, max_episode_length=length)))
            return rows

        from_views(), chain()                                       # warm-up
        times = {"views": [], "chain": []}
        for _ in range(3):
            for label, fn in (("views", from_views), ("chain", chain)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[label].append(time.perf_counter() - t0)
        result["evaluate_members_P4"] = {"P": P, "n_per_member": n, "max_episode_length_s": length,
                                         "from_views_ms": float(np.median(times["views"])) * 1e3, "export_file_load_run_ms": float(np.median(times["chain"])) * 1e3,
                                         "speedup": float(np.median(times["chain"]) / np.median(times["views"])),
                                         "rounds_ms": {q: [x * 1e3 for x in v] for q, v in times.items()}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
