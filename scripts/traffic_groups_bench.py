#!/usr/bin/env python3
"""What traffic groups (G groups of n_per_group environments with their own stmpc_sim_cfg in one world: csrc/stmpc_sim_groups_kernels.hpp) cost and
gain next to the paths that existed before them, at Kmax = 16:
  (a) the overhead of grouping: a G = 1 grouped MergeVecEnv.step and EpisodeRunner.tick (ST controller) at N = 4096 against the plain entries of
      the same N and seed -- the same worlds bit for bit, the same grids -- next to the plain entries' own round-to-round spread
  (b) the gain: one grouped env step / one combined-controller tick for the five reference traffic types at 256 and 4096 environments per group
      against five separate worlds (five contexts) stepped one after another, the path before groups
  (c) one episodes.cross_matrix run: the five shipped actors x the five traffic types; wall time and ticks per second (nothing to compare with)
The sides of a comparison are timed in the same process, interleaved, in three rounds (windows of 20 calls with a synchronisation at both ends);
medians are reported.  Writes profiles/env/groups_bench.json and prints it as one JSON line.
   usage: python scripts/traffic_groups_bench.py [--n-per-group 256 4096] [--steps 200] [--warmup 20] [--tick-steps 20] [--tick-warmup 3] [--cells 256]
          python scripts/traffic_groups_bench.py --table     prints the JSON's figures as the tables DESIGN section 16 quotes (no GPU needed)"""
import argparse
import json
import os
import sys
import time

from _timing import timed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
KMAX = 16
FIVE = ("low", "medium", "default", "moderate", "fast")
ACTORS = ("low1", "medium1", "default1", "moderate1", "fast1")


def tables(result):
    o = result["overhead_G1"]
    rows = ["| N = %d, G = 1 | plain entries | grouped entries | grouped / plain | plain entries' spread over rounds |" % o["N"], "|---|---|---|---|---|"]
    for what, unit, scale in (("env_step", "us", 1.0), ("st_tick", "ms", 1e-3)):
        rows.append("| %s | %.1f %s | %.1f %s | %.3f | %.1f %% |" % (what.replace("_", " "), o[what + "_plain_us"] * scale, unit, o[what + "_grouped_us"] * scale, unit,
                                                                  o[what + "_ratio"], 100.0 * o[what + "_plain_spread"]))
    rows += ["", "| n per group (5 traffic types) | grouped env step | 5 separate env steps | vs separate | grouped combined tick | 5 separate ticks | vs separate |",
             "|---|---|---|---|---|---|---|"]
    for r in sorted(result["gain_five_types"].values(), key=lambda r: r["n_per_group"]):
        rows.append("| %d | %.1f us | %.1f us | %.2f x | %.2f ms | %.2f ms | %.2f x |" % (
            r["n_per_group"], r["grouped_step_us"], r["separate_steps_us"], r["step_speedup"], r["grouped_tick_us"] / 1e3, r["separate_ticks_us"] / 1e3, r["tick_speedup"]))
    c = result.get("cross_matrix")
    if c:
        rows += ["", "`cross_matrix`, %d models x %d traffic types x %d episodes of at most %.0f s: %.2f s wall, %d runner ticks, %.0f environment ticks per second." % (
            c["models"], c["traffic"], c["n_per_cell"], c["max_episode_length_s"], c["wall_s"], c["runner_ticks"], c["env_ticks_per_s"])]
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-per-group", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--overhead-n", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--tick-steps", type=int, default=20)
    ap.add_argument("--tick-warmup", type=int, default=3)
    ap.add_argument("--cells", type=int, default=256)
    ap.add_argument("--skip-cross", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "env", "groups_bench.json"))
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
    from rl_mpc_lanemerging_amd import _capi, actor, combined_bench, episodes, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    pkg.apply_overrides(combined_bench.COMBINED_MEDIUM_1)
    S = pkg.Settings
    dev = torch.device("cuda", torch.cuda.current_device())
    result = {"kmax": KMAX, "steps": args.steps, "tick_steps": args.tick_steps, "backend": _capi.backend_info(), "gain_five_types": {}}
    med = lambda v: float(np.median(v))
    spread = lambda v: float((max(v) - min(v)) / np.median(v))

    def lone_settings(name):
        """The global Settings with one traffic type's values, for building a separate world the way it was done before groups."""
        snap = S.snapshot()
        pkg.apply_overrides(episodes.TRAFFIC_TYPES[name])
        return snap

    # (a) G = 1 against the plain entries
    N = args.overhead_n
    env_p = vec_env.MergeVecEnv(N, env_id="sumo-jerk-continuous-v0", seed=1)
    env_g = vec_env.MergeVecEnv(N, env_id="sumo-jerk-continuous-v0", seed=1, traffic=["default"])
    run_p = episodes.EpisodeRunner(N, seed=1, controller="st", ctx=_capi.Context(-1), kmax=KMAX)
    run_g = episodes.EpisodeRunner(N, seed=1, controller="st", ctx=_capi.Context(-1), kmax=KMAX, traffic=["default"])
    zero = torch.zeros(N, dtype=torch.float64, device=dev)
    env_p.reset(), env_g.reset()
    rounds = {"step_p": [], "step_g": [], "tick_p": [], "tick_g": []}
    for _ in range(3):
        rounds["step_p"].append(timed(lambda: env_p.step(zero), args.steps, args.warmup, torch))
        rounds["step_g"].append(timed(lambda: env_g.step(zero), args.steps, args.warmup, torch))
        rounds["tick_p"].append(timed(run_p.tick, args.tick_steps, args.tick_warmup, torch))
        rounds["tick_g"].append(timed(run_g.tick, args.tick_steps, args.tick_warmup, torch))
    env_p.check_error(), env_g.check_error(), run_p.ctx.check_error(), run_g.ctx.check_error()
    result["overhead_G1"] = {"N": N,
                             "env_step_plain_us": med(rounds["step_p"]) * 1e6, "env_step_grouped_us": med(rounds["step_g"]) * 1e6,
                             "env_step_ratio": med(rounds["step_g"]) / med(rounds["step_p"]), "env_step_plain_spread": spread(rounds["step_p"]),
                             "st_tick_plain_us": med(rounds["tick_p"]) * 1e6, "st_tick_grouped_us": med(rounds["tick_g"]) * 1e6,
                             "st_tick_ratio": med(rounds["tick_g"]) / med(rounds["tick_p"]), "st_tick_plain_spread": spread(rounds["tick_p"]),
                             "rounds_us": {q: [x * 1e6 for x in v] for q, v in rounds.items()}}
    print("overhead_G1", json.dumps(result["overhead_G1"], sort_keys=True), flush=True)
    del env_p, env_g, run_p, run_g

    # (b) the five reference traffic types: one grouped world against five separate ones
    G = len(FIVE)
    for n in args.n_per_group:
        N = G * n
        genv = vec_env.MergeVecEnv(N, env_id="sumo-jerk-continuous-v0", seed=1, traffic=list(FIVE))
        gctx = _capi.Context(-1)
        grun = episodes.EpisodeRunner(N, seed=1, controller="combined", policy=actor.ActorPopulation(list(ACTORS), n, gctx, S), ctx=gctx, kmax=KMAX, traffic=list(FIVE))
        lenvs, lruns = [], []
        for g, name in enumerate(FIVE):
            snap = lone_settings(name)
            lenvs.append(vec_env.MergeVecEnv(n, env_id="sumo-jerk-continuous-v0", seed=vec_env.episode_seed(1, g)))
            lctx = _capi.Context(-1)
            lruns.append(episodes.EpisodeRunner(n, seed=vec_env.episode_seed(1, g), controller="combined", policy=actor.DDPGActor(ACTORS[g], n, lctx, S, dev), ctx=lctx,
                                                kmax=KMAX))
            S.restore(snap)
        zero, lzero = torch.zeros(N, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev)
        genv.reset()
        for e in lenvs:
            e.reset()

        def lone_steps():
            for e in lenvs:
                e.step(lzero)

        def lone_ticks():
            for r in lruns:
                r.tick()

        rounds = {"step_g": [], "step_l": [], "tick_g": [], "tick_l": []}
        for _ in range(3):
            rounds["step_g"].append(timed(lambda: genv.step(zero), args.steps, args.warmup, torch))
            rounds["step_l"].append(timed(lone_steps, args.steps, args.warmup, torch))
            rounds["tick_g"].append(timed(grun.tick, args.tick_steps, args.tick_warmup, torch))
            rounds["tick_l"].append(timed(lone_ticks, args.tick_steps, args.tick_warmup, torch))
        genv.check_error(), gctx.check_error()
        for e, r in zip(lenvs, lruns):
            e.check_error(), r.ctx.check_error()
        result["gain_five_types"]["n%d" % n] = {
            "G": G, "n_per_group": n, "rows": N,
            "grouped_step_us": med(rounds["step_g"]) * 1e6, "separate_steps_us": med(rounds["step_l"]) * 1e6, "step_speedup": med(rounds["step_l"]) / med(rounds["step_g"]),
            "grouped_tick_us": med(rounds["tick_g"]) * 1e6, "separate_ticks_us": med(rounds["tick_l"]) * 1e6, "tick_speedup": med(rounds["tick_l"]) / med(rounds["tick_g"]),
            "rounds_us": {q: [x * 1e6 for x in v] for q, v in rounds.items()}}
        print("n%d" % n, json.dumps(result["gain_five_types"]["n%d" % n], sort_keys=True), flush=True)
        del genv, grun, lenvs, lruns

    # (c) the models x traffic matrix in one run
    if not args.skip_cross:
        length = 100.0
        cctx = _capi.Context(-1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cm = episodes.cross_matrix(list(ACTORS), list(FIVE), args.cells, seed=1, ctx=cctx, kmax=KMAX, max_episode_length=length)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        ticks = cm["stats"]["ticks"]
        result["cross_matrix"] = {"models": len(ACTORS), "traffic": len(FIVE), "n_per_cell": args.cells, "rows": int(len(ticks)), "max_episode_length_s": length,
                                  "wall_s": wall, "runner_ticks": int(ticks.max()), "env_ticks": int(ticks.sum()), "env_ticks_per_s": float(ticks.sum() / wall),
                                  "merged": [[c["merged"] for c in row] for row in cm["matrix"]], "crashed": [[c["crashed"] for c in row] for row in cm["matrix"]]}
        print("cross_matrix", json.dumps(result["cross_matrix"], sort_keys=True), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
