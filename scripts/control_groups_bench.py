#!/usr/bin/env python3
"""What controller groups (C groups of n_per_cell environments, each decided under its own stmpc_combined_cfg in one batch:
csrc/stmpc_cc_groups_kernels.hpp) cost and gain next to the path that existed before them, at Kmax = 16: the combined-controller tick of
episodes.EpisodeRunner for the first C cells of the reference's grid search (combined.grid_search_cells(), main.py:62-81), C in {1, 4, 13}, at 256 and
4096 environments per cell, once as ONE runner with ``control=cells`` and once as C separate runners (C contexts) built through the plain entries with
the cell's values in the global Settings and ticked one after another.  Every cell faces the same traffic draws (one seed).  C = 1 is the overhead of
the grouped entries themselves, reported next to the plain tick's own round-to-round spread.
One cost of grouping is by construction and is reported beside the times: a grouped tick evaluates the policy Rmax times over ALL rows, the separate
runners stop at each cell's own ROLLOUT_LENGTH (``policy_rows_*``: rows x evaluations per tick).
The sides are timed in the same process, interleaved, in three rounds (windows of at most 20 ticks with a synchronisation at both ends); medians are
reported.  Writes profiles/combined/groups_bench.json and prints it as one JSON line.
   usage: python scripts/control_groups_bench.py [--n-per-cell 256 4096] [--cells 1 4 13] [--tick-steps 10] [--tick-warmup 2]
          python scripts/control_groups_bench.py --table     prints the JSON's figures as the table DESIGN section 17 quotes (no GPU needed)"""
import argparse
import json
import os
import sys

from _timing import timed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
KMAX = 16
ACTOR, TRAFFIC, SEED = "medium1", "medium", 1


def tables(result):
    rows = ["| C cells x n per cell | grouped tick | C separate ticks | separate / grouped | separate ticks' spread over rounds | policy rows per tick, grouped / separate |",
            "|---|---|---|---|---|---|"]
    for r in sorted(result["ticks"].values(), key=lambda r: (r["n_per_cell"], r["C"])):
        rows.append("| %d x %d | %.2f ms | %.2f ms | %.2f x | %.1f %% | %d / %d |" % (
            r["C"], r["n_per_cell"], r["grouped_tick_us"] / 1e3, r["separate_ticks_us"] / 1e3, r["speedup"], 100.0 * r["separate_spread"],
            r["policy_rows_grouped"], r["policy_rows_separate"]))
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-per-cell", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--cells", type=int, nargs="+", default=[1, 4, 13])
    ap.add_argument("--tick-steps", type=int, default=10)
    ap.add_argument("--tick-warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "combined", "groups_bench.json"))
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
    from rl_mpc_lanemerging_amd import _capi, actor, combined, combined_bench, episodes
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    pkg.apply_overrides(combined_bench.COMBINED_MEDIUM_1)
    S = pkg.Settings
    dev = torch.device("cuda", torch.cuda.current_device())
    grid = combined.grid_search_cells()
    tr = dict(episodes.TRAFFIC_TYPES[TRAFFIC], seed=SEED)
    result = {"kmax": KMAX, "tick_steps": args.tick_steps, "actor": ACTOR, "traffic": TRAFFIC, "backend": _capi.backend_info(), "ticks": {}}
    med = lambda v: float(np.median(v))
    spread = lambda v: float((max(v) - min(v)) / np.median(v))
    for n in args.n_per_cell:
        for C in args.cells:
            cells = grid[:C]
            gctx = _capi.Context(-1)
            grun = episodes.EpisodeRunner(C * n, controller="combined", policy=actor.ActorPopulation([ACTOR] * C, n, gctx, S), ctx=gctx, kmax=KMAX, traffic=[tr] * C,
                                          control=cells)
            lruns = []
            for cell in cells:                      # the path before groups: the cell's values in the global Settings, one runner and context per cell
                snap = S.snapshot()
                pkg.apply_overrides(cell)
                lctx = _capi.Context(-1)
                lruns.append(episodes.EpisodeRunner(n, controller="combined", policy=actor.DDPGActor(ACTOR, n, lctx, S, dev), ctx=lctx, kmax=KMAX, traffic=[tr]))
                S.restore(snap)

            def lone_ticks():
                for r in lruns:
                    r.tick()

            rounds = {"tick_g": [], "tick_l": []}
            for _ in range(3):
                rounds["tick_g"].append(timed(grun.tick, args.tick_steps, args.tick_warmup, torch))
                rounds["tick_l"].append(timed(lone_ticks, args.tick_steps, args.tick_warmup, torch))
            gctx.check_error()
            for r in lruns:
                r.ctx.check_error()
            lengths = [max(int(c["ROLLOUT_LENGTH"]), 1) for c in cells]
            key = "C%d_n%d" % (C, n)
            result["ticks"][key] = {"C": C, "n_per_cell": n, "rows": C * n, "grouped_tick_us": med(rounds["tick_g"]) * 1e6, "separate_ticks_us": med(rounds["tick_l"]) * 1e6,
                                    "speedup": med(rounds["tick_l"]) / med(rounds["tick_g"]), "grouped_spread": spread(rounds["tick_g"]),
                                    "separate_spread": spread(rounds["tick_l"]), "policy_rows_grouped": max(lengths) * C * n, "policy_rows_separate": sum(lengths) * n,
                                    "rounds_us": {q: [x * 1e6 for x in v] for q, v in rounds.items()}}
            print(key, json.dumps(result["ticks"][key], sort_keys=True), flush=True)
            del grun, lruns
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
