#!/usr/bin/env python3
"""What the first-step shield controller (st.do_conditional_st_based_on_first_step, st.py:805-814: csrc/stmpc_fs_kernels.hpp, first_step.py) costs per
tick next to the combined controller (dqn.RLAgent.do_combined_control) on the SAME states: N = 4096 tick states of combined_bench.bench_states at
Kmax = 8 with the reference's ddpg_medium1 actor under configs/combined_medium_1.json, both with sparse_control as the episode runner uses them.
A first-step tick is one actor launch, control.get_ego_speed_from_jerk, one predictor step, the feasibility probe's solve and the controller's solve of
the taken-over states; a combined tick is ROLLOUT_LENGTH = 5 actor launches and rollout steps, then the same two solves.  Every timed tick is the same
tick of the same episodes (the evaluation counters are restored before each).
The sides are timed in the same process, interleaved, in three rounds (windows of at most 20 ticks with a synchronisation at both ends); medians are
reported.  Writes profiles/combined/first_step_bench.json and prints it as one JSON line.
   usage: python scripts/first_step_bench.py [--n 4096] [--tick-steps 20] [--tick-warmup 3]
          python scripts/first_step_bench.py --table     prints the JSON's figures as the table DESIGN section 18 quotes (no GPU needed)"""
import argparse
import json
import os
import sys

from _timing import timed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
SEED = 3000


def tables(result):
    r = result
    rows = ["| N | first-step tick | combined tick | combined / first-step | spread over rounds, first-step / combined | taken over, first-step / combined | controller solves per tick, first-step / combined |",
            "|---|---|---|---|---|---|---|"]
    rows.append("| %d | %.2f ms (%.0f ticks/s) | %.2f ms (%.0f ticks/s) | %.2f x | %.1f %% / %.1f %% | %d / %d | %d / %d |" % (
        r["n"], r["first_step_tick_us"] / 1e3, r["first_step_ticks_per_s"], r["combined_tick_us"] / 1e3, r["combined_ticks_per_s"], r["speedup"],
        100.0 * r["first_step_spread"], 100.0 * r["combined_spread"], r["first_step_takeovers"], r["combined_takeovers"], r["first_step_control_solves"],
        r["combined_control_solves"]))
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--tick-steps", type=int, default=20)
    ap.add_argument("--tick-warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "combined", "first_step_bench.json"))
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
    from rl_mpc_lanemerging_amd import _capi, actor, combined, combined_bench, first_step
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    pkg.apply_overrides(combined_bench.COMBINED_MEDIUM_1)
    S = pkg.Settings
    dev = torch.device("cuda", torch.cuda.current_device())
    n = args.n
    params = _capi.Params.from_settings(S)
    ego, kc, ox, ov, evals0 = combined_bench.bench_states(n, SEED, S)
    d_ego, d_k = torch.as_tensor(ego, device=dev), torch.as_tensor(kc, device=dev)
    d_ox, d_ov, d_oa = torch.as_tensor(ox, device=dev), torch.as_tensor(ov, device=dev), torch.zeros(ox.shape, dtype=torch.float64, device=dev)
    d_evals0 = torch.as_tensor(evals0, device=dev)
    # a context each: the two controllers keep their scratch apart, as two runners would
    fctx, cctx = _capi.Context(-1), _capi.Context(-1)
    fpol = actor.DDPGActor(combined_bench.COMBINED_MEDIUM_1_ACTOR, n, fctx, S, dev)
    cpol = actor.DDPGActor(combined_bench.COMBINED_MEDIUM_1_ACTOR, n, cctx, S, dev)
    fs = first_step.FirstStepController(n, fctx, params, sparse_control=True)
    ccfg = _capi.CombinedCfg.from_settings(S, sparse_control=True)
    cur_ego4 = torch.zeros(n, 4, dtype=torch.float64, device=dev)
    last = {}

    def first_step_tick():
        fpol.evals.copy_(d_evals0)
        cur_ego4.copy_(d_ego[:, :4])
        jerk = fpol(1, cur_ego4, d_k, d_ox, d_ov, d_oa)
        last["f"] = fs.decide_jerk(d_ego, d_k, d_ox, d_ov, jerk, d_oa)

    def combined_tick():
        cpol.evals.copy_(d_evals0)
        last["c"] = combined.decide_batch_device(cctx, params, ccfg, d_ego, d_k, d_ox, d_ov, cpol, None, d_oa=d_oa)

    rounds = {"f": [], "c": []}
    for _ in range(3):
        rounds["f"].append(timed(first_step_tick, args.tick_steps, args.tick_warmup, torch))
        rounds["c"].append(timed(combined_tick, args.tick_steps, args.tick_warmup, torch))
    fctx.check_error()
    cctx.check_error()
    # the work of ONE tick of each side, from the contexts' own counters
    fctx.first_step_counts(reset=True)
    cctx.combined_counts(reset=True)
    first_step_tick()
    combined_tick()
    torch.cuda.synchronize()
    f_dec, f_take, f_solves = fctx.first_step_counts()
    c_dec, c_solves = cctx.combined_counts()
    med = lambda v: float(np.median(v))
    spread = lambda v: float((max(v) - min(v)) / np.median(v))
    result = {"n": n, "kmax": int(ox.shape[1]), "tick_steps": args.tick_steps, "actor": "ddpg_medium1", "state_seed": SEED, "backend": _capi.backend_info(),
              "rollout_length": int(S.ROLLOUT_LENGTH), "first_step_tick_us": med(rounds["f"]) * 1e6, "combined_tick_us": med(rounds["c"]) * 1e6,
              "first_step_ticks_per_s": 1.0 / med(rounds["f"]), "combined_ticks_per_s": 1.0 / med(rounds["c"]), "speedup": med(rounds["c"]) / med(rounds["f"]),
              "first_step_spread": spread(rounds["f"]), "combined_spread": spread(rounds["c"]), "first_step_decisions": f_dec, "first_step_takeovers": f_take,
              "first_step_control_solves": f_solves, "combined_decisions": c_dec, "combined_takeovers": int(last["c"]["takeover"].sum().item()),
              "combined_control_solves": c_solves, "rounds_us": {q: [x * 1e6 for x in v] for q, v in rounds.items()}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
