#!/usr/bin/env python3
"""What one TD3 update (learner.TD3Learner: both critics in blockIdx.y of one launch sequence) costs next to the DDPG update of the same learner
shapes (21-400-300 networks), at minibatch sizes B and policy delays d, on a ring of 4096 synthetic rows.  The two learners are timed in the same
process, interleaved, in three rounds (windows of 20 calls of ``update(10)`` with a synchronisation at both ends); medians are reported, per update.
A TD3 learner whose delay is never due runs both critics and finds its other three launches empty: TD3's critic half.  From it, the actor half
is (TD3 at delay 1) - (critic half), DDPG's one-critic half is (DDPG) - (actor half), and ``second_critic_share`` = ((TD3 at delay 1) - (DDPG)) /
(DDPG's critic half): what the second critic adds, as a share of one more critic pass.  The JSON carries every raw figure.
Writes profiles/learner/td3_bench.json and prints it as one JSON line.
   usage: python scripts/td3_bench.py [--batch 100 1024] [--delay 1 2] [--steps 100] [--warmup 10]
          python scripts/td3_bench.py --table     prints the JSON's figures as the table DESIGN section 26 quotes (no GPU needed)"""
import argparse
import json
import os
import statistics
import sys

from _timing import timed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
RING, PER_CALL, NEVER = 4096, 10, 1 << 30


def table(result):
    rows = ["| B | DDPG update | TD3, delay 1 | TD3, delay 2 | critics only (delay never due) | TD3 delay 1 / DDPG | second critic, share of one more critic pass |", "|---|---|---|---|---|---|---|"]
    for r in sorted(result["shapes"].values(), key=lambda r: r["batch"]):
        rows.append("| %d | %.1f us | %.1f us | %.1f us | %.1f us | %.2f x | %.2f |" % (
            r["batch"], r["ddpg_us"], r["td3_us"]["1"], r["td3_us"].get("2", float("nan")), r["td3_critics_only_us"], r["td3_us"]["1"] / r["ddpg_us"],
            r["second_critic_share"]))
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[100, 1024])
    ap.add_argument("--delay", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "learner", "td3_bench.json"))
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
    from rl_mpc_lanemerging_amd import _capi, learner
    ctx = _capi.default_context()
    rng = np.random.default_rng(0)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    rows = (t(rng.normal(0, 1, (RING, 20)).astype(np.float32)), t(rng.integers(0, 500, RING).astype(np.int32)), t(rng.uniform(-5, 5, RING)), t(rng.normal(0, 1, RING)),
            t(rng.normal(0, 1, (RING, 20)).astype(np.float32)), t(rng.random(RING) < 0.05), t(np.zeros(RING, bool)))

    def filled(L):
        sd = L.state_dict()                                         # last layers away from zero, so that no pass is degenerate
        for slot, net in sd["params"].items():
            if isinstance(net, dict) and not slot.endswith(("_m", "_v")):
                net["w2"] = rng.normal(0, 0.05, net["w2"].shape).astype(np.float32)
        L.load_state_dict({"params": sd["params"], "counters": None})
        L.push(*rows)
        return L

    result = {"ring": RING, "steps": args.steps, "updates_per_call": PER_CALL, "rounds": args.rounds, "backend": _capi.backend_info(), "shapes": {}}
    for B in args.batch:
        kw = dict(n_obs=20, batch=B, capacity=RING, replay_start=0)
        legs = {"ddpg": filled(learner.DDPGLearner(20, learner.DDPGConfig(**kw), seed=1, ctx=ctx))}
        for d in list(args.delay) + [NEVER]:
            legs["td3_%d" % d] = filled(learner.TD3Learner(20, learner.TD3Config(policy_delay=d, **kw), seed=1, ctx=ctx))
        times = {k: [] for k in legs}
        for _ in range(args.rounds):                                # interleaved: every leg once per round
            for k, L in legs.items():
                times[k].append(timed(lambda: L.update(PER_CALL), args.steps, args.warmup, torch) / PER_CALL * 1e6)
        ctx.check_error()
        med = {k: statistics.median(v) for k, v in times.items()}
        r = {"batch": B, "ddpg_us": med["ddpg"], "td3_us": {str(d): med["td3_%d" % d] for d in args.delay}, "td3_critics_only_us": med["td3_%d" % NEVER],
             "rounds_us": times}
        d1 = med["td3_%d" % args.delay[0]]
        r["actor_half_us"] = d1 - med["td3_%d" % NEVER]
        r["ddpg_critic_half_us"] = med["ddpg"] - r["actor_half_us"]
        r["second_critic_share"] = (d1 - med["ddpg"]) / r["ddpg_critic_half_us"]
        result["shapes"][str(B)] = r
        for L in legs.values():
            assert np.isfinite(L.stats()["critic_loss"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
