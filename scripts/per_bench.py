#!/usr/bin/env python3
"""What prioritised replay (learner.PERConfig: a sum tree over the ring, csrc/stmpc_per_kernels.hpp) costs next to uniform minibatches, at the shipped
shape: 21-400-300 networks, B = 100, a ring of 10^6 rows (a tree of 2^21 - 1 nodes), of which the first pushes fill 65536.  Per learner kind (DDPG,
TD3) the uniform and the prioritised learner are timed in the same process, interleaved, in three rounds: updates in windows of ``--steps`` calls of
``update(10)``, pushes in windows of ``--steps`` calls of ``push`` of 4096 rows, a synchronisation at both ends of a window; medians are reported.
A prioritised update is eight launches where the uniform one is six (the sampling step, the priority update); a prioritised push is the same one
launch, whose last workgroup also recomputes the new leaves' ancestors.
Writes profiles/learner/per_bench.json and prints it as one JSON line.
   usage: python scripts/per_bench.py [--steps 100] [--warmup 10]
          python scripts/per_bench.py --profile    one short prioritised DDPG and TD3 run and nothing else (the command a kernel trace is taken of)
          python scripts/per_bench.py --table      prints the JSON's figures as the table DESIGN section 28 quotes (no GPU needed)"""
import argparse
import json
import os
import statistics
import sys

from _timing import timed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
CAPACITY, BATCH, PUSH_N, PREFILL, PER_CALL = 1000000, 100, 4096, 16, 10


def table(result):
    rows = ["| learner | uniform update | prioritised update | ratio | uniform push of 4096 | prioritised push of 4096 | ratio |", "|---|---|---|---|---|---|---|"]
    for kind in ("ddpg", "td3"):
        r = result[kind]
        rows.append("| %s | %.1f us (%.0f / s) | %.1f us (%.0f / s) | %.2f x | %.1f us (%.0f / s) | %.1f us (%.0f / s) | %.2f x |" % (
            kind.upper(), r["update_us"]["uniform"], 1e6 / r["update_us"]["uniform"], r["update_us"]["per"], 1e6 / r["update_us"]["per"], r["update_ratio"],
            r["push_us"]["uniform"], 1e6 / r["push_us"]["uniform"], r["push_us"]["per"], 1e6 / r["push_us"]["per"], r["push_ratio"]))
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "learner", "per_bench.json"))
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--profile", action="store_true")
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
    N = PUSH_N
    rows = (t(rng.normal(0, 1, (N, 20)).astype(np.float32)), t(rng.integers(0, 500, N).astype(np.int32)), t(rng.uniform(-5, 5, N)), t(rng.normal(0, 1, N)),
            t(rng.normal(0, 1, (N, 20)).astype(np.float32)), t(rng.random(N) < 0.05), t(np.zeros(N, bool)))

    def filled(L):
        sd = L.state_dict()                                         # last layers away from zero, so that no pass is degenerate
        for slot, net in sd["params"].items():
            if isinstance(net, dict) and not slot.endswith(("_m", "_v")):
                net["w2"] = rng.normal(0, 0.05, net["w2"].shape).astype(np.float32)
        L.load_state_dict({"params": sd["params"], "counters": None})
        for _ in range(PREFILL):
            L.push(*rows)
        return L

    def legs(kind):
        Cfg, Lrn = (learner.TD3Config, learner.TD3Learner) if kind == "td3" else (learner.DDPGConfig, learner.DDPGLearner)
        kw = dict(n_obs=20, batch=BATCH, capacity=CAPACITY, replay_start=0)
        return {"uniform": filled(Lrn(20, Cfg(**kw), seed=1, ctx=ctx)), "per": filled(Lrn(20, Cfg(per=learner.PERConfig(), **kw), seed=1, ctx=ctx))}

    if args.profile:
        for kind in ("ddpg", "td3"):
            L = legs(kind)["per"]
            L.update(50)
            L.push(*rows)
            torch.cuda.synchronize()
            assert np.isfinite(L.stats()["critic_loss"])
        ctx.check_error()
        return
    result = {"capacity": CAPACITY, "batch": BATCH, "push_rows": PUSH_N, "prefill_rows": PREFILL * PUSH_N, "steps": args.steps, "updates_per_call": PER_CALL,
              "rounds": args.rounds, "tree_nodes": 2 * learner.per_leaves(CAPACITY) - 1, "backend": _capi.backend_info()}
    for kind in ("ddpg", "td3"):
        L = legs(kind)
        upd, psh = {k: [] for k in L}, {k: [] for k in L}
        for _ in range(args.rounds):                                # interleaved: every leg once per round
            for k in L:
                upd[k].append(timed(lambda: L[k].update(PER_CALL), args.steps, args.warmup, torch) / PER_CALL * 1e6)
            for k in L:
                psh[k].append(timed(lambda: L[k].push(*rows), args.steps, args.warmup, torch) * 1e6)
        ctx.check_error()
        r = {"update_us": {k: statistics.median(v) for k, v in upd.items()}, "push_us": {k: statistics.median(v) for k, v in psh.items()},
             "update_rounds_us": upd, "push_rounds_us": psh}
        r["update_ratio"] = r["update_us"]["per"] / r["update_us"]["uniform"]
        r["push_ratio"] = r["push_us"]["per"] / r["push_us"]["uniform"]
        r["updates_per_s"] = {k: 1e6 / v for k, v in r["update_us"].items()}
        r["pushes_per_s"] = {k: 1e6 / v for k, v in r["push_us"].items()}
        tree = L["per"].priorities()
        assert tree[0] > 0 and all(np.isfinite(x.stats()["critic_loss"]) for x in L.values())
        result[kind] = r
        del L
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
