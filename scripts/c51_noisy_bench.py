#!/usr/bin/env python3
"""Updates per second and acting time of ``learner.C51Learner`` with and without the noisy output layer (``C51Config(noisy=NoisyConfig())``), plain
and dueling head, at the shipped shape 20 -> 256 -> 5 x 51 (B = 50, as scripts/c51_dueling_bench.py).  A noisy leg's acting time is a noisy ``act()``:
the acting draw's compose and the act kernel.  With ``--parent-tree`` the plain learner is also timed in a built checkout of the parent commit, the two
trees' legs interleaved (parent, this, parent, this, ...) in one session: the plain path's median must lie within the spread of the parent's own
repeats.  The noisy legs are recorded without a pass mark.  Writes profiles/learner/c51_noisy_bench.json.

Each leg runs in a child process of its own under a time limit; a child that fails or runs out of time ends the benchmark.
    python scripts/c51_noisy_bench.py [--parent-tree DIR] [--updates 2000] [--repeats 5] [--out FILE]
    python scripts/c51_noisy_bench.py --child plain|noisy|dueling|noisy_dueling --tree DIR --updates N      (one leg, one JSON line)"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"shipped": (20, 256, 5, 51, 50)}      # (n_obs, h1, A, K, B)
RING, N_ACT = 256, 1024


def child(kind, shape, tree, updates):
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import numpy as np
    import torch
    from _timing import timed
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, A, K, B = SHAPES[shape]
    rng = np.random.default_rng(0)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    kw = dict(dueling=True) if "dueling" in kind else {}
    if "noisy" in kind:                                             # (the parent's C51Config does not take the key)
        kw["noisy"] = learner.NoisyConfig()
    L = learner.C51Learner((n_obs, A), learner.C51Config(n_obs=n_obs, n_actions=A, h1=h1, batch=B, capacity=RING, n_atoms=K, **kw), seed=0)
    for o in range(0, RING, 64):
        L.push(dev(rng.normal(size=(64, n_obs)).astype(np.float32)), None, dev(rng.integers(0, A, 64).astype(np.int32)), dev(rng.normal(size=64)),
               dev(rng.normal(size=(64, n_obs)).astype(np.float32)), dev(rng.random(64) < 0.1), dev(np.zeros(64, dtype=bool)))
    per_update = timed(lambda: L.update(1), updates, updates // 10 + 1, torch)
    obs = dev(rng.normal(size=(N_ACT, n_obs)).astype(np.float32))
    per_act = timed(lambda: L.act(obs, None, eps=0.0), 400, 40, torch)
    assert L.stats()["updates"] == updates + updates // 10 + 1
    print(json.dumps({"kind": kind, "shape": shape, "updates_per_s": 1.0 / per_update, "act_us": per_act * 1e6, "act_rows": N_ACT, "updates": updates}))


def leg(kind, shape, tree, updates, timeout):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--shape", shape, "--tree", tree, "--updates", str(updates)],
                       capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit("the %s %s leg in %s failed (exit %d): nothing more is started" % (kind, shape, tree, p.returncode))
    return json.loads(p.stdout.strip().splitlines()[-1])


def series(legs):
    rates = sorted(r["updates_per_s"] for r in legs)
    acts = sorted(r["act_us"] for r in legs)
    return {"updates_per_s": [r["updates_per_s"] for r in legs], "median_updates_per_s": rates[len(rates) // 2], "min": rates[0], "max": rates[-1],
            "act_us": [r["act_us"] for r in legs], "median_act_us": acts[len(acts) // 2]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--shape", default="shipped")
    ap.add_argument("--tree", default=REPO)
    ap.add_argument("--parent-tree")
    ap.add_argument("--updates", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "learner", "c51_noisy_bench.json"))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.shape, args.tree, args.updates)
    out = {"shapes": {k: dict(zip(("n_obs", "h1", "n_actions", "n_atoms", "batch"), v)) for k, v in SHAPES.items()}, "act_rows": N_ACT}
    raw = {"parent_plain": [], "plain": []}
    for rep in range(args.repeats):                                 # interleaved: parent, this, parent, this, ...
        if args.parent_tree:
            raw["parent_plain"].append(leg("plain", "shipped", os.path.abspath(args.parent_tree), args.updates, args.timeout))
        raw["plain"].append(leg("plain", "shipped", REPO, args.updates, args.timeout))
        print("repeat", rep, " ".join("%s %.0f/s" % (k, v[-1]["updates_per_s"]) for k, v in raw.items() if v), flush=True)
    out["plain_shipped"] = series(raw["plain"])
    if args.parent_tree:
        out["parent_plain_shipped"] = series(raw["parent_plain"])
        par, med = out["parent_plain_shipped"], out["plain_shipped"]["median_updates_per_s"]
        out["plain_within_parent_spread"] = bool(par["min"] <= med <= par["max"] or med >= par["max"])
    for kind, shape in (("noisy", "shipped"), ("dueling", "shipped"), ("noisy_dueling", "shipped")):
        out["%s_%s" % (kind, shape)] = series([leg(kind, shape, REPO, args.updates, args.timeout) for _ in range(3)])
        print(kind, shape, "%.0f updates/s" % out["%s_%s" % (kind, shape)]["median_updates_per_s"], flush=True)
    sys.path.insert(0, REPO)
    from rl_mpc_lanemerging_amd import _capi
    out["backend"] = _capi.backend_info()
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
    print("wrote", args.out)
    if args.parent_tree and not out["plain_within_parent_spread"]:
        raise SystemExit("the plain path's median %.0f updates/s is below the parent's spread %.0f ... %.0f" % (med, par["min"], par["max"]))


if __name__ == "__main__":
    main()
