#!/usr/bin/env python3
"""Updates per second of ``DQNLearner`` (20 -> 256 -> 5, B = 50: the shape dqn_bench.py reports) and ``DDPGLearner`` (400 x 300, B = 100) with
``n_step`` in {1, 3, 5}, and of the same two learners in a second checkout of the repository (the parent commit, built: only n_step = 1 exists
there).

A measurement is one child process: a warm-up and ``--repeats`` timed windows of about a second each (``UPDATES`` updates per window), its figure
the median window.  Every configuration is measured in ``--rounds`` processes, and the processes of the configurations ALTERNATE within a round
(the parent and this commit's n_step = 1 next to each other, their order swapped from round to round), so that clock and machine drift fall on
all of them alike.  profiles/learner/nstep_bench.json records, for every configuration, each process's figure, their median and the
process-to-process spread (min, max), the largest within-process spread, and whether this commit's n_step = 1 lies within the parent's spread
(and, one-sided, whether it lies below it).

A child that fails or runs out of time ends the benchmark.
    python scripts/nstep_bench.py [--parent PATH_TO_BUILT_CHECKOUT] [--rounds 5] [--repeats 3]
    python scripts/nstep_bench.py --child dqn|ddpg --n-step N [--tree PATH] --updates U --repeats R      (one measurement, one JSON line)"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UPDATES = {"dqn": 30000, "ddpg": 3000}                             # per timed window: about a second each
N_ENVS, PUSHES, RING = 64, 8, 384                                   # 512 rows into 384: a wrapped ring; 5 * 64 <= 384


def child(kind, n_step, tree, updates, repeats):
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    from rl_mpc_lanemerging_amd import learner
    rng = np.random.default_rng(0)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    kw = {"n_step": n_step} if n_step > 1 else {}                    # (the parent's configs do not know the field)
    if kind == "dqn":
        L = learner.DQNLearner((20, 5), learner.DQNConfig(n_obs=20, n_actions=5, h1=256, batch=50, capacity=RING, **kw), seed=0,
                               **({"rows_per_push": N_ENVS} if n_step > 1 else {}))
    else:
        L = learner.DDPGLearner(20, learner.DDPGConfig(n_obs=20, h1=400, h2=300, batch=100, capacity=RING, replay_start=0, **kw), seed=0,
                                **({"rows_per_push": N_ENVS} if n_step > 1 else {}))
    for _ in range(PUSHES):
        u = rng.random(N_ENVS)
        act = dev(rng.integers(0, 5, N_ENVS).astype(np.int32)) if kind == "dqn" else dev(rng.uniform(-1, 1, N_ENVS))
        L.push(dev(rng.normal(size=(N_ENVS, 20)).astype(np.float32)), dev(rng.integers(0, 200, N_ENVS).astype(np.int32)), act, dev(rng.normal(size=N_ENVS)),
               dev(rng.normal(size=(N_ENVS, 20)).astype(np.float32)), dev(u < 0.02), dev((u >= 0.02) & (u < 0.03)))
    warm = updates // 4 + 1
    L.update(warm)
    torch.cuda.synchronize()
    rates = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        L.update(updates)
        torch.cuda.synchronize()
        rates.append(updates / (time.perf_counter() - t0))
    assert L.stats()["updates"] == warm + updates * repeats
    rates.sort()
    print(json.dumps({"updates_per_s": rates[len(rates) // 2], "min": rates[0], "max": rates[-1], "runs": rates, "updates": updates, "repeats": repeats}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--n-step", type=int, default=1)
    ap.add_argument("--tree", default=REPO)
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--updates", type=int, default=0, help="updates per timed window (default: UPDATES of the learner)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=120)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.n_step, os.path.abspath(args.tree), args.updates or UPDATES[args.child], args.repeats)
    out = {"shapes": {"dqn": "20-256-5, B = 50", "ddpg": "20(+1)-400-300, B = 100"}, "ring": {"rows_per_push": N_ENVS, "capacity": RING},
           "rounds": args.rounds, "windows_per_process": args.repeats, "updates_per_window": UPDATES}
    runs = {}
    for rnd in range(args.rounds):
        for kind in ("dqn", "ddpg"):
            jobs = [("%s_n1" % kind, 1, REPO)]
            if args.parent:
                jobs.append(("%s_parent" % kind, 1, os.path.abspath(args.parent)))
            if rnd % 2:
                jobs.reverse()                                      # who goes first alternates
            jobs += [("%s_n%d" % (kind, n), n, REPO) for n in (3, 5)]
            for key, n, tree in jobs:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--n-step", str(n), "--tree", tree, "--updates",
                                    str(args.updates or UPDATES[kind]), "--repeats", str(args.repeats)], capture_output=True, text=True, timeout=args.timeout)
                if p.returncode != 0:
                    sys.stderr.write(p.stdout + p.stderr)
                    raise SystemExit("the %s measurement of round %d failed (exit %d): nothing more is started" % (key, rnd, p.returncode))
                runs.setdefault(key, []).append(json.loads(p.stdout.strip().splitlines()[-1]))
                print("round %d %-12s %.0f updates/s" % (rnd, key, runs[key][-1]["updates_per_s"]), flush=True)
    for key, rs in runs.items():
        per = sorted(r["updates_per_s"] for r in rs)
        out[key] = {"updates_per_s": per[len(per) // 2], "min": per[0], "max": per[-1], "processes": [r["updates_per_s"] for r in rs],
                    "within_process_spread": max((r["max"] - r["min"]) / r["updates_per_s"] for r in rs)}
    for kind in ("dqn", "ddpg"):
        base = out["%s_n1" % kind]
        for n in (3, 5):
            out["%s_n%d_over_n1" % (kind, n)] = out["%s_n%d" % (kind, n)]["updates_per_s"] / base["updates_per_s"]
        if args.parent:
            par = out["%s_parent" % kind]
            out["%s_n1_over_parent" % kind] = base["updates_per_s"] / par["updates_per_s"]
            out["%s_n1_within_parent_spread" % kind] = bool(par["min"] <= base["updates_per_s"] <= par["max"])
            out["%s_n1_below_parent_spread" % kind] = bool(base["updates_per_s"] < par["min"])      # (above it is no cost)
    path = os.path.join(REPO, "profiles", "learner", "nstep_bench.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
    print(json.dumps({k: v for k, v in out.items() if not isinstance(v, dict)}, sort_keys=True))
    print("wrote", path)


if __name__ == "__main__":
    main()
