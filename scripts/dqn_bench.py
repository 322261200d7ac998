#!/usr/bin/env python3
"""Updates per second of ``learner.DQNLearner`` at the reference's shape (20 -> 256 -> 5, B = 50), with and without prioritised replay, next to the
same update written in eager PyTorch on the same GPU (the yardstick; no ratio is a condition).  Writes profiles/learner/dqn_bench.json.

Each measurement runs in a child process of its own under a time limit; a child that fails or runs out of time ends the benchmark.
    python scripts/dqn_bench.py [--updates 2000] [--repeats 5]
    python scripts/dqn_bench.py --child fused|fused_per|eager --updates N --repeats R      (one measurement, one JSON line)"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
N_OBS, H1, A, B, RING = 20, 256, 5, 50, 256


def _problem():
    import numpy as np
    from rl_mpc_lanemerging_amd import learner
    rng = np.random.default_rng(0)
    net = learner.init_q_net(N_OBS, H1, A, rng)
    replay = {"s": rng.normal(size=(RING, N_OBS)).astype(np.float32), "s2": rng.normal(size=(RING, N_OBS)).astype(np.float32),
              "a": rng.integers(0, A, RING).astype(np.int32), "r": rng.normal(size=RING), "term": rng.random(RING) < 0.1}
    return net, replay


def _median_rate(run, updates, repeats, sync):
    run(updates // 10 + 1)
    sync()
    rates = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        run(updates)
        sync()
        rates.append(updates / (time.perf_counter() - t0))
    rates.sort()
    return {"updates_per_s": rates[len(rates) // 2], "min": rates[0], "max": rates[-1], "updates": updates, "repeats": repeats}


def child(kind, updates, repeats):
    import numpy as np
    import torch
    from rl_mpc_lanemerging_amd import learner
    net, replay = _problem()
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    if kind.startswith("fused"):
        cfg = learner.DQNConfig(n_obs=N_OBS, n_actions=A, h1=H1, batch=B, capacity=RING, per=learner.PERConfig() if kind == "fused_per" else None)
        L = learner.DQNLearner((N_OBS, A), cfg, seed=0, init=net)
        for o in range(0, RING, 64):
            sl = slice(o, o + 64)
            L.push(dev(replay["s"][sl]), None, dev(replay["a"][sl]), dev(replay["r"][sl]), dev(replay["s2"][sl]), dev(replay["term"][sl]),
                   dev(np.zeros(64, dtype=bool)))
        res = _median_rate(lambda n: L.update(n), updates, repeats, torch.cuda.synchronize)
        assert L.stats()["updates"] == (updates // 10 + 1) + updates * repeats
    else:                                                           # dqn.py:322-342 with uniform minibatches, tensors resident on the device
        from torch import nn
        q = nn.Sequential(nn.Linear(N_OBS, H1), nn.ReLU(), nn.Linear(H1, A)).cuda()
        qt = nn.Sequential(nn.Linear(N_OBS, H1), nn.ReLU(), nn.Linear(H1, A)).cuda()
        qt.load_state_dict(q.state_dict())
        opt, crit = torch.optim.Adam(q.parameters(), lr=2e-4), nn.SmoothL1Loss()
        s, s2, a, r = dev(replay["s"]), dev(replay["s2"]), dev(replay["a"].astype(np.int64)), dev(replay["r"].astype(np.float32))
        mask = dev((~replay["term"]).astype(np.float32))
        count = [0]

        def run(n):
            for _ in range(n):
                idx = torch.randint(0, RING, (B,), device="cuda")
                with torch.no_grad():
                    best = torch.argmax(q(s2[idx]), dim=1, keepdim=True)
                    y = r[idx] + mask[idx] * 0.999 * torch.gather(qt(s2[idx]), 1, best).flatten()
                opt.zero_grad()
                loss = crit(torch.gather(q(s[idx]), 1, a[idx][:, None]).flatten(), y)
                loss.backward()
                opt.step()
                count[0] += 1
                if count[0] % 500 == 0:
                    qt.load_state_dict(q.state_dict())
        res = _median_rate(run, updates, repeats, torch.cuda.synchronize)
    res["kind"] = kind
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--updates", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.updates, args.repeats)
    out = {"shape": {"n_obs": N_OBS, "h1": H1, "n_actions": A, "batch": B}}
    for kind in ("fused", "fused_per", "eager"):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--updates", str(args.updates), "--repeats", str(args.repeats)],
                           capture_output=True, text=True, timeout=args.timeout)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit("the %s measurement failed (exit %d): nothing more is started" % (kind, p.returncode))
        out[kind] = json.loads(p.stdout.strip().splitlines()[-1])
        print(kind, "%.0f updates/s" % out[kind]["updates_per_s"], flush=True)
    out["fused_over_eager"] = out["fused"]["updates_per_s"] / out["eager"]["updates_per_s"]
    out["fused_per_over_eager"] = out["fused_per"]["updates_per_s"] / out["eager"]["updates_per_s"]
    from rl_mpc_lanemerging_amd import _capi
    out["backend"] = _capi.backend_info()
    path = os.path.join(REPO, "profiles", "learner", "dqn_bench.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
    print("wrote", path)


if __name__ == "__main__":
    main()
