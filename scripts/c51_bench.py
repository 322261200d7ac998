#!/usr/bin/env python3
"""Updates per second of ``learner.C51Learner`` at 20 -> 256 -> 5 x 51, B = 50, next to ``learner.DQNLearner`` on the same replay data and to the same
C51 update written in eager PyTorch on the same GPU (yardsticks; no ratio is a condition).  Writes profiles/learner/c51_bench.json.

Each measurement runs in a child process of its own under a time limit; a child that fails or runs out of time ends the benchmark.
    python scripts/c51_bench.py [--updates 2000] [--repeats 5] [--out FILE]
    python scripts/c51_bench.py --child c51|dqn|eager --updates N --repeats R      (one measurement, one JSON line)"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
N_OBS, H1, A, K, B, RING = 20, 256, 5, 51, 50, 256
V_MIN, V_MAX, GAMMA = -10.0, 10.0, 0.999


def _replay():
    import numpy as np
    rng = np.random.default_rng(0)
    return {"s": rng.normal(size=(RING, N_OBS)).astype(np.float32), "s2": rng.normal(size=(RING, N_OBS)).astype(np.float32),
            "a": rng.integers(0, A, RING).astype(np.int32), "r": rng.normal(size=RING), "term": rng.random(RING) < 0.1}


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
    replay = _replay()
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    if kind in ("c51", "dqn"):
        if kind == "c51":
            L = learner.C51Learner((N_OBS, A), learner.C51Config(n_obs=N_OBS, n_actions=A, h1=H1, batch=B, capacity=RING, n_atoms=K, v_min=V_MIN, v_max=V_MAX), seed=0)
        else:
            L = learner.DQNLearner((N_OBS, A), learner.DQNConfig(n_obs=N_OBS, n_actions=A, h1=H1, batch=B, capacity=RING), seed=0)
        for o in range(0, RING, 64):
            sl = slice(o, o + 64)
            L.push(dev(replay["s"][sl]), None, dev(replay["a"][sl]), dev(replay["r"][sl]), dev(replay["s2"][sl]), dev(replay["term"][sl]),
                   dev(np.zeros(64, dtype=bool)))
        res = _median_rate(lambda n: L.update(n), updates, repeats, torch.cuda.synchronize)
        assert L.stats()["updates"] == (updates // 10 + 1) + updates * repeats
    else:                                                           # the same update (double targets, l / u projection by index_add_) with tensors resident on the device
        from torch import nn
        mk = lambda: nn.Sequential(nn.Linear(N_OBS, H1), nn.ReLU(), nn.Linear(H1, A * K)).cuda()
        q, qt = mk(), mk()
        qt.load_state_dict(q.state_dict())
        opt = torch.optim.Adam(q.parameters(), lr=2e-4)
        s, s2, a, r = dev(replay["s"]), dev(replay["s2"]), dev(replay["a"].astype(np.int64)), dev(replay["r"].astype(np.float32))
        mask = dev((~replay["term"]).astype(np.float32))
        z = torch.linspace(V_MIN, V_MAX, K, device="cuda")
        dz = (V_MAX - V_MIN) / (K - 1)
        rows = torch.arange(B, device="cuda")
        count = [0]

        def run(n):
            for _ in range(n):
                idx = torch.randint(0, RING, (B,), device="cuda")
                with torch.no_grad():
                    best = (torch.softmax(q(s2[idx]).view(B, A, K), -1) * z).sum(-1).argmax(1)
                    pn = torch.softmax(qt(s2[idx]).view(B, A, K), -1)[rows, best]
                    b = ((r[idx][:, None] + GAMMA * mask[idx][:, None] * z[None, :]).clamp(V_MIN, V_MAX) - V_MIN) / dz
                    lo, up = b.floor().long(), b.ceil().long()
                    m = torch.zeros(B, K, device="cuda")
                    m.view(-1).index_add_(0, (lo + rows[:, None] * K).view(-1), (pn * (up.float() - b + (lo == up).float())).view(-1))
                    m.view(-1).index_add_(0, (up + rows[:, None] * K).view(-1), (pn * (b - lo.float())).view(-1))
                opt.zero_grad()
                logp = torch.log_softmax(q(s[idx]).view(B, A, K), -1)[rows, a[idx]]
                loss = -(m * logp).sum(-1).mean()
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "learner", "c51_bench.json"))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.updates, args.repeats)
    out = {"shape": {"n_obs": N_OBS, "h1": H1, "n_actions": A, "n_atoms": K, "batch": B}}
    for kind in ("c51", "dqn", "eager"):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--updates", str(args.updates), "--repeats", str(args.repeats)],
                           capture_output=True, text=True, timeout=args.timeout)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit("the %s measurement failed (exit %d): nothing more is started" % (kind, p.returncode))
        out[kind] = json.loads(p.stdout.strip().splitlines()[-1])
        print(kind, "%.0f updates/s" % out[kind]["updates_per_s"], flush=True)
    out["c51_over_eager"] = out["c51"]["updates_per_s"] / out["eager"]["updates_per_s"]
    out["c51_over_dqn"] = out["c51"]["updates_per_s"] / out["dqn"]["updates_per_s"]
    from rl_mpc_lanemerging_amd import _capi
    out["backend"] = _capi.backend_info()
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
