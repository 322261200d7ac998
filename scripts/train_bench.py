#!/usr/bin/env python3
"""Updates/s of the fused DDPG update (learner.DDPGLearner.update, six HIP launches) and frames/s of the whole training loop
(act -> env.step -> push -> one update) at N environments, for several minibatch sizes, next to the torch twin of the same update in eager
PyTorch-ROCm (autograd + torch.optim.Adam + Polyak + index_select sampling) on the same GPU in the same run.  Both sides are timed in windows of
20 calls with a synchronisation at both ends.  Writes profiles/learner/train_bench.json and prints it as one JSON line.
   usage: python scripts/train_bench.py [--n 4096] [--batch 100 1024 4096] [--steps 200] [--warmup 20] [--one-update B]
--one-update B runs a single update of batch B after filling the replay (for a kernel trace: rocprofv3 --kernel-trace --stats -- python ...)."""
import argparse
import json
import os
import sys

from _timing import timed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


class TorchTwin:
    """The same update in eager PyTorch on the device: what a user would write around MergeVecEnv."""

    def __init__(self, torch, cfg, ring, params):
        nn = torch.nn
        self.torch, self.cfg, self.ring = torch, cfg, ring

        def net(p, n_in):
            m = nn.Sequential(nn.Linear(n_in, cfg.h1), nn.ReLU(), nn.Linear(cfg.h1, cfg.h2), nn.ReLU(), nn.Linear(cfg.h2, 1)).cuda()
            with torch.no_grad():
                for lin, (w, b) in zip((m[0], m[2], m[4]), (("w0", "b0"), ("w1", "b1"), ("w2", "b2"))):
                    lin.weight.copy_(torch.as_tensor(p[w])); lin.bias.copy_(torch.as_tensor(p[b]))
            return m
        ns = cfg.n_obs + 1
        self.pi, self.pi_t = net(params["actor"], ns), net(params["actor"], ns)
        self.q, self.q_t = net(params["critic"], ns + 1), net(params["critic"], ns + 1)
        self.opt_q = torch.optim.Adam(self.q.parameters(), lr=cfg.lr_q, betas=(cfg.beta1, cfg.beta2), eps=cfg.eps)
        self.opt_pi = torch.optim.Adam(self.pi.parameters(), lr=cfg.lr_pi, betas=(cfg.beta1, cfg.beta2), eps=cfg.eps)

    def update(self):
        torch, c, ns = self.torch, self.cfg, self.cfg.n_obs + 1
        rows = self.ring.index_select(0, torch.randint(0, self.ring.shape[0], (c.batch,), device="cuda"))
        s, a, s2, r, mask = rows[:, :ns], rows[:, ns:ns + 1], rows[:, 32:32 + ns], rows[:, 64], rows[:, 65]
        squash = lambda z: torch.tanh(z) * c.tanh_scale + c.tanh_mean
        with torch.no_grad():
            y = r + c.gamma * mask * self.q_t(torch.cat([s2, squash(self.pi_t(s2))], 1))[:, 0]
        loss = torch.nn.functional.mse_loss(self.q(torch.cat([s, a], 1))[:, 0], y)
        self.opt_q.zero_grad(); loss.backward(); self.opt_q.step()
        aloss = -self.q(torch.cat([s, squash(self.pi(s))], 1)).mean()
        self.opt_pi.zero_grad(); aloss.backward(); self.opt_pi.step()
        with torch.no_grad():
            for tgt, src in ((self.pi_t, self.pi), (self.q_t, self.q)):
                torch._foreach_mul_(list(tgt.parameters()), 1 - c.tau)
                torch._foreach_add_(list(tgt.parameters()), list(src.parameters()), alpha=c.tau)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--batch", type=int, nargs="+", default=[100, 1024, 4096])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--one-update", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "learner", "train_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import rl_mpc_lanemerging_amd as pkg
    if pkg.build.needs_build():
        raise SystemExit("build the library first (__graft_entry__.build())")
    from rl_mpc_lanemerging_amd import _capi, learner, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    ctx = _capi.default_context()
    env = vec_env.MergeVecEnv(args.n, seed=1, ctx=ctx)
    result = {"n": args.n, "steps": args.steps, "backend": _capi.backend_info(), "batches": {}}
    for B in ([args.one_update] if args.one_update else args.batch):
        cfg = learner.DDPGConfig(n_obs=env.obs_dim, batch=B, capacity=1 << 20, replay_start=0)
        L = learner.DDPGLearner(env, cfg, seed=1)
        state = {"obs": env.reset()}

        def loop_step(update=True, L=L, state=state):
            obs = state["obs"]
            ticks = env.episode_ticks.clone()
            a = L.act(obs, ticks, noise=True)
            nobs, r, term, trunc, info = env.step(a)
            L.push(obs, ticks, a, r, nobs, term, trunc, final_obs=info["final_observation"])
            if update:
                L.update(1)
            state["obs"] = nobs
        for _ in range(40):                                         # fill: 40 N transitions
            loop_step(update=False)
        torch.cuda.synchronize()
        if args.one_update:
            L.update(1)
            torch.cuda.synchronize()
            print(json.dumps({"one_update": B, **L.stats()}))
            return
        sd = L.state_dict()
        fill = int(sd["counters"][1])
        ring = torch.as_tensor(ctx.ddpg_replay_read(L.handle, 0, fill), device="cuda")
        twin = TorchTwin(torch, cfg, ring, sd["params"])
        rounds = {"fused": [], "torch": []}
        for _ in range(3):                                          # interleaved rounds in one process
            rounds["fused"].append(timed(lambda: L.update(1), args.steps, args.warmup, torch))
            rounds["torch"].append(timed(twin.update, args.steps, args.warmup, torch))
        t_loop = timed(loop_step, args.steps, args.warmup, torch)
        t_env = timed(lambda: loop_step(update=False), args.steps, args.warmup, torch)
        env.drain_episode_stats()
        fused, tw = float(np.median(rounds["fused"])), float(np.median(rounds["torch"]))
        result["batches"][str(B)] = {
            "fused_update_us": fused * 1e6, "torch_twin_update_us": tw * 1e6, "fused_updates_per_s": 1 / fused, "torch_twin_updates_per_s": 1 / tw,
            "torch_over_fused": tw / fused, "rounds_us": {k: [x * 1e6 for x in v] for k, v in rounds.items()},
            "loop_step_us": t_loop * 1e6, "loop_frames_per_s": args.n / t_loop, "loop_without_update_step_us": t_env * 1e6,
            "loop_without_update_frames_per_s": args.n / t_env, "stats": L.stats()}
        del L, twin
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
