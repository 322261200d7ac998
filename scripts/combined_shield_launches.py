#!/usr/bin/env python3
"""The launch sequence of the envs behind the combined controller, for a kernel trace: reset and three steps of vec_env.CombinedShieldVecEnv (the
pretrained ddpg_medium1 actor), then of vec_env.QCombinedShieldVecEnv behind a lone Q-actor and behind a population of two, each at n = 100, the
"default" traffic, shield_kmax 16, the control cell ROLLOUT_LENGTH 3 / ST_TEST_ROLLOUTS 2, fixed actions.  These kernels cost their launch, so two
builds that step at the same speed show the same kernel names in the same order.
   usage: rocprofv3 --kernel-trace -f csv -d DIR -o t -- python scripts/combined_shield_launches.py
          python scripts/combined_shield_launches.py --names <DIR/.../t_kernel_trace.csv>       (the kernel names in start order, one per line)"""
import csv
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
N, KMAX, STEPS, ENV_ID, HIDDEN = 100, 16, 3, "sumo-jerk-v0", 16
CELL = {"ROLLOUT_LENGTH": 3, "ST_TEST_ROLLOUTS": 2}


def names(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    return [r["Kernel_Name"] for r in rows]


def main():
    import numpy as np
    import torch
    import rl_mpc_lanemerging_amd as pkg
    if pkg.build.needs_build():
        raise SystemExit("build the library first (__graft_entry__.build())")
    from rl_mpc_lanemerging_amd import _capi, actor, combined_bench, episodes, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    pkg.apply_overrides(combined_bench.COMBINED_MEDIUM_1)
    pkg.apply_overrides(episodes.TRAFFIC_TYPES["default"])
    S = pkg.Settings
    dev = torch.device("cuda", torch.cuda.current_device())
    table = np.array(vec_env.env_cfg(ENV_ID, "Continuous")._actions, dtype=np.float64)
    tmp = tempfile.mkdtemp()

    def q_actor(ctx, n, seed):
        rng = np.random.default_rng(seed)
        net = {"w0": rng.normal(0, 0.6, (HIDDEN, 20)).astype(np.float32), "b0": rng.normal(0, 0.3, HIDDEN).astype(np.float32),
               "w1": rng.normal(0, 0.6, (table.size, HIDDEN)).astype(np.float32), "b1": rng.normal(0, 0.3, table.size).astype(np.float32)}
        path = os.path.join(tmp, "q%d.npz" % seed)
        with open(path, "wb") as fh:
            np.savez(fh, **net, action_values=table)
        return actor.DQNActor(path, n, ctx, S)
    policies = {"actor": lambda ctx: actor.DDPGActor(combined_bench.COMBINED_MEDIUM_1_ACTOR, N, ctx, S, dev),
                "q-actor": lambda ctx: q_actor(ctx, N, 0),
                "q-population": lambda ctx: actor.QActorPopulation([q_actor(ctx, 1, s) for s in (0, 1)], N // 2, ctx, S)}
    for kind, make in policies.items():
        ctx = _capi.Context(-1)
        if kind == "actor":
            env = vec_env.CombinedShieldVecEnv(N, make(ctx), seed=7, ctx=ctx, shield_kmax=KMAX, control=CELL)
            action = torch.full((N,), 0.5, dtype=torch.float64, device=dev)
        else:
            env = vec_env.QCombinedShieldVecEnv(N, make(ctx), env_id=ENV_ID, seed=7, ctx=ctx, shield_kmax=KMAX, control=CELL)
            action = torch.full((N,), 3, dtype=torch.int32, device=dev)
        env.reset()
        for _ in range(STEPS):
            env.step(action)
        torch.cuda.synchronize()
        env.check_error()
        print(kind, "takeovers", int(env._info["takeover"].sum()), "counts", env.shield_counts(), flush=True)
        ctx.close()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--names":
        print("\n".join(names(sys.argv[2])))
    else:
        main()
