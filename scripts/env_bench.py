#!/usr/bin/env python3
"""Env-steps/s of the vector environment (vec_env.MergeVecEnv, stmpc_env_step_device) with seeded random continuous actions under
configs/train_moderate_1.json's traffic, next to a bare world tick (stmpc_sim_view_device + stmpc_sim_step_device) of the same N timed in the
same run.  Prints one JSON line.   usage: python scripts/env_bench.py [--n 4096 65536] [--steps 200] [--warmup 20]"""
import argparse
import json
import os
import sys

from _timing import WINDOW, timed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

TRAIN_MODERATE_1 = {"REWARD_FUNCTION": "Slotted Jerk", "ALT_J_WEIGHT": 0.1, "OTHER_CAR_SPEED": 11.0, "BASE_TRAFFIC_INTERVAL": 1.2, "CRASH_MIN_S": 20,
                    "CRASH_REWARD": -10, "SUCCESS_REWARD": 10, "TIME_REWARD": -0.1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import torch
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import _capi, episodes, vec_env
    if pkg.build.needs_build():
        pkg.build.build()
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    pkg.apply_overrides(TRAIN_MODERATE_1)
    ctx = _capi.default_context()
    out = {"metric": "env-steps/s (MergeVecEnv, sumo-jerk-continuous-v0, Slotted Jerk, train_moderate_1 traffic)", "backend": _capi.backend_info(), "runs": []}
    for n in a.n:
        g = torch.Generator(device="cuda")
        g.manual_seed(a.seed)
        env = vec_env.MergeVecEnv(n, seed=a.seed, ctx=ctx)
        env.reset()
        acts = [torch.randn(n, generator=g, device="cuda", dtype=torch.float64) * 3.0 for _ in range(16)]
        i = [0]

        def env_step():
            env.step(acts[i[0] & 15])
            i[0] += 1

        def raw_step():                      # the C-ABI entry alone (what MergeVecEnv.step adds on top: the episode tick counter)
            ctx.env_step(env.params, env.sim_cfg, env.cfg, n, acts[i[0] & 15].data_ptr(), env._obs[0].data_ptr(), env.obs_dim, env._reward.data_ptr(),
                         env._term.data_ptr(), env._trunc.data_ptr(), env._final_obs.data_ptr(), env._final_stats.data_ptr())
            i[0] += 1

        t_env = timed(env_step, a.steps, a.warmup, torch)
        t_raw = timed(raw_step, a.steps, a.warmup, torch)
        st = env.drain_episode_stats()
        # the bare world tick of the same N: sim_view (the planner's Kmax = 32) + sim_step with a fixed command.  Every world must stay live for
        # the whole timed window (a finished world's k_sim_step returns at once): windows of WINDOW ticks from a fresh sim_init (outside the
        # timed region; at 10 m/s an ego covers 40 m of its 260 m ramp in 20 ticks), each checked to end with every status still 0
        ctx_b = _capi.Context(-1)
        cfg = episodes.sim_cfg(a.seed, float(pkg.Settings.MAX_EPISODE_LENGTH))
        K = 32
        z = lambda *s, dtype=torch.float64: torch.zeros(s, dtype=dtype, device="cuda")
        ego5, k, ox, ov, oa, cmd = z(n, 5), z(n, dtype=torch.int32), z(n, K), z(n, K), z(n, K), z(n) + 10.0
        params = _capi.Params.from_settings(pkg.Settings)

        def bare():
            ctx_b.sim_view(cfg, n, K, ego5.data_ptr(), k.data_ptr(), ox.data_ptr(), ov.data_ptr(), oa.data_ptr())
            ctx_b.sim_step(params, cfg, n, cmd.data_ptr())

        st_dev = z(n, dtype=torch.int32)

        def all_live():
            ctx_b.sim_status_device(n, st_dev.data_ptr())
            if int((st_dev != 0).sum()) != 0:
                raise RuntimeError("a bare world finished inside a timed window: the baseline would time idle worlds")

        ctx_b.sim_init(cfg, n)
        t_bare = timed(bare, a.steps, min(a.warmup, WINDOW), torch, before_window=lambda: ctx_b.sim_init(cfg, n), after_window=all_live)
        ctx_b.close()
        out["runs"].append({"n": n, "env_step_ms": 1e3 * t_env, "env_step_capi_ms": 1e3 * t_raw, "bare_view_step_ms": 1e3 * t_bare,
                            "env_steps_per_s": n / t_env, "ratio_env_to_bare": t_env / t_bare, "ratio_capi_to_bare": t_raw / t_bare,
                            "episodes_finished": int(len(st["env"])), "steps": a.steps, "warmup": a.warmup})
        del env
    print(json.dumps(out))


if __name__ == "__main__":
    main()
