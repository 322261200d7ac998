// stmpc_env_groups_kernels.hpp -- reward groups: one vector environment of R groups of n_per_group consecutive environments, each group rewarded under its
// own settings, in the launches of a lone env.  The reference treats the reward as a per-run setting -- dqn.get_reward_function (dqn.py:449-460) picks
// one of four functions, every file under its configs/ overrides their weights, merge_gym.py:25 adds INVALID_ACTION_PENALTY -- and compares rewards by
// one TRAIN_DDPG run per setting; here the envs of several settings are stepped side by side.
//
// Every kernel is the arithmetic of its lone twin in stmpc_env_kernels.hpp (env_act_body, env_post_body, reward -- called, not copied)
// on an ECfg whose reward fields come from row e / n_per_group of a device table of RewardRow, e the environment's row in the world:
//   k_env_act_rg          k_env_act with the row's invalid-action penalty;
//   k_env_post_rg         k_env_post (an ungrouped world);
//   k_env_post_rg_groups  k_env_post_groups (a world of traffic groups; reward group = traffic group, so the row is blockIdx.y's, looked up the same way);
//   k_env_reward_rg       k_env_reward.
// k_env_reset / k_env_reset_groups read no field that may differ between reward groups (the observation has none) and serve a grouped env unchanged.
// Launch shape of the lone env: 64-thread workgroups, one thread per environment, a flat grid over the N rows of an ungrouped world.  A workgroup there
// spans up to 64 / n_per_group + 1 groups, so the row index is a per-thread value and the table is a plain global array read with per-lane (vector)
// loads, after the thread's bounds check: a table in the kernel arguments or in constant memory comes in through scalar loads, which need one
// address per wavefront -- a per-lane index into it would make the compiler copy the struct array to scratch or loop over the lanes' distinct values.
// The table is at most 64 rows of 112 bytes: after the first wavefront it is served from the L2 / vector L1 of every compute unit.
// Nothing else differs between groups: the action mode and table, the tick, the limits, the car length, autoreset, the log and the observation are the
// shared ECfg's, which the host has checked to be equal.
#pragma once
#include "stmpc_sim_groups_kernels.hpp"

namespace stmpc {
namespace env {

struct RewardRow {                          // what may differ between reward groups (stmpc_env_cfg's fields of the same names)
    double crash_r, success_r, time_r, wt_smooth, wt_safe, wt_eff, alt_v, alt_a, alt_j, alt_d, min_follow, desired_speed, penalty;
    int reward, pad;
};
struct RewardTab {
    const RewardRow *rows;                  // device, [R]
    int n_per_group;                        // environment e of the world reads rows[e / n_per_group]
};

// the shared cfg with the reward settings of world row `e` (e < R * n_per_group: the caller has checked its bounds)
__device__ __forceinline__ ECfg cfg_of_row(const ECfg &c, const RewardTab &t, int e) {
    const RewardRow r = t.rows[e / t.n_per_group];
    ECfg o = c;
    o.crash_r = r.crash_r; o.success_r = r.success_r; o.time_r = r.time_r; o.wt_smooth = r.wt_smooth; o.wt_safe = r.wt_safe; o.wt_eff = r.wt_eff;
    o.alt_v = r.alt_v; o.alt_a = r.alt_a; o.alt_j = r.alt_j; o.alt_d = r.alt_d; o.min_follow = r.min_follow; o.desired_speed = r.desired_speed;
    o.penalty = r.penalty; o.reward = r.reward;
    return o;
}

#ifdef STMPC_UNIT_ENV        // (the kernels of the unit that launches them)
// k_env_act with the penalty of the environment's reward group (the only field of the action handling that may differ)
__global__ void __launch_bounds__(64) k_env_act_rg(ECfg c, RewardTab tab, int N, sim::State s, EState es, const void *__restrict__ action) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const int live = s.status[e] == 0;
    es.live[e] = live;
    if (!live) return;
    c.penalty = tab.rows[e / tab.n_per_group].penalty;
    env_act_body(c, e, s, es, action);
}

__global__ void __launch_bounds__(64) k_env_post_rg(ECfg c, RewardTab tab, sim::Cfg sc, int N, sim::State s, EState es, float *__restrict__ obs, int obs_stride,
                                                    double *__restrict__ rew, unsigned char *__restrict__ term, unsigned char *__restrict__ trunc,
                                                    float *__restrict__ final_obs, double *__restrict__ final_stats) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const ECfg ce = cfg_of_row(c, tab, e);
    env_post_body(ce, sc, c.seed, 0, N, s, es, obs, obs_stride, rew, term, trunc, final_obs, final_stats);
}

// obs, rew, term, trunc, final_obs and final_stats have G * n_per_group rows; the host has checked that the reward groups are the traffic groups
__global__ void __launch_bounds__(64) k_env_post_rg_groups(ECfg c, RewardTab tab, const sim::Cfg *__restrict__ groups, int n_per_group, sim::State s, EState es,
                                                           float *__restrict__ obs, int obs_stride, double *__restrict__ rew, unsigned char *__restrict__ term,
                                                           unsigned char *__restrict__ trunc, float *__restrict__ final_obs, double *__restrict__ final_stats) {
    const int local = blockIdx.x * blockDim.x + threadIdx.x;
    if (local >= n_per_group) return;
    const sim::Cfg sc = groups[blockIdx.y];
    const int row0 = (int)blockIdx.y * n_per_group;
    const size_t off = (size_t)row0;
    const ECfg ce = cfg_of_row(c, tab, row0 + local);
    env_post_body(ce, sc, sc.seed, row0, n_per_group, sim::state_slice(s, off), estate_slice(es, off), obs + off * obs_stride, obs_stride, rew + off, term + off,
                  trunc + off, final_obs ? final_obs + off * obs_stride : nullptr, final_stats ? final_stats + off * NSTAT : nullptr);
}

__global__ void __launch_bounds__(64) k_env_reward_rg(ECfg c, RewardTab tab, int N, int Kmax, const double *__restrict__ ego4, const int *__restrict__ k,
                                                      const double *__restrict__ ox, const double *__restrict__ jerk, const int *__restrict__ crashed,
                                                      const int *__restrict__ arrived, double *__restrict__ out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const ECfg ce = cfg_of_row(c, tab, e);
    int n = k[e];
    n = n < 0 ? 0 : (n > Kmax ? Kmax : n);
    out[e] = reward(ce, ego4[(size_t)e * 4 + 0], ego4[(size_t)e * 4 + 1], ego4[(size_t)e * 4 + 2], ego4[(size_t)e * 4 + 3], ox + (size_t)e * Kmax, n, jerk[e],
                    crashed && crashed[e] != 0, arrived && arrived[e] != 0);
}
#endif

}  // namespace env
}  // namespace stmpc
