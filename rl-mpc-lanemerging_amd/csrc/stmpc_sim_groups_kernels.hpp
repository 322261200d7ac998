// stmpc_sim_groups_kernels.hpp -- traffic groups in the batched world: G groups of n_per_group consecutive environments, each with its own sim::Cfg, in the
// launches of an ungrouped world.  The reference varies its experiments along exactly this axis: configs/{train,combined,cross,ddpg}_*.json differ in
// BASE_TRAFFIC_INTERVAL and OTHER_CAR_SPEED (the highway flow of control.py:215-226) and are run one process per traffic type; here the worlds of several
// traffic types are stepped, used as one vector environment (merge_gym.py) and reset side by side.
//
// Every entry is the body of its single-cfg kernel (sim_init_body / sim_step_body of stmpc_cc_kernels.hpp, env_post_body / env_reset_body of
// stmpc_env_kernels.hpp -- not a copy) on the cfg blockIdx.y selects from a device table of sim::Cfg.  blockIdx.y is wave-uniform and the table is read
// before the workgroup's first store, so the struct comes in through scalar loads like the by-value argument it replaces.  Workgroup (x, g) serves local
// rows [64 x, 64 x + 64) of group g: a workgroup never spans two groups and a group's tail lanes are masked as a lone world of n_per_group environments
// masks them.  The body sees the group's slice of every [N]... array (state_slice / estate_slice and the step tensors moved on by g * n_per_group rows),
// so its environment index is the LOCAL row: the random draws (uniform01(seed, env, ctr), cruise_speed, episode_seed / episode_ctr of the autoreset) are
// those of the lone world made from groups[g], while the state lives at the global row g * n_per_group + local.  Shared by all groups: the episode log
// with its slot counter (a row's environment column holds the global row), the error word and the action table.
// k_sim_view and k_env_act read nothing that may differ between groups (sensor_radius; ECfg) and serve a grouped world unchanged with N = G * n_per_group.
#pragma once
#include "stmpc_env_kernels.hpp"

namespace stmpc {
namespace sim {

#ifdef STMPC_UNIT_ENV        // (the kernels of the unit that launches them)
__global__ void __launch_bounds__(64) k_sim_init_groups(const Cfg *__restrict__ groups, int n_per_group, State s) {
    const Cfg c = groups[blockIdx.y];
    sim_init_body(c, n_per_group, state_slice(s, (size_t)blockIdx.y * n_per_group));
}

__global__ void __launch_bounds__(64) k_sim_step_groups(DevP p, const Cfg *__restrict__ groups, int n_per_group, State s, const double *__restrict__ cmd_speed,
                                                        double crash_min_s) {
    const Cfg c = groups[blockIdx.y];
    const size_t off = (size_t)blockIdx.y * n_per_group;
    sim_step_body(p, c, n_per_group, state_slice(s, off), cmd_speed + off, crash_min_s);
}
#endif

}  // namespace sim

namespace env {

#ifdef STMPC_UNIT_ENV        // (the kernels of the unit that launches them)
// obs, rew, term, trunc, final_obs and final_stats have G * n_per_group rows
__global__ void __launch_bounds__(64) k_env_post_groups(ECfg c, const sim::Cfg *__restrict__ groups, int n_per_group, sim::State s, EState es, float *__restrict__ obs,
                                                        int obs_stride, double *__restrict__ rew, unsigned char *__restrict__ term, unsigned char *__restrict__ trunc,
                                                        float *__restrict__ final_obs, double *__restrict__ final_stats) {
    const sim::Cfg sc = groups[blockIdx.y];
    const int row0 = (int)blockIdx.y * n_per_group;
    const size_t off = (size_t)row0;
    env_post_body(c, sc, sc.seed, row0, n_per_group, sim::state_slice(s, off), estate_slice(es, off), obs + off * obs_stride, obs_stride, rew + off, term + off,
                  trunc + off, final_obs ? final_obs + off * obs_stride : nullptr, final_stats ? final_stats + off * NSTAT : nullptr);
}

__global__ void __launch_bounds__(64) k_env_reset_groups(ECfg c, const sim::Cfg *__restrict__ groups, int n_per_group, sim::State s, EState es, float *__restrict__ obs,
                                                         int obs_stride) {
    const sim::Cfg sc = groups[blockIdx.y];
    const size_t off = (size_t)blockIdx.y * n_per_group;
    env_reset_body(c, sc, n_per_group, sim::state_slice(s, off), estate_slice(es, off), obs ? obs + off * obs_stride : nullptr, obs_stride);
}
#endif

}  // namespace env
}  // namespace stmpc
