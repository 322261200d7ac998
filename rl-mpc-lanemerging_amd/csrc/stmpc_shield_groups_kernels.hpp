// stmpc_shield_groups_kernels.hpp -- the first-step shield (stmpc_shield_env_kernels.hpp; st.do_conditional_st_based_on_first_step, st.py:805-814) in front
// of the vector environment's group axes: traffic groups (stmpc_sim_groups_kernels.hpp), reward groups (stmpc_env_groups_kernels.hpp) and the traffic
// mix (stmpc_traffic_mix_kernels.hpp).  Nothing in the shield depends on the traffic type or on the reward -- the view, the predictor step, the probe
// and st.do_st_control read the planner's parameters -- so a grouped shielded step is the lone shielded step with a group-aware action stage:
//   k_shield_env_pre_groups      k_shield_env_pre with the world cfg of the environment's traffic group, groups[e / n_per_group];
//   k_shield_env_pre_mix         ... with the cfg of the traffic type the environment's current episode drew (TrafficMix::type[e]);
//   k_shield_env_pre_rg          ... of an ungrouped world, with the invalid-action penalty of the environment's reward group (k_env_act_rg's rule);
//   k_shield_env_pre_rg_groups   both: traffic group = reward group, so one row index selects the world cfg and the penalty;
//   k_shield_env_apply_groups    k_shield_env_apply with the takeover penalty of row e / n_per_penalty of a device table of P values
//                                (P = 1: n_per_penalty = N, one penalty for all; else one per group).
// Every kernel calls the body of its lone twin (shield_env_pre_body, shield_env_apply_body: sim::sim_view_env, handle_action and the takeover branch in its
// operation order -- not copies), between them the body of stmpc_first_step_device runs unchanged on all N rows, and after them the world and post kernels
// of the context's shape: the launch count of the lone shielded step.
// Launch shape of the lone kernels: one thread per environment, 64-thread workgroups, a flat grid over the N rows.  A workgroup spans up to
// 64 / n_per_group + 1 groups, so the group is a per-lane value and the tables are read as stmpc_env_groups_kernels.hpp reads its RewardTab: plain global
// arrays, per-lane (vector) loads after the thread's bounds check (the host has checked N = count * n_per_group, so e / n_per_group < count).  Of the
// group's sim::Cfg only the fields sim_view_env reads are loaded (the copy is a value the compiler takes apart).  No LDS, no atomic; the error word is
// latched with a plain store of 1, as k_env_act latches it.
#pragma once
#include "stmpc_env_groups_kernels.hpp"
#include "stmpc_shield_env_kernels.hpp"
#include "stmpc_traffic_mix_kernels.hpp"

namespace stmpc {
namespace env {

struct PenaltyTab {
    const double *values;                   // device, [P]
    int n_per_penalty;                      // environment e of the world reads values[e / n_per_penalty]
};

#ifdef STMPC_UNIT_ENV        // (the kernels of the unit that launches them)
__global__ void __launch_bounds__(64) k_shield_env_pre_groups(ECfg c, const sim::Cfg *__restrict__ groups, int n_per_group, int N, int kmax, sim::State s, EState es,
                                                              const void *__restrict__ action, ShieldView w) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const sim::Cfg sc = groups[e / n_per_group];
    shield_env_pre_body(c, sc, e, kmax, s, es, action, w);
}

__global__ void __launch_bounds__(64) k_shield_env_pre_mix(ECfg c, sim::Cfg sc, TrafficMix m, int N, int kmax, sim::State s, EState es,
                                                           const void *__restrict__ action, ShieldView w) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    shield_env_pre_body(c, cfg_of_type(sc, m, m.type[e]), e, kmax, s, es, action, w);
}

__global__ void __launch_bounds__(64) k_shield_env_pre_rg(ECfg c, RewardTab tab, sim::Cfg sc, int N, int kmax, sim::State s, EState es,
                                                          const void *__restrict__ action, ShieldView w) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    c.penalty = tab.rows[e / tab.n_per_group].penalty;
    shield_env_pre_body(c, sc, e, kmax, s, es, action, w);
}

// (the host has checked that the reward groups are the traffic groups: tab.n_per_group is the world's n_per_group)
__global__ void __launch_bounds__(64) k_shield_env_pre_rg_groups(ECfg c, RewardTab tab, const sim::Cfg *__restrict__ groups, int N, int kmax, sim::State s, EState es,
                                                                 const void *__restrict__ action, ShieldView w) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const int g = e / tab.n_per_group;
    c.penalty = tab.rows[g].penalty;
    const sim::Cfg sc = groups[g];
    shield_env_pre_body(c, sc, e, kmax, s, es, action, w);
}

__global__ void __launch_bounds__(64) k_shield_env_apply_groups(ECfg c, PenaltyTab pen, int N, sim::State s, EState es, const void *__restrict__ action,
                                                                const double *__restrict__ sh_speed, const int *__restrict__ sh_takeover,
                                                                const int *__restrict__ sh_reason, int *count, int *tag, unsigned char *__restrict__ takeover,
                                                                int *__restrict__ reason, double *__restrict__ exec_jerk, double *__restrict__ exec_action,
                                                                int *__restrict__ takeover_ticks) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    shield_env_apply_body(c, pen.values[e / pen.n_per_penalty], e, s, es, action, sh_speed, sh_takeover, sh_reason, count, tag, takeover, reason, exec_jerk,
                          exec_action, takeover_ticks);
}
#endif

}  // namespace env
}  // namespace stmpc
