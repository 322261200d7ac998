// stmpc_shield_env_kernels.hpp -- the vector environment stepped behind the first-step shield (st.do_conditional_st_based_on_first_step, st.py:805-814):
// the env's action is a PROPOSAL, the shield decides what is executed, and the learner is told.  One step is
//   k_shield_env_pre     the env's action handling (k_env_act's, through the same device functions) + the planner's view of the current state
//                        (sim::k_sim_view's body, called) + the proposed speed, in one launch instead of three;
//   the body of stmpc_first_step_device on that view and proposal (stmpc_fs_kernels.hpp and the batched solves, shared, not copied);
//   k_shield_env_apply   where the shield took over: the executed speed, the projected jerk of that speed, the takeover penalty; for every
//                        environment what was executed and the takeovers of its episode so far;
//   sim::k_sim_step and env::k_env_post, unchanged.
// One thread per environment, 64-thread workgroups, a flat grid over the N rows: the lone env's launch shape.  Every per-environment value is a
// per-lane value read and written with plain vector loads and stores after the thread's bounds check; there is no per-block index or table, no
// LDS and no atomic (the error word is latched with a plain store of 1, as k_env_act latches it).  Both kernels are a few dozen fp64 operations per
// lane next to the solves between them: their cost is their launch, so nothing here is tuned for occupancy beyond the 64-thread workgroup that
// keeps one wavefront per workgroup and lets N = 96 fill a second, partial one.
#pragma once
#include "stmpc_env_kernels.hpp"

namespace stmpc {
namespace env {

struct ShieldView {                         // device arrays: the planner's view handed to the shield (the layout stmpc_first_step_device takes)
    double *ego5;                           // [N][5]
    int *k;                                 // [N]
    double *ox, *ov;                        // [N][kmax]
    double *proposal;                       // [N] the proposed speed
};

// k_env_act's dispatch (handle_action, called) + the shield's view and proposal, for environment e (e < N: the caller has checked its bounds) under
// the env cfg `c` and the world cfg `sc` of that environment -- the body of k_shield_env_pre and of its grouped forms
// (stmpc_shield_groups_kernels.hpp).  A finished environment gets the view k_sim_view
// gives it and proposes the speed its action would command from that state -- what episodes.EpisodeRunner(controller="first_step") proposes for a
// finished environment, so that the context's stmpc_first_step_counts are the runner's row for row -- while its step state is left alone, as
// k_env_act leaves it.  An index out of range latches the error word as k_env_act does (a running environment's only) and proposes -- and
// commands -- the current speed, which is what sim::k_sim_step makes of k_env_act's NaN command, so that no NaN reaches the predictor or the solver.
__device__ __forceinline__ void shield_env_pre_body(const ECfg &c, const sim::Cfg &sc, int e, int kmax, const sim::State &s, const EState &es,
                                                    const void *__restrict__ action, const ShieldView &w) {
    sim::sim_view_env(sc, kmax, s, e, w.ego5, w.k, w.ox, w.ov, nullptr);
    const int live = s.status[e] == 0;
    es.live[e] = live;
    const double v = s.ego4[e * 4 + 2], a = s.ego4[e * 4 + 3], prev_a = es.prev_a[e];
    double pjerk, inv, cmd;
    if (handle_action(c, action, e, v, a, prev_a, cmd, pjerk, inv)) {
        if (live) es.err[0] = 1u;
        cmd = v;
    }
    w.proposal[e] = cmd;
    if (!live) return;                                                     // (k_sim_step idles finished environments)
    es.cmd[e] = cmd; es.pjerk[e] = pjerk; es.inv[e] = inv;
}

// After the shield's decision (sh_*: k_fs_decide's outputs for the N rows), for environment e (e < N) -- the body of k_shield_env_apply and of
// k_shield_env_apply_groups.  Where it took over a live environment: the command becomes the
// shield's speed, the projected jerk that of the executed speed -- the third branch of AccelerationEnv._do_action (merge_gym.py:208-212) in
// exactly this operation order -- and the tick's invalid-action reward grows by takeover_penalty * tick.  count / tag: the takeovers of the
// environment's current episode and the episode they were counted in; the count restarts when es.episode[e] has moved on (k_env_post's autoreset),
// so the value written on the tick an episode ends is still that episode's.  exec_action may be NULL (discrete envs: the index is not rewritten).
__device__ __forceinline__ void shield_env_apply_body(const ECfg &c, double takeover_penalty, int e, const sim::State &s, const EState &es,
                                                      const void *__restrict__ action, const double *__restrict__ sh_speed,
                                                      const int *__restrict__ sh_takeover, const int *__restrict__ sh_reason, int *count, int *tag,
                                                      unsigned char *__restrict__ takeover, int *__restrict__ reason, double *__restrict__ exec_jerk,
                                                      double *__restrict__ exec_action, int *__restrict__ takeover_ticks) {
    const int ep = es.episode[e];
    int cnt = tag[e] == ep ? count[e] : 0;
    if (!es.live[e]) {                                                     // finished before this tick: nothing is executed, nothing is counted
        takeover[e] = 0; reason[e] = 0; exec_jerk[e] = 0.0;
        if (exec_action) exec_action[e] = ((const double *)action)[e];
        takeover_ticks[e] = count[e];
        return;
    }
    const bool take = sh_takeover[e] != 0;
    double pjerk = es.pjerk[e];
    if (take) {
        const double cmd = sh_speed[e];
        const double v = s.ego4[e * 4 + 2];
        pjerk = (clip((cmd - v) / c.tick, c.a_min, c.a_max) - es.prev_a[e]) / c.tick;
        es.cmd[e] = cmd; es.pjerk[e] = pjerk;
        es.inv[e] = es.inv[e] + takeover_penalty * c.tick;
        ++cnt;
    }
    count[e] = cnt; tag[e] = ep;
    takeover[e] = take ? 1 : 0;
    reason[e] = sh_reason[e];
    exec_jerk[e] = pjerk;
    if (exec_action) exec_action[e] = take ? clip(pjerk, c.j_min, c.j_max) : ((const double *)action)[e];
    takeover_ticks[e] = cnt;
}

#ifdef STMPC_UNIT_ENV        // (the kernels of the unit that launches them)
__global__ void __launch_bounds__(64) k_shield_env_pre(ECfg c, sim::Cfg sc, int N, int kmax, sim::State s, EState es, const void *__restrict__ action,
                                                       ShieldView w) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    shield_env_pre_body(c, sc, e, kmax, s, es, action, w);
}

__global__ void __launch_bounds__(64) k_shield_env_apply(ECfg c, double takeover_penalty, int N, sim::State s, EState es, const void *__restrict__ action,
                                                         const double *__restrict__ sh_speed, const int *__restrict__ sh_takeover,
                                                         const int *__restrict__ sh_reason, int *count, int *tag, unsigned char *__restrict__ takeover,
                                                         int *__restrict__ reason, double *__restrict__ exec_jerk, double *__restrict__ exec_action,
                                                         int *__restrict__ takeover_ticks) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    shield_env_apply_body(c, takeover_penalty, e, s, es, action, sh_speed, sh_takeover, sh_reason, count, tag, takeover, reason, exec_jerk, exec_action, takeover_ticks);
}
#endif

}  // namespace env
}  // namespace stmpc
