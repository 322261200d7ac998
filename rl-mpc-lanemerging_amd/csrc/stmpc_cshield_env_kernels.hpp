// stmpc_cshield_env_kernels.hpp -- the vector environment stepped behind the combined controller (dqn.RLAgent.do_combined_control, dqn.py:117-200):
// the env's action is the controller's FIRST action, an actor on the device proposes the later rollout steps, the decision rules choose what is
// executed, and the learner is told.  One step is
//   k_cshield_env_pre    the env's action handling (k_env_act's, through the same device function) + the planner's view of the current state with the
//                        other vehicles' accelerations (sim::k_sim_view's body, called), into the start rows and the rollout's current rows + the
//                        first action + the rollout's time counter;
//   for step = 1 ... max(L, 1): from step 2 on the body of stmpc_actor_eval_device on the current rows, then the body of stmpc_rollout_step_device;
//   the body of stmpc_combined_decide_device (shared with the entries, not copied);
//   k_shield_env_apply   (stmpc_shield_env_kernels.hpp, unchanged: the rule of the first-step shield serves the combined controller's decision as it is);
//   sim::k_sim_step and env::k_env_post, unchanged.
// One thread per environment, 64-thread workgroups, a flat grid over the N rows: the lone env's launch shape.  Every per-environment value is a
// per-lane value read and written with plain vector loads and stores after the thread's bounds check; no LDS, no atomic.  The kernels are a view walk
// and a few stores per lane next to L actor launches and two batched solves: their cost is their launch.
#pragma once
#include "stmpc_shield_env_kernels.hpp"

namespace stmpc {
namespace env {

enum { ROLLOUT_TIME_ENV = 0, ROLLOUT_TIME_DEPLOYED = 1 };      // stmpc_cshield_env_cfg.rollout_time

struct CShieldView {                        // device arrays: what the rollout and the decision read (the layouts of stmpc_rollout_step_device)
    double *ego5;                           // [N][5] the start state
    int *k;                                 // [N]
    double *ox, *ov;                        // [N][kmax] the start state's vehicles
    double *cur_ego4;                       // [N][4] the rollout's current state: a second copy of the view
    double *cur_ox, *cur_ov, *cur_oa;       // [N][kmax]
    double *first_action;                   // [N] the action's jerk
    int *evals;                             // [N] the rollout actor's time counter
    int *evals_tag;                         // [N] "deployed" time: the episode `evals` was counted in
};

// The count environment e's next proposal is evaluated at: the episode's ticks ("env" time), or the evaluations of its current episode so far
// ("deployed" time; the count restarts when es.episode[e] has moved on, as the takeover count of k_shield_env_apply does).
__device__ __forceinline__ int cshield_evals_now(int rollout_time, const sim::State &s, const EState &es, const CShieldView &w, int e) {
    if (rollout_time == ROLLOUT_TIME_ENV) return s.ticks[e];
    return w.evals_tag[e] == es.episode[e] ? w.evals[e] : 0;
}

#ifdef STMPC_UNIT_ENV        // (the kernels of the unit that launches them)
// k_env_act's dispatch (handle_action, called) + the controller's view, first action and time counter.  A finished environment gets the view
// k_sim_view gives it and proposes its action from that state -- what episodes.EpisodeRunner(controller="combined") decides for a finished
// environment -- while its step state is left alone, as k_env_act leaves it.  (Continuous jerks only: handle_action cannot refuse one.)
__global__ void __launch_bounds__(64) k_cshield_env_pre(ECfg c, sim::Cfg sc, int N, int kmax, int rollout_time, sim::State s, EState es,
                                                        const void *__restrict__ action, CShieldView w) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    sim::sim_view_env(sc, kmax, s, e, w.ego5, w.k, w.ox, w.ov, w.cur_oa);
    for (int q = 0; q < 4; ++q) w.cur_ego4[(size_t)e * 4 + q] = w.ego5[(size_t)e * 5 + q];
    for (int i = 0; i < kmax; ++i) { w.cur_ox[(size_t)e * kmax + i] = w.ox[(size_t)e * kmax + i]; w.cur_ov[(size_t)e * kmax + i] = w.ov[(size_t)e * kmax + i]; }
    w.first_action[e] = ((const double *)action)[e];
    const int n = cshield_evals_now(rollout_time, s, es, w, e);
    w.evals[e] = n + 1;                                                    // (this tick's proposal was one evaluation)
    w.evals_tag[e] = es.episode[e];
    const int live = s.status[e] == 0;
    es.live[e] = live;
    if (!live) return;                                                     // (k_sim_step idles finished environments)
    const double v = s.ego4[e * 4 + 2], a = s.ego4[e * 4 + 3], prev_a = es.prev_a[e];
    double pjerk, inv, cmd;
    handle_action(c, action, e, v, a, prev_a, cmd, pjerk, inv);
    es.cmd[e] = cmd; es.pjerk[e] = pjerk; es.inv[e] = inv;
}

// stmpc_cshield_env_evals_device
__global__ void __launch_bounds__(64) k_cshield_env_evals(int N, int rollout_time, sim::State s, EState es, CShieldView w, int *__restrict__ out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    out[e] = cshield_evals_now(rollout_time, s, es, w, e);
}
#endif

}  // namespace env
}  // namespace stmpc
