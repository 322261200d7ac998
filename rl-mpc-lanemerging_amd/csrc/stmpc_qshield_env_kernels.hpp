// stmpc_qshield_env_kernels.hpp -- the DISCRETE vector environments (JerkEnv, AccelerationEnv) stepped behind the combined controller
// (dqn.RLAgent.do_combined_control, dqn.py:117-200, which DQNAgent inherits) with a Q-network (DQNAgent.get_control, dqn.py:375-380) proposing the
// later rollout steps: the env's action INDEX is the controller's first action.  One step is
//   k_qshield_env_pre    the env's action handling (k_env_act's, through the same device function) + the planner's view of the current state with the
//                        other vehicles' accelerations (sim::k_sim_view's body, called), into the start rows and the rollout's current rows + the
//                        first action: the jerk the index stands for, by the Q-actor's own rule (stmpc_qactor_kernels.hpp);
//   for step = 1 ... max(L, 1): from step 2 on the body of stmpc_qactor_eval_device (or of stmpc_pop_qactor_eval_device) on the current rows, then the
//                        body of stmpc_rollout_step_device;
//   the body of stmpc_combined_decide_device, k_shield_env_apply with exec_action == NULL (a discrete index is not rewritten), sim::k_sim_step and
//   env::k_env_post, all unchanged.
// The Q-network has no time feature, so this env keeps NO time counter: there is no evals, no evals_tag, no rollout_time and no *_evals_device entry
// (CShieldView's two counter rows stay unread and unwritten here).
// One thread per environment, 64-thread workgroups, a flat grid over the N rows: k_cshield_env_pre's launch shape.  Every per-environment value is a
// per-lane value read and written with plain vector loads and stores after the thread's bounds check; no LDS, no atomic (the error word is latched
// with a plain store of 1, as k_env_act latches it).  The kernel is a view walk and a few stores per lane next to L - 1 Q-network launches and two
// batched solves: its cost is its launch.
#pragma once
#include "stmpc_cshield_env_kernels.hpp"

namespace stmpc {
namespace env {

// The jerk the controller's rollout step 1 applies for table entry `value` on a state whose ego acceleration is a_ego -- what k_qactor_eval returns as
// `jerk` for that index on that state, bit for bit (qactor_eval_body's last lines with the env's table, tick and jerk limits): the entry itself in jerk
// mode; in acceleration mode clip((value - a_ego) / tick, j_min, j_max) in fp64, the comparisons in the Q-actor's order.
__device__ __forceinline__ double qshield_first_action(const ECfg &c, double value, double a_ego) {
    if (c.mode == ACT_JERK) return value;
    double v = (value - a_ego) / c.tick;
    v = v < c.j_min ? c.j_min : (v > c.j_max ? c.j_max : v);
    return v;
}

#ifdef STMPC_UNIT_ENV        // (the kernels of the unit that launches them)
// k_env_act's dispatch (handle_action, called) + the controller's view and first action.  A finished environment gets the view k_sim_view gives it and
// its first action from that state, while its step state is left alone, as k_env_act leaves it.  An index out of range follows the first-step shield's
// rule (shield_env_pre_body): a running environment latches the error word; running or not, the command is the current speed and the first action 0.0
// -- no table entry is read, and no NaN reaches the rollout, the predictor or the solver.
__global__ void __launch_bounds__(64) k_qshield_env_pre(ECfg c, sim::Cfg sc, int N, int kmax, sim::State s, EState es, const void *__restrict__ action,
                                                        CShieldView w) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    sim::sim_view_env(sc, kmax, s, e, w.ego5, w.k, w.ox, w.ov, w.cur_oa);
    for (int q = 0; q < 4; ++q) w.cur_ego4[(size_t)e * 4 + q] = w.ego5[(size_t)e * 5 + q];
    for (int i = 0; i < kmax; ++i) { w.cur_ox[(size_t)e * kmax + i] = w.ox[(size_t)e * kmax + i]; w.cur_ov[(size_t)e * kmax + i] = w.ov[(size_t)e * kmax + i]; }
    const int live = s.status[e] == 0;
    es.live[e] = live;
    const double v = s.ego4[e * 4 + 2], a = s.ego4[e * 4 + 3], prev_a = es.prev_a[e];
    double pjerk, inv, cmd, first = 0.0;
    if (handle_action(c, action, e, v, a, prev_a, cmd, pjerk, inv)) {
        if (live) es.err[0] = 1u;
        cmd = v;
    } else {
        first = qshield_first_action(c, c.actions[((const int *)action)[e]], w.cur_ego4[(size_t)e * 4 + 3]);
    }
    w.first_action[e] = first;
    if (!live) return;                                                     // (k_sim_step idles finished environments)
    es.cmd[e] = cmd; es.pjerk[e] = pjerk; es.inv[e] = inv;
}
#endif

}  // namespace env
}  // namespace stmpc
