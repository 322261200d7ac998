// stmpc_qactor_pop_kernels.hpp -- a population axis on the Q-network policy: P Q-networks, each on its own slice of one batch of states, in ONE
// launch.  The reference compares its DQN agents run by run (DQNAgent.get_control, dqn.py:375-380, behind one evaluation process per model: double
// against plain targets, clipped against unclipped, the freeze period, prioritised against uniform replay, seeds, traffic types); here the members
// -- created actors, or zero-copy views of learners' online or target networks, a DQN population's members among them -- face the environments of
// one world side by side.
//
// The entry is k_qactor_eval's body (qactor_eval_body of stmpc_qactor_kernels.hpp, not a copy) with the member blockIdx.y selects from a device table
// of QActorMember.  blockIdx.y is wave-uniform and no kernel writes the table, so the struct comes in through scalar loads like the by-value
// arguments it replaces.  Workgroup (x, m) serves local rows [16 x, 16 x + 16) of member m = global rows m * n_per_member + local: a 16-row tile
// never spans two members, and a member's tail rows are masked as a lone actor on n_per_member rows masks them.  Every global index -- ego4 (the
// acceleration mode's read of ego4[e * 4 + 3] too), k_count, ox / ov / oa, live, feat, action, q, jerk -- is the body's `row0 + local`.  The
// summation orders are the lone actor's, so a member's bits do not depend on who else is in the population.  LDS per workgroup is the lone actor's
// ddpg_tile_bytes(h1p, Ap).  No atomics, and no workgroup writes a row of another member.
#pragma once
#include "stmpc_qactor_kernels.hpp"

namespace stmpc {

struct QActorMember {               // what differs per member: what dqn_q reads of a DqnDev, and the actor's own constants
    DdpgNet q;                      // the learner's base.q (a view) or the actor's own network: fixed from the owner's create to its destroy
    int n_obs, h1p, A, Ap;
    int target;                     // 0: online network, 1: target network (a view)
    int accel;                      // 0: jerk mode, 1: acceleration mode
    const double *table;            // [A] the member's action table
    double tick, jerk_min, jerk_max;
};

// the state arrays, live, feat, action, q and jerk have P * n_per_member rows
__global__ void __launch_bounds__(AT_THREADS) k_qactor_eval_pop(FeatCfg f, const QActorMember *__restrict__ members, int n_per_member, int Kmax,
                                                                const double *__restrict__ ego4, const int *__restrict__ k_count, const double *__restrict__ ox,
                                                                const double *__restrict__ ov, const double *__restrict__ oa, const int *__restrict__ live,
                                                                float *feat, int feat_stride, int *action, float *q, double *jerk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char qa_smem[];
    const QActorMember M = members[blockIdx.y];
    DqnDev D{};
    D.base.q = M.q; D.base.n_obs = M.n_obs; D.base.h1p = M.h1p; D.A = M.A; D.Ap = M.Ap;
    const QActorOut o{M.table, M.tick, M.jerk_min, M.jerk_max, M.accel, feat_stride, feat, action, q, jerk};
    qactor_eval_body(f, D, M.target, (int)blockIdx.y * n_per_member, n_per_member, Kmax, ego4, k_count, ox, ov, oa, live, o, qa_smem);
}

}  // namespace stmpc
