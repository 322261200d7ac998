// stmpc_c51actor_pop_kernels.hpp -- a population axis on the categorical (C51) policy: P logits networks, each with its own support and on its own
// slice of one batch of states, in ONE launch.  What stmpc_qactor_pop_kernels.hpp is for the Q-network policy, for the distributional head of the
// reference's third agent (rainbow.py) doing DQNAgent.get_control's job (dqn.py:375-380): the sweeps a C51 population trains -- support, double,
// target period, gamma, n-step, seed, prioritised replay, sigma0 -- face the environments of one world side by side instead of one evaluation
// process per model.
//
// The entry is k_c51actor_eval's body (c51actor_eval_body of stmpc_c51actor_kernels.hpp, not a copy) with the member blockIdx.y selects from a device
// table of C51ActorMember.  blockIdx.y is wave-uniform and no kernel writes the table, so the struct comes in through scalar loads like the by-value
// arguments it replaces, and the C51Dev the body reads is rebuilt from it in registers.  Workgroup (x, m) serves local rows [16 x, 16 x + 16) of
// member m = global rows m * n_per_member + local: a 16-row tile never spans two members, and a member's tail rows are masked as a lone actor on
// n_per_member rows masks them.  Every global index -- ego4 (the acceleration mode's read of ego4[e * 4 + 3] too), k_count, ox / ov / oa, live, feat,
// action, q, jerk -- is the body's `row0 + local`.  The summation orders, the fp64 softmax statistics and the support (v_min, dz: fp64, copied from
// the member, never recomputed here) are the lone actor's, so a member's bits do not depend on who else is in the population.  The dueling branch is
// uniform across a workgroup (one head per population).  LDS per workgroup is the lone actor's ddpg_tile_bytes(h1p, Ap).  No atomics, and no
// workgroup writes a row of another member.
#pragma once
#include "stmpc_c51actor_kernels.hpp"

namespace stmpc {

struct C51ActorMember {             // what differs per member: what the body reads of a C51Dev, and the actor's own constants
    DdpgNet q;                      // the learner's dev.dq.base.q (a view) or the actor's own network: fixed from the owner's create to its destroy
    int n_obs, h1p, A, Ap;
    int K, dueling;                 // atoms; 1: the dueling head (Ap = pad16((A + 1) K))
    double v_min, v_max, dz;        // the support as the owner holds it
    int target;                     // 0: online network, 1: target network (a view)
    int accel;                      // 0: jerk mode, 1: acceleration mode
    const double *table;            // [A] the member's action table
    double tick, jerk_min, jerk_max;
};

// the state arrays, live, feat, action, q and jerk have P * n_per_member rows; q: float32 [rows][A], the expected values
__global__ void __launch_bounds__(AT_THREADS) k_c51actor_eval_pop(FeatCfg f, const C51ActorMember *__restrict__ members, int n_per_member, int Kmax,
                                                                  const double *__restrict__ ego4, const int *__restrict__ k_count, const double *__restrict__ ox,
                                                                  const double *__restrict__ ov, const double *__restrict__ oa, const int *__restrict__ live,
                                                                  float *feat, int feat_stride, int *action, float *q, double *jerk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char qa_smem[];
    const C51ActorMember M = members[blockIdx.y];
    C51Dev D{};
    D.dq.base.q = M.q; D.dq.base.n_obs = M.n_obs; D.dq.base.h1p = M.h1p; D.dq.A = M.A; D.dq.Ap = M.Ap;
    D.K = M.K; D.dueling = M.dueling; D.v_min = M.v_min; D.v_max = M.v_max; D.dz = M.dz;
    const QActorOut o{M.table, M.tick, M.jerk_min, M.jerk_max, M.accel, feat_stride, feat, action, q, jerk};
    c51actor_eval_body(f, D, M.target, (int)blockIdx.y * n_per_member, n_per_member, Kmax, ego4, k_count, ox, ov, oa, live, o, qa_smem);
}

}  // namespace stmpc
