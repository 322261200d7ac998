// stmpc_actor_pop_kernels.hpp -- a population axis on the policy evaluation: P actors, each on its own slice of one batch of states, in ONE launch.
// The reference evaluates its trained agents one EVALUATE_COMBINED_DDPG run per model (DDPGAgent.load + get_control, ddpg.py:38-44, 83-87, for the
// MODEL_NAME of each configs/combined_<traffic>_{1,2,3}.json), and train_ddpg_all_with_lr_drop (ddpg.py:96-117) closes with an evaluation of what it trained; here
// the members of a population -- shipped actors, files, or zero-copy views of learners' weights -- face the environments of one world side by side.
//
// The entry is k_actor_eval's body (actor_eval_body of stmpc_actor_kernels.hpp, not a copy) with the member blockIdx.y selects from a device table of
// ActorDev.  blockIdx.y is wave-uniform and the table is read before the workgroup's first store, so the struct comes in through scalar loads like
// the by-value argument it replaces.  Workgroup (x, m) serves local rows [16 x, 16 x + 16) of member m = global rows m * n_per_member + local: a
// 16-row tile never spans two members, and a member's tail rows are masked as a lone actor on n_per_member rows masks them.  The summation orders are
// the lone actor's, so a member's bits do not depend on who else is in the population.  LDS per workgroup is the single actor's.
#pragma once
#include "stmpc_actor_kernels.hpp"

namespace stmpc {

// the state arrays, evals, live, feat_out and jerk_out have P * n_per_member rows
__global__ void __launch_bounds__(AT_THREADS) k_actor_eval_pop(FeatCfg f, const ActorDev *__restrict__ members, int n_per_member, int Kmax,
                                                               const double *__restrict__ ego4, const int *__restrict__ k_count, const double *__restrict__ ox,
                                                               const double *__restrict__ ov, const double *__restrict__ oa, const int *__restrict__ live,
                                                               int *evals, float *feat_out, int feat_stride, double *jerk_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char at_smem[];
    const ActorDev A = members[blockIdx.y];
    actor_eval_body(f, A, (int)blockIdx.y * n_per_member, n_per_member, Kmax, ego4, k_count, ox, ov, oa, live, evals, feat_out, feat_stride, jerk_out, at_smem);
}

}  // namespace stmpc
