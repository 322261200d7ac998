// stmpc_c51_pop_kernels.hpp -- a population axis on the categorical (C51) learner: P independent C51 learners (each its own replay ring, logits
// network, target, Adam state, counters, tickets, seed, constants, support [v_min, v_max], double flag, target_period and n_step) advance with ONE
// launch per kernel of stmpc_c51_kernels.hpp, as stmpc_dqn_pop_kernels.hpp does for the DQN learner.  What a user asks of the categorical agent --
// which support fits this env's returns, double against plain action selection, which target_period, gamma, n_step and seed, prioritised against
// uniform replay -- is a sweep of lone runs; a population is those runs side by side, for the launch count of one.
//
// Every entry here is the lone kernel's body (the __device__ functions of stmpc_c51_kernels.hpp and stmpc_dqn_kernels.hpp, not a copy) on the member
// blockIdx.y selects from a device table of C51Dev.  blockIdx.y is wave-uniform and the table is read before the workgroup's first store and never
// written by a kernel, so the struct comes in through scalar loads like the by-value argument it replaces.  gridDim.x is the per-member block
// count and each member has its own tickets, so dg_last_block counts one member's workgroups; no atomics and no reduction across members: a
// member's bits do not depend on who else is in the population.  LDS per workgroup is the lone learner's c51_tile_bytes(h1p, Ap, K): the members
// share n_obs, h1, n_actions, n_atoms, batch and capacity, so one LDS size and one grid serve them all.
//   k_c51_push_pop / k_c51_act_pop   member m owns rows [m * n, (m + 1) * n) of the step tensors; a 16-row acting tile never spans two members, and
//                                    the exploration hash is keyed by the row local to the slice, the member's seed and the member's own DG_ACTS.
//                                    eps arrives by value, one float per member (DqnEps); a member whose eps is 0 draws nothing, takes no ticket
//                                    and leaves its acting counter alone, as the lone learner called with eps = 0
//   k_c51_fwd_pop                    c51_fwd_body: the support (v_min, v_max, dz) is the member's own struct's, and the n-step dispatch inside the
//                                    body is per member (wave-uniform: one member per workgroup)
//   k_c51_adam_pop                   the learning rates arrive by value (DdpgLr); the hard copy of the target and the replay_start gate are decided
//                                    from the member's own counters and target_period
// Prioritised replay and the statistics need no kernel here: k_per_sample_pop, k_per_update_pop and k_ddpg_stats_pop serve on a second table of the
// members' base structs (DdpgDev [P]), and the tree part of a push is dqn_push_body's own (per_push_tree in the member's last workgroup).
#pragma once
#include "stmpc_c51_kernels.hpp"
#include "stmpc_dqn_pop_kernels.hpp"

namespace stmpc {

__global__ void __launch_bounds__(256) k_c51_push_pop(const C51Dev *__restrict__ members, int n, const float *__restrict__ obs, const float *__restrict__ next_obs,
                                                      const float *__restrict__ final_obs, int obs_stride, const int *__restrict__ action,
                                                      const double *__restrict__ reward, const unsigned char *__restrict__ term, const unsigned char *__restrict__ trunc) {
    const DqnDev D = members[blockIdx.y].dq;
    const size_t e0 = (size_t)blockIdx.y * n, o0 = e0 * obs_stride;
    dqn_push_body(D, n, obs + o0, next_obs + o0, final_obs ? final_obs + o0 : nullptr, obs_stride, action + e0, reward + e0, term + e0, trunc + e0);
}

// dbg_q (may be null) [P * n][A]: the expected values
__global__ void __launch_bounds__(AT_THREADS) k_c51_act_pop(const C51Dev *__restrict__ members, int n, const float *__restrict__ obs, int obs_stride, DqnEps eps,
                                                            int *__restrict__ action, float *__restrict__ dbg_q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dg_smem[];
    const C51Dev D = members[blockIdx.y];
    const size_t e0 = (size_t)blockIdx.y * n;
    c51_act_body(D, n, obs + e0 * obs_stride, obs_stride, eps.eps[blockIdx.y], (int)((eps.explore >> blockIdx.y) & 1ull), action + e0,
                 dbg_q ? dbg_q + e0 * D.dq.A : nullptr, dg_smem);
}

__global__ void __launch_bounds__(AT_THREADS) k_c51_fwd_pop(const C51Dev *__restrict__ members, int B, int gate) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dg_smem[];
    const C51Dev D = members[blockIdx.y];
    c51_fwd_body<false>(D, B, gate, nullptr, nullptr, dg_smem);
}
// (a population of dueling members: they share the head)
__global__ void __launch_bounds__(AT_THREADS) k_c51_fwd_duel_pop(const C51Dev *__restrict__ members, int B, int gate) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dg_smem[];
    const C51Dev D = members[blockIdx.y];
    c51_fwd_body<true>(D, B, gate, nullptr, nullptr, dg_smem);
}

__global__ void __launch_bounds__(64 * DG_WG_WAVES) k_c51_wgrad_pop(const C51Dev *__restrict__ members, int Bp, int gate) {
    __shared__ double part_s[DG_WG_WAVES][256];
    const DdpgDev L = members[blockIdx.y].dq.base;
    ddpg_wgrad_body(L, 1, Bp, gate, part_s);
}

__global__ void __launch_bounds__(256) k_c51_adam_pop(const C51Dev *__restrict__ members, DdpgLr lrs, int gate) {
    const DqnDev D = members[blockIdx.y].dq;
    dqn_adam_body(D, lrs.lr[blockIdx.y], 0, gate);
}

}  // namespace stmpc
