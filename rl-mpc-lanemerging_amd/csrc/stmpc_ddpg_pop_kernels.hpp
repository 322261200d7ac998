// stmpc_ddpg_pop_kernels.hpp -- a population axis on the DDPG learner: P independent learners (each its own replay ring, networks, Adam state,
// counters, tickets, seed and constants) advance with ONE launch per kernel of stmpc_ddpg_kernels.hpp.  The reference trains its agents one
// TRAIN_DDPG run (ddpg.py:44-80) per seed -- the train_{traffic_type}_{seed}.json configs and the ddpg_*{1,2,...} checkpoints its
// pretrained_models/README.md lists -- and at the shipped shape one learner's update keeps seven workgroups of the device busy; the members of a
// population fill the rest.
//
// Every entry here is the single-learner kernel's body (the __device__ functions of stmpc_ddpg_kernels.hpp, not a copy) on the member blockIdx.y
// selects from a device table of DdpgDev.  blockIdx.y is wave-uniform and the table is read before the workgroup's first store, so the struct comes
// in through scalar loads like the by-value argument it replaces.  gridDim.x is the per-member block count and each member has its own tickets, so
// dg_last_block counts one member's workgroups; no float atomics, no reduction across members: a member's bits do not depend on who else is in the
// population.  LDS per workgroup is the single learner's.
//   k_replay_push_pop / k_ddpg_act_pop   member m owns rows [m * n, (m + 1) * n) of the step tensors; a 16-row acting tile never spans two
//                                       members, and the noise is keyed by the row local to the slice, as for a lone learner acting on it
//   k_ddpg_adam_pop                     the learning rates arrive by value (DdpgLr), so the chain stays free of host-to-device copies and capturable
#pragma once
#include "stmpc_ddpg_kernels.hpp"

namespace stmpc {

constexpr int DG_POP_MAX = 64;
struct DdpgLr { float lr[DG_POP_MAX]; };

__global__ void __launch_bounds__(256) k_replay_push_pop(const DdpgDev *__restrict__ members, int n, const float *__restrict__ obs, const float *__restrict__ next_obs,
                                                         const float *__restrict__ final_obs, int obs_stride, const int *__restrict__ ticks,
                                                         const int *__restrict__ next_ticks, const double *__restrict__ action, const double *__restrict__ reward,
                                                         const unsigned char *__restrict__ term, const unsigned char *__restrict__ trunc) {
    const DdpgDev L = members[blockIdx.y];
    const size_t e0 = (size_t)blockIdx.y * n, o0 = e0 * obs_stride;
    ddpg_push_body(L, n, obs + o0, next_obs + o0, final_obs ? final_obs + o0 : nullptr, obs_stride, ticks + e0, next_ticks ? next_ticks + e0 : nullptr, action + e0,
                   reward + e0, term + e0, trunc + e0);
}

__global__ void __launch_bounds__(AT_THREADS) k_ddpg_critic_fwd_pop(const DdpgDev *__restrict__ members, int B, int gate) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dg_smem[];
    const DdpgDev L = members[blockIdx.y];
    ddpg_critic_fwd_body(L, B, gate, dg_smem);
}

__global__ void __launch_bounds__(AT_THREADS) k_ddpg_actor_fwd_pop(const DdpgDev *__restrict__ members, int B, int gate) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dg_smem[];
    const DdpgDev L = members[blockIdx.y];
    ddpg_actor_fwd_body(L, B, gate, dg_smem);
}

__global__ void __launch_bounds__(64 * DG_WG_WAVES) k_ddpg_wgrad_pop(const DdpgDev *__restrict__ members, int which, int Bp, int gate) {
    __shared__ double part_s[DG_WG_WAVES][256];
    const DdpgDev L = members[blockIdx.y];
    ddpg_wgrad_body(L, which, Bp, gate, part_s);
}

__global__ void __launch_bounds__(256) k_ddpg_adam_pop(const DdpgDev *__restrict__ members, int which, DdpgLr lrs, int mode, int bump, int gate) {
    const DdpgDev L = members[blockIdx.y];
    ddpg_adam_body(L, which, lrs.lr[blockIdx.y], mode, bump, gate);
}

// out [P][4]
__global__ void __launch_bounds__(64) k_ddpg_stats_pop(const DdpgDev *__restrict__ members, int B, double *out) {
    const DdpgDev L = members[blockIdx.y];
    ddpg_stats_body(L, B, out + 4 * (size_t)blockIdx.y);
}

// dbg (may be null) [P * n][4]
__global__ void __launch_bounds__(AT_THREADS) k_ddpg_act_pop(const DdpgDev *__restrict__ members, int n, const float *__restrict__ obs, int obs_stride,
                                                             const int *__restrict__ ticks, int noise, double *__restrict__ action, unsigned int *__restrict__ dbg) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dg_smem[];
    const DdpgDev L = members[blockIdx.y];
    const size_t e0 = (size_t)blockIdx.y * n;
    ddpg_act_body(L, n, obs + e0 * obs_stride, obs_stride, ticks + e0, noise, action + e0, dbg ? dbg + 4 * e0 : nullptr, dg_smem);
}

}  // namespace stmpc
