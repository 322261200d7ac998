// stmpc_td3_pop_kernels.hpp -- a population axis on the TD3 learner: P independent TD3 learners (each its own ring, actor, two critics, Adam state,
// counters, tickets, seed, constants, smoothing noise and policy_delay) advance with ONE launch per kernel of stmpc_td3_kernels.hpp, as
// stmpc_ddpg_pop_kernels.hpp does for the DDPG learner.  The reference compares per-seed, per-traffic TRAIN_DDPG runs (the train_{traffic}_{seed}.json
// configs, train_ddpg_all_with_lr_drop); TD3 adds target_noise, noise_clip and policy_delay to what such a sweep varies.
//
// Every entry is the lone learner's body (the __device__ functions of stmpc_td3_kernels.hpp, not a copy) on the member blockIdx.z selects from a
// device table of Td3Dev.  blockIdx.y keeps its meaning -- the view in the critic kernels, actor / critic 1 / critic 2 in k_td3_adam_finish -- and
// gridDim.x, gridDim.y are the lone learner's, so dg_last_block counts one member's workgroups on that member's own tickets; gridDim.z enters no
// count.  The gate (ddpg_gate) and the delay predicate (td3_due) read the member's own counters and its own delay: a gated member, or one whose
// delayed half is not due, returns from its workgroups while the others work, and the host never learns which.  The member is taken as a
// reference into the table (two DdpgDev: a by-value copy would be the whole struct); blockIdx.z is wave-uniform and the table is never written by
// a kernel, so the fields a body uses arrive through scalar loads.  No float atomics, no reduction across members.
// Acting and pushing need no kernel here: k_ddpg_act_pop / k_replay_push_pop serve on a table of the members' base structs (v[0]).
#pragma once
#include "stmpc_td3_kernels.hpp"
#include "stmpc_ddpg_pop_kernels.hpp"

namespace stmpc {

__global__ void __launch_bounds__(AT_THREADS) k_td3_critic_fwd_pop(const Td3Dev *__restrict__ members, int B, int gate) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dg_smem[];
    td3_critic_fwd_body(members[blockIdx.z], B, gate, nullptr, dg_smem);
}

__global__ void __launch_bounds__(64 * DG_WG_WAVES) k_td3_wgrad_pop(const Td3Dev *__restrict__ members, int which, int Bp, int gate) {
    __shared__ double part_s[DG_WG_WAVES][256];
    td3_wgrad_body(members[blockIdx.z], which, Bp, gate, part_s);
}

__global__ void __launch_bounds__(AT_THREADS) k_td3_actor_fwd_pop(const Td3Dev *__restrict__ members, int B, int gate) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dg_smem[];
    td3_actor_fwd_body(members[blockIdx.z], B, gate, dg_smem);
}

__global__ void __launch_bounds__(256) k_td3_adam_critics_pop(const Td3Dev *__restrict__ members, DdpgLr lrs, int gate) {
    td3_adam_critics_body(members[blockIdx.z], lrs.lr[blockIdx.z], gate);
}

__global__ void __launch_bounds__(256) k_td3_adam_finish_pop(const Td3Dev *__restrict__ members, DdpgLr lrs, int gate) {
    td3_adam_finish_body(members[blockIdx.z], lrs.lr[blockIdx.z], gate);
}

// out [P][6]
__global__ void __launch_bounds__(64) k_td3_stats_pop(const Td3Dev *__restrict__ members, int B, double *out) {
    td3_stats_body(members[blockIdx.z], B, out + 6 * (size_t)blockIdx.z);
}

}  // namespace stmpc
