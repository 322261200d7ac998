// stmpc_per_pop_kernels.hpp -- prioritised replay for the populations: the sampling step and the priority update of stmpc_per_kernels.hpp over the
// members of a DDPG population (a device table of DdpgDev, the member in blockIdx.y as in stmpc_ddpg_pop_kernels.hpp) and of a TD3 population (a table
// of Td3Dev, the member in blockIdx.z as in stmpc_td3_pop_kernels.hpp).  "Prioritised against uniform replay" and "which alpha / beta" are sweeps of
// the kind a population runs side by side; the reference's hand-written trainer ships with USE_PRIORITIZED_ER = True (config.py).
//
// Every entry is the lone kernel's body (per_sample_body / per_update_body, not a copy) in ONE workgroup of PER_THREADS threads per member, with the
// lone kernel's static LDS.  Each is a latency chain -- about log2(L) dependent fp64 loads, or as many load-add-store-barrier levels -- that keeps one
// compute unit busy, so P chains in one launch run next to one another.  The tree part of a push needs no kernel here: ddpg_push_body calls
// per_push_tree in the member's last workgroup when the member has a tree, under k_replay_push_pop as under k_replay_push.
//   * a member without a tree (DdpgDev::tree null: it samples uniformly) returns at once, so a population may mix prioritised and uniform members;
//   * the gate (ddpg_gate) reads the member's own counters: a gated member's tree changes through pushes only;
//   * both returns happen before the body's first barrier and for the whole workgroup: the member index is the workgroup's, the table is never written
//     by a kernel and the counters not by these kernels, so the predicate is workgroup-uniform;
//   * no atomics, no reduction across members: an internal node is still recomputed as left + right, and a member's bits do not depend on who else is
//     in the population.
// TD3: the body runs on the member's view 0 (the base's struct: tree, idx, weights, critic 1's Q - y); critic 2's Q - y is view 1's atd, so per_td's
// rule -- the larger magnitude of both critics, on every update -- needs no table of its own.
#pragma once
#include "stmpc_per_kernels.hpp"
#include "stmpc_ddpg_pop_kernels.hpp"
#include "stmpc_td3_pop_kernels.hpp"

namespace stmpc {

__global__ void __launch_bounds__(PER_THREADS) k_per_sample_pop(const DdpgDev *__restrict__ members, int B, int Bp, int gate) {
    __shared__ double red[PER_THREADS];
    const DdpgDev L = members[blockIdx.y];
    if (!L.tree) return;
    per_sample_body(L, B, Bp, gate, red);
}

__global__ void __launch_bounds__(PER_THREADS) k_per_update_pop(const DdpgDev *__restrict__ members, int B, int gate) {
    __shared__ int idx_s[PER_MAX_B];
    const DdpgDev L = members[blockIdx.y];
    if (!L.tree) return;
    per_update_body(L, nullptr, B, gate, idx_s);
}

__global__ void __launch_bounds__(PER_THREADS) k_per_sample_td3_pop(const Td3Dev *__restrict__ members, int B, int Bp, int gate) {
    __shared__ double red[PER_THREADS];
    const DdpgDev &L = members[blockIdx.z].v[0];
    if (!L.tree) return;
    per_sample_body(L, B, Bp, gate, red);
}

__global__ void __launch_bounds__(PER_THREADS) k_per_update_td3_pop(const Td3Dev *__restrict__ members, int B, int gate) {
    __shared__ int idx_s[PER_MAX_B];
    const Td3Dev &T3 = members[blockIdx.z];
    if (!T3.v[0].tree) return;
    per_update_body(T3.v[0], T3.v[1].atd, B, gate, idx_s);
}

}  // namespace stmpc
