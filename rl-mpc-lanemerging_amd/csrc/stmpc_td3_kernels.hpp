// stmpc_td3_kernels.hpp -- TD3 (Fujimoto et al. 2018) on the DDPG learner's pieces: a second critic, clipped noise on the target action, the minimum
// of the two target critics, and the actor and all targets stepped only every policy_delay-th update.
//
// A TD3 learner is TWO VIEWS of one learner (Td3Dev::v): v[0] is the base DDPG learner's struct (actor, critic 1, workspace, ring, counters, tickets),
// v[1] the same struct with q = critic 2, critic 2's workspace and tickets of its own.  Every kernel below is a body of stmpc_ddpg_kernels.hpp on the
// view blockIdx.y selects, so the second critic rides in the grid's y dimension of launches that fill a fraction of the device.  One update is six
// launches whose shapes never change; whether it is gated (replay_start) or its delayed half is due is decided on the device from the counters:
//   k_td3_critic_fwd    (tiles, 2)   gather, pi_target(s'), smoothing noise, BOTH target critics (so the minimum needs no other workgroup), then the
//                                    view's own online critic forward and backward into its own workspace: nine ddpg_layer passes
//   k_td3_wgrad         (jobs, 2)    both critics' weight gradients
//   k_td3_adam_critics  (blocks, 2)  Adam step of both critics, no Polyak
//   k_td3_actor_fwd     (tiles)      } the actor against critic 1 as just stepped: only if (updates + 1) % policy_delay == 0
//   k_td3_wgrad         (jobs, 1)    }
//   k_td3_adam_finish   (blocks, 3)  if due: the actor's Adam step and the Polyak update of the actor's and both critics' targets; always: updates += 1
// Each kernel's text is a __device__ body taking the learner's struct by reference; the __global__ entry passes its by-value argument, and the
// population's entries (stmpc_td3_pop_kernels.hpp) a row of a device table.  The bodies read blockIdx.x / .y and gridDim.x / .y only.
// No float atomics, no sums across workgroups: a run is bit-reproducible.  With target noise 0, policy_delay 1 and critic 2 equal to critic 1 every
// bit equals the DDPG update's (the critic's Polyak reads nothing the actor step writes, so doing it after that step changes nothing).
#pragma once
#include "stmpc_ddpg_kernels.hpp"

namespace stmpc {

constexpr unsigned long long TD3_STREAM = 0x7464336E6F697365ull;    // the smoothing draws' seed is seed ^ this ("td3noise")

struct Td3Dev {
    DdpgDev v[2];                   // the two views (above)
    unsigned int *tick;             // [1]: k_td3_adam_finish's ticket
    float sigma, clip;              // smoothing noise: standard deviation and clip, absolute
    int delay;                      // policy_delay >= 1
};

// is the delayed half of the current update due?  (gate = 0, the gradient-only debug entry: always)
__device__ __forceinline__ bool td3_due(const Td3Dev &T3, int gate) {
    return !gate || (T3.v[0].cnt[DG_UPDATES] + 1) % T3.delay == 0;
}

// eps of minibatch row r of update upd: clip(sigma * gauss, -c, +c), gauss formed as k_ddpg_act's on the stream TD3_STREAM
__device__ __forceinline__ float td3_smoothing(const Td3Dev &T3, unsigned long long seed, long long upd, int r) {
    unsigned int u1, u2;
    const float e = T3.sigma * dg_gauss(dg_hash(seed ^ TD3_STREAM, (unsigned long long)upd, (unsigned long long)r), u1, u2);
    return e < -T3.clip ? -T3.clip : (e > T3.clip ? T3.clip : e);
}

// dbg (may be null) float32 [B][5]: eps, a', Qt1, Qt2, y of the minibatch; with it the pass ends there and writes nothing else
template <bool NS>
__device__ __forceinline__ void td3_critic_fwd_pass(const Td3Dev &T3, int B, int gate, float *__restrict__ dbg, unsigned char *dg_smem) {
    const DdpgDev &L = T3.v[blockIdx.y];
    if (!ddpg_gate(L, gate)) return;
    const DdpgTile T = ddpg_tile(dg_smem, L.h1p, L.h2p);
    const int tid = threadIdx.x, r0 = blockIdx.x * AT_TM, ns = L.n_obs + 1;
    const int row = tid >> 5, part = tid & 31;
    const long long upd = L.cnt[DG_UPDATES];
    ddpg_gather_tile<NS>(L, T, r0, B, L.cnt[DG_FILL], upd);
    __syncthreads();
    // a' = clip(pi_target(s') + eps, Box)
    const float z = ddpg_target_out(L, L.pi, T);
    if (part == 0) {
        const float eps = td3_smoothing(T3, L.seed, upd, r0 + row);
        const float a = (ddpg_tanh(z) * L.scale + L.mean) + eps;
        T.Xn[row * AT_KIN + ns] = a < L.a_low ? L.a_low : (a > L.a_high ? L.a_high : a);
        T.sc[row * 4 + 3] = eps;
    }
    __syncthreads();
    // min of both target critics on (s', a')
    const float q1 = ddpg_target_out(L, T3.v[0].q, T);
    __syncthreads();
    const float q2 = ddpg_target_out(L, T3.v[1].q, T);
    const float y = T.sc[row * 4 + 0] + (ddpg_discount<NS>(L, T) * T.sc[row * 4 + 1]) * (q2 < q1 ? q2 : q1);
    if (dbg) {
        if (blockIdx.y == 0 && part == 0 && r0 + row < B) {
            float *o = dbg + 5 * (size_t)(r0 + row);
            o[0] = T.sc[row * 4 + 3]; o[1] = T.Xn[row * AT_KIN + ns]; o[2] = q1; o[3] = q2; o[4] = y;
        }
        return;
    }
    __syncthreads();
    ddpg_critic_online(L, T, r0, B, y);
}
// (ddpg_critic_fwd_body's two instances)
__device__ __forceinline__ void td3_critic_fwd_body(const Td3Dev &T3, int B, int gate, float *__restrict__ dbg, unsigned char *dg_smem) {
    if (T3.v[0].n_step > 1) td3_critic_fwd_pass<true>(T3, B, gate, dbg, dg_smem);
    else td3_critic_fwd_pass<false>(T3, B, gate, dbg, dg_smem);
}
__global__ void __launch_bounds__(AT_THREADS) k_td3_critic_fwd(Td3Dev T3, int B, int gate, float *__restrict__ dbg) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dg_smem[];
    td3_critic_fwd_body(T3, B, gate, dbg, dg_smem);
}

// which = 1: both critics (gridDim.y = 2); which = 0: the actor, from view 0's workspace (gridDim.y = 1), if the delayed half is due
__device__ __forceinline__ void td3_wgrad_body(const Td3Dev &T3, int which, int Bp, int gate, double (*part_s)[256]) {
    if (!which && !td3_due(T3, gate)) return;
    ddpg_wgrad_body(T3.v[blockIdx.y], which, Bp, gate, part_s);
}
__global__ void __launch_bounds__(64 * DG_WG_WAVES) k_td3_wgrad(Td3Dev T3, int which, int Bp, int gate) {
    __shared__ double part_s[DG_WG_WAVES][256];
    td3_wgrad_body(T3, which, Bp, gate, part_s);
}

__device__ __forceinline__ void td3_actor_fwd_body(const Td3Dev &T3, int B, int gate, unsigned char *dg_smem) {
    if (!td3_due(T3, gate)) return;
    ddpg_actor_fwd_body(T3.v[0], B, gate, dg_smem);
}
__global__ void __launch_bounds__(AT_THREADS) k_td3_actor_fwd(Td3Dev T3, int B, int gate) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dg_smem[];
    td3_actor_fwd_body(T3, B, gate, dg_smem);
}

// Adam step of critic blockIdx.y with its own moments, beta powers and ticket; the target stays (t0 / t1 are re-packed from the unchanged target)
__device__ __forceinline__ void td3_adam_critics_body(const Td3Dev &T3, float lr, int gate) {
    const DdpgDev &L = T3.v[blockIdx.y];
    if (!ddpg_gate(L, gate)) return;
    const DdpgNet &net = L.q;
    const int np = dg_nparam(L.h1p, L.h2p);
    const float pw1 = net.bpow[0] * L.beta1, pw2 = net.bpow[1] * L.beta2;
    const float step = lr / (1.0f - pw1), bc2s = sqrtf(1.0f - pw2);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < np; i += gridDim.x * blockDim.x) {
        const float w = ddpg_adam_step(L, net, i, net.w[i], step, bc2s);
        net.w[i] = w;
        ddpg_repack(L, net, i, w, net.wt[i]);
    }
    __syncthreads();
    if (threadIdx.x == 0 && dg_last_block(L.tick + DG_T_ADAM + 1, gridDim.x)) { net.bpow[0] = pw1; net.bpow[1] = pw2; }
}
__global__ void __launch_bounds__(256) k_td3_adam_critics(Td3Dev T3, float lr, int gate) { td3_adam_critics_body(T3, lr, gate); }

// blockIdx.y = 0: the actor (Adam step, Polyak), 1 and 2: critic 1 and 2 (Polyak), all with the re-pack and only if the delayed half is due.
// The last workgroup of the whole grid advances the actor's beta powers (if it stepped) and ends the update.
__device__ __forceinline__ void td3_adam_finish_body(const Td3Dev &T3, float lr, int gate) {
    const DdpgDev &L = T3.v[blockIdx.y == 2];
    if (!ddpg_gate(L, gate)) return;
    const DdpgNet &net = blockIdx.y ? L.q : L.pi;
    const int np = dg_nparam(L.h1p, L.h2p);
    const long long upd = L.cnt[DG_UPDATES];
    const bool due = (upd + 1) % T3.delay == 0;
    const float pw1 = L.pi.bpow[0] * L.beta1, pw2 = L.pi.bpow[1] * L.beta2;
    const float step = lr / (1.0f - pw1), bc2s = sqrtf(1.0f - pw2);
    if (due)
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < np; i += gridDim.x * blockDim.x) {
            float w = net.w[i];
            if (blockIdx.y == 0) { w = ddpg_adam_step(L, net, i, w, step, bc2s); net.w[i] = w; }
            const float wt = L.omtau * net.wt[i] + L.tau * w;
            net.wt[i] = wt;
            ddpg_repack(L, net, i, w, wt);
        }
    __syncthreads();
    if (threadIdx.x == 0 && dg_last_block(T3.tick, gridDim.x * gridDim.y)) {
        if (due) { L.pi.bpow[0] = pw1; L.pi.bpow[1] = pw2; }
        L.cnt[DG_UPDATES] = upd + 1;
    }
}
__global__ void __launch_bounds__(256) k_td3_adam_finish(Td3Dev T3, float lr, int gate) { td3_adam_finish_body(T3, lr, gate); }

// loss 1, loss 2, mean Q1, mean Q2 of the last minibatch, fill, updates -> out [6] fp64 (ddpg_stats_body's fixed summation order)
__device__ __forceinline__ void td3_stats_body(const Td3Dev &T3, int B, double *out) {
    const int lane = threadIdx.x;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int r = lane; r < B; r += 64)
        for (int c = 0; c < 2; ++c) { s[c] += (double)T3.v[c].arow[2 * r]; s[2 + c] += (double)T3.v[c].arow[2 * r + 1]; }
    for (int o = 1; o < 64; o <<= 1)
        for (int c = 0; c < 4; ++c) s[c] += __shfl_xor(s[c], o);
    if (lane == 0) {
        for (int c = 0; c < 4; ++c) out[c] = s[c] / (double)B;
        out[4] = (double)T3.v[0].cnt[DG_FILL]; out[5] = (double)T3.v[0].cnt[DG_UPDATES];
    }
}
__global__ void __launch_bounds__(64) k_td3_stats(Td3Dev T3, int B, double *out) { td3_stats_body(T3, B, out); }

}  // namespace stmpc
