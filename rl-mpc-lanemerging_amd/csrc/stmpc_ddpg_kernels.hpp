// stmpc_ddpg_kernels.hpp -- an on-device DDPG learner next to the vector environment: replay ring, fused update, acting with exploration noise.
// The algorithm restates the `all` library's ddpg preset (the reference's TRAIN_DDPG, ddpg.py:44-80); the networks have the shapes of the
// reference's checkpoints: actor (n_obs + 1) -> h1 -> ReLU -> h2 -> ReLU -> 1 -> tanh * scale + mean, critic (n_obs + 2) -> h1 -> ReLU -> h2 -> ReLU -> 1,
// float32 like the reference's modules.
//
// One update is six launches whose shapes depend on (B, network shape) alone; every counter (ring cursor, fill, frames, update index, Adam's
// beta powers) lives in device memory, so a chain act -> env step -> push -> updates needs no host synchronisation and can be captured as a graph:
//   k_ddpg_critic_fwd   one workgroup per 16 minibatch rows: draws the rows' replay indices (splitmix64 of seed, update index, row), gathers them,
//                       pi_target(s'), Q_target(s', a'), y, Q(s, a), and the backward pass down to dZ1; activations stay in LDS, the matrix products
//                       are v_mfma_f32_16x16x4_f32 loops over actor_layer's packed operands (ddpg_layer: short summation chains); X, H1, H2, dZ2, dZ1, dz go to a workspace for the weight gradients
//   k_ddpg_wgrad        dW = dZ^T * H: one workgroup per 16 x 16 output tile, the batch (K = B) dealt to eight waves in 16-row groups, the eight partial
//                       tiles added in wave order through LDS: a fixed summation order, no float atomics, no cross-workgroup partial sums.
//                       The bias gradients and the last layer's are the same product with a vector of ones / dz as one operand
//   k_ddpg_adam         Adam (bias-corrected; the beta powers are running float32 products kept on the device) + the Polyak update of the target +
//                       the re-packing of both into the lane order actor_layer consumes (and of W1^T, the backward pass's operand)
//   k_ddpg_actor_fwd    pi(s), Q(s, pi(s)) with the critic as it is now, dQ/da through the critic, the tanh squash and the actor down to dZ1
//   k_ddpg_wgrad, k_ddpg_adam for the actor.
// Parameters are kept row-major and PADDED (input width 32, hidden widths to multiples of 16; pad entries are zero and stay zero: their gradients are
// exact zeros) so that biases and the last layer are read in place; minibatch rows are padded to a multiple of 16 with zero loss weight.
// Counters that several workgroups read and one must advance are advanced by the LAST workgroup to finish (an integer ticket), after every
// workgroup has read them.
#pragma once
#include "stmpc_actor_kernels.hpp"

namespace stmpc {

constexpr int DG_ROW = 68;          // replay row, float32: [0, 32) s, time feature, action, zeros; [32, 64) s', time feature, zeros; 64 reward; 65 mask
constexpr int DG_R = 64, DG_MASK = 65;
constexpr int DG_DONE = 67;         // terminated || truncated, written by the push of a learner with n_step > 1 (stmpc_nstep_kernels.hpp); else zero
constexpr int DG_WG_WAVES = 8;      // waves per weight-gradient tile
// counters (int64): ring cursor, fill, updates done, acting calls with noise, frames pushed
enum { DG_CURSOR = 0, DG_FILL = 1, DG_UPDATES = 2, DG_ACTS = 3, DG_FRAMES = 4, DG_NCNT = 8 };
// tickets (uint32): push, act, adam of the critic, adam of the actor
enum { DG_T_PUSH = 0, DG_T_ACT = 1, DG_T_ADAM = 2, DG_NTICK = 4 };

struct DdpgNet {                    // one network and everything derived from it
    float *w, *wt, *m, *v, *g;      // padded row-major: W0 [h1p][32] | b0 [h1p] | W1 [h2p][h1p] | b1 [h2p] | W2 [h2p] | b2 [4]: online, target, Adam moments, gradient
    float *p0, *p1, *p1t;           // online W0, W1 packed for actor_layer; W1^T packed ([h1p / 16][h2p / 16][64][4])
    float *t0, *t1;                 // target W0, W1 packed
    float *bpow;                    // [2]: beta1^t, beta2^t
    int n_in;
};

struct DdpgDev {
    DdpgNet pi, q;
    float *ring;                    // [capacity][DG_ROW]
    long long *cnt;                 // [DG_NCNT]
    unsigned int *tick;             // [DG_NTICK]
    float *aX, *aH1, *aH2, *aD2, *aD1, *adz, *arow;   // workspace of one minibatch: [Bp][32], [Bp][h1p], [Bp][h2p], [Bp][h2p], [Bp][h1p], [Bp], [Bp][2] (loss, Q)
    int n_obs, h1p, h2p, h1, h2, capacity;
    long long replay_start;
    unsigned long long seed;
    float gamma, tau, beta1, beta2, omb1, omb2, omtau, eps, time_scale, scale, mean, noise_std, a_low, a_high;
    // prioritised replay (stmpc_per_kernels.hpp); all null / 0 on a learner that samples uniformly, whose kernels then do what they did without these
    double *tree;                   // [2 * per_L - 1] sum tree
    long long *idx;                 // [Bp] ring rows of the current update's minibatch
    float *aw, *atd;                // [Bp] importance weights; [Bp] Q - y of the last critic pass
    double per_alpha, per_beta, per_min, per_max;
    long long per_L;                // leaves: capacity rounded up to a power of two
    // multi-step returns (stmpc_nstep_kernels.hpp); n_step <= 1 on a learner with one-step targets, whose kernels then do what they did without these
    int n_step, rows_push;          // the window's length n (<= 16) and the rows N of every push
};
struct NstepWin { float R, disc; long long last; int m; };   // a row's window: return, gamma^m, the ring row of its last transition, its length

__host__ __device__ inline int dg_o_b0(int h1p) { return h1p * AT_KIN; }
__host__ __device__ inline int dg_o_w1(int h1p) { return h1p * AT_KIN + h1p; }
__host__ __device__ inline int dg_o_b1(int h1p, int h2p) { return dg_o_w1(h1p) + h2p * h1p; }
__host__ __device__ inline int dg_o_w2(int h1p, int h2p) { return dg_o_b1(h1p, h2p) + h2p; }
__host__ __device__ inline int dg_o_b2(int h1p, int h2p) { return dg_o_w2(h1p, h2p) + h2p; }
__host__ __device__ inline int dg_nparam(int h1p, int h2p) { return dg_o_b2(h1p, h2p) + 4; }

__host__ __device__ inline unsigned long long dg_mix(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// splitmix64 of (seed, a, b): two rounds of the generator stmpc_env_episode_seed uses
__host__ __device__ inline unsigned long long dg_hash(unsigned long long seed, unsigned long long a, unsigned long long b) {
    const unsigned long long G = 0x9E3779B97F4A7C15ull;
    return dg_mix(dg_mix(seed + G * (a + 1ull)) + G * (b + 1ull));
}
constexpr unsigned long long DG_NOISE_STREAM = 0x6E6F697365ull;     // the noise draws' seed is seed ^ this

// the last workgroup of a launch to get here (one call per workgroup, by thread 0, after the workgroup's reads of the counters) returns true
__device__ __forceinline__ bool dg_last_block(unsigned int *ticket, unsigned int nblocks) {
    __threadfence();
    const unsigned int t = atomicAdd(ticket, 1u);
    if (t + 1u != nblocks) return false;
    *ticket = 0u;
    return true;
}

// ring row of minibatch row r: the sampling step's (prioritised replay) or the hash's
__device__ __forceinline__ long long dg_row_index(const DdpgDev &L, long long upd, long long fill, int r) {
    return L.idx ? L.idx[r] : (long long)(dg_hash(L.seed, (unsigned long long)upd, (unsigned long long)r) % (unsigned long long)fill);
}
__device__ __forceinline__ void per_push_tree(const DdpgDev &L, long long cursor, int N);      // stmpc_per_kernels.hpp
__device__ __forceinline__ NstepWin nstep_window(const DdpgDev &L, long long i, long long cursor);                      // stmpc_nstep_kernels.hpp
__device__ __forceinline__ void nstep_gather_tile(const DdpgDev &L, float *X, float *Xn, float *sc, long long idx, bool valid);   // stmpc_nstep_kernels.hpp
__device__ __forceinline__ void nstep_gather_body(const DdpgDev &L, int B, float *out, long long fill, long long upd);  // stmpc_nstep_kernels.hpp

// ---- replay ---------------------------------------------------------------------------------------------------------------------------------
// (k_dqn_push of stmpc_dqn_kernels.hpp is a sibling of ddpg_push_body with an int32 action column and no time feature: a fix here belongs there too)
// (every kernel's body is a __device__ function of the learner's struct: the single-learner entry passes its by-value argument, the population
// entry of stmpc_ddpg_pop_kernels.hpp the member blockIdx.y selects)
__device__ __forceinline__ void ddpg_push_body(const DdpgDev &L, int N, const float *__restrict__ obs, const float *__restrict__ next_obs, const float *__restrict__ final_obs,
                                               int obs_stride, const int *__restrict__ ticks, const int *__restrict__ next_ticks, const double *__restrict__ action,
                                               const double *__restrict__ reward, const unsigned char *__restrict__ term, const unsigned char *__restrict__ trunc) {
    const long long cursor = L.cnt[DG_CURSOR], fill = L.cnt[DG_FILL], frames = L.cnt[DG_FRAMES];
    const int ns = L.n_obs + 1;
    const float done_v = L.n_step > 1 ? 1.f : 0.f;                  // what a done row's DG_DONE column gets (hoisted: one test per launch, not per column)
    for (long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x; x < (long long)N * DG_ROW; x += (long long)gridDim.x * blockDim.x) {
        const int e = (int)(x / DG_ROW), c = (int)(x % DG_ROW);
        const bool done = term[e] || trunc[e];
        float v = 0.f;
        if (c < L.n_obs) v = obs[(size_t)e * obs_stride + c];
        else if (c == L.n_obs) v = L.time_scale * (float)ticks[e];
        else if (c == ns) v = (float)action[e];
        else if (c >= 32 && c < 32 + L.n_obs) v = (done && final_obs ? final_obs : next_obs)[(size_t)e * obs_stride + (c - 32)];
        else if (c == 32 + L.n_obs) v = L.time_scale * (float)((done || !next_ticks) ? ticks[e] + 1 : next_ticks[e]);
        else if (c == DG_R) v = (float)reward[e];
        else if (c == DG_MASK) v = term[e] ? 0.f : 1.f;
        else if (c == DG_DONE) v = done ? done_v : 0.f;
        L.ring[(size_t)((cursor + e) % L.capacity) * DG_ROW + c] = v;
    }
    __syncthreads();
    __shared__ int last_s;
    const bool last = threadIdx.x == 0 && dg_last_block(L.tick + DG_T_PUSH, gridDim.x);
    if (last) {
        L.cnt[DG_CURSOR] = (cursor + N) % L.capacity;
        L.cnt[DG_FILL] = fill + N < L.capacity ? fill + N : L.capacity;
        L.cnt[DG_FRAMES] = frames + N;
    }
    if (!L.tree) return;
    if (threadIdx.x == 0) last_s = last;
    __syncthreads();
    if (last_s) per_push_tree(L, cursor, N);                       // the new rows' priorities, in this one workgroup
}
__global__ void __launch_bounds__(256) k_replay_push(DdpgDev L, int N, const float *__restrict__ obs, const float *__restrict__ next_obs, const float *__restrict__ final_obs,
                                                     int obs_stride, const int *__restrict__ ticks, const int *__restrict__ next_ticks, const double *__restrict__ action,
                                                     const double *__restrict__ reward, const unsigned char *__restrict__ term, const unsigned char *__restrict__ trunc) {
    ddpg_push_body(L, N, obs, next_obs, final_obs, obs_stride, ticks, next_ticks, action, reward, term, trunc);
}

// the minibatch of the current update index, gathered: out [B][DG_ROW] (tests and diagnostics; the update gathers in its first kernel)
__global__ void k_replay_gather(DdpgDev L, int B, float *out) {
    const long long fill = L.cnt[DG_FILL], upd = L.cnt[DG_UPDATES];
    if (fill < 1) return;
    if (L.n_step > 1) { nstep_gather_body(L, B, out, fill, upd); return; }
    for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < B * DG_ROW; x += gridDim.x * blockDim.x) {
        const int r = x / DG_ROW, c = x % DG_ROW;
        const long long idx = dg_row_index(L, upd, fill, r);
        out[x] = L.ring[(size_t)idx * DG_ROW + c];
    }
}

// ---- pieces of the forward / backward passes ----------------------------------------------------------------------------------------------------
// One layer of the update's passes, out[16][np] from in[16][kp] * W^T with W packed as actor_layer's.  BWD = false: out = relu(. + bias); BWD = true:
// out (in place over the forward activation) = out > 0 ? . : 0 (no bias, the ReLU's mask).  Same operands and lane order as actor_layer, another
// summation order: every 16-wide k block is summed on its own (four independent MFMAs of 4 k each, added pairwise) and the block sums are added
// in k order in fp64 (four VALU additions per four MFMAs) and rounded to float32 once, with the bias -- instead of one chain of kp fused multiply-adds.  The replay's rows resemble each other, so a long chain's rounding
// error repeats from row to row and survives the mean over the minibatch; measured against the float64 twin the short float32 chains are what keeps the
// gradients within the float32 twin's error (tests/test_learner.py).  Acting keeps actor_layer itself.
// (dqn_out_layer of stmpc_dqn_kernels.hpp is the BWD = false case without the ReLU, same loops and summation order: a fix here belongs there too)
template <bool BWD>
__device__ __forceinline__ void ddpg_layer(const float *in, int in_ld, int kp, const float *packed, const float *bias, float *out, int out_ld, int np) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int j = lane & 15, kk = lane >> 4;
    const int kblocks = kp >> 4;
    const float *ap = in + (size_t)j * in_ld + 4 * kk;
    const at_f4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int nt = wave; nt < (np >> 4); nt += nwaves) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        const at_f4 *bp = (const at_f4 *)packed + ((size_t)nt * kblocks) * 64 + lane;
        for (int kb = 0; kb < kblocks; ++kb) {
            const at_f4 b = bp[(size_t)kb * 64];
            const at_f4 a = *(const at_f4 *)(ap + kb * 16);
            const at_f4 t0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, zero, 0, 0, 0);
            const at_f4 t1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, zero, 0, 0, 0);
            const at_f4 t2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, zero, 0, 0, 0);
            const at_f4 t3 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, zero, 0, 0, 0);
            const at_f4 blk = (t0 + t1) + (t2 + t3);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] += (double)blk[r];
        }
        const int n = nt * 16 + j;
        const double bv = BWD ? 0.0 : (double)bias[n];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float *o = out + (size_t)(kk * 4 + r) * out_ld + n;
            const float v = (float)(acc[r] + bv);
            if (BWD) *o = *o > 0.f ? v : 0.f;
            else *o = v > 0.f ? v : 0.f;
        }
    }
}

// tanh rounded once to float32 (through fp64): the device's tanhf is good to a couple of ulps, but its error has a sign, and a bias of that size in
// pi_target(s') shifts every y of a minibatch the same way -- visible in the gradients of a critic whose mean TD error is small
__device__ __forceinline__ float ddpg_tanh(float z) { return (float)tanh((double)z); }

// z[row] = H2[row] . w2 + b2 for the 16 rows: 32 lanes per row (512 threads), the butterfly of k_actor_eval; every lane of a row gets the sum
__device__ __forceinline__ float ddpg_out_dot(const float *H2, int h2_ld, int h2p, const float *w2, float b2) {
    const int row = threadIdx.x >> 5, part = threadIdx.x & 31;
    double s = 0.0;                                                 // (float32 products are exact in fp64)
    for (int n = part; n < h2p; n += 32) s += (double)H2[(size_t)row * h2_ld + n] * (double)w2[n];
    s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4); s += __shfl_xor(s, 8); s += __shfl_xor(s, 16);
    return (float)(s + (double)b2);
}

// LDS tile [16][ld] -> global [16][w] (rows of a workspace array)
__device__ __forceinline__ void ddpg_store_tile(const float *t, int ld, float *g, int w) {
    for (int x = threadIdx.x; x < AT_TM * w; x += blockDim.x) g[x] = t[(size_t)(x / w) * ld + (x % w)];
}

struct DdpgTile {                   // LDS of the two per-tile kernels
    float *X, *Xn, *H1, *H2, *sc;   // [16][32], [16][32], [16][h1p + 4], [16][h2p + 4], scalars [16][4]
    int h1_ld, h2_ld;
};
__device__ __forceinline__ DdpgTile ddpg_tile(unsigned char *smem, int h1p, int h2p) {
    DdpgTile t;
    t.h1_ld = h1p + 4; t.h2_ld = h2p + 4;
    t.X = (float *)smem;
    t.Xn = t.X + AT_TM * AT_KIN;
    t.sc = t.Xn + AT_TM * AT_KIN;
    t.H1 = t.sc + AT_TM * 4;
    t.H2 = t.H1 + (size_t)AT_TM * t.h1_ld;
    return t;
}
__host__ inline size_t ddpg_tile_bytes(int h1p, int h2p) {
    return ((size_t)2 * AT_TM * AT_KIN + AT_TM * 4 + (size_t)AT_TM * (h1p + 4) + (size_t)AT_TM * (h2p + 4)) * sizeof(float);
}

// may this update run?  (the `all` preset's _should_train: more frames seen than replay_start); gate = 0 for the gradient-only debug entry
__device__ __forceinline__ bool ddpg_gate(const DdpgDev &L, int gate) {
    return L.cnt[DG_FILL] >= 1 && (!gate || L.cnt[DG_FRAMES] > L.replay_start);
}

// ---- critic pass ------------------------------------------------------------------------------------------------------------------------------
// (its stages are functions of their own because the TD3 critic pass of stmpc_td3_kernels.hpp is made of the same ones)
// gather: 32 lanes per row; X = (s, a), Xn = s', sc = (reward, mask); n_step > 1: s' and the mask of the window's last row, sc = (R, mask, gamma^m)
// (NS: the n-step instance.  The passes that form a target are compiled twice and entered through ONE test of L.n_step, so that the one-step
// instance is the one-step learner's own instruction stream)
template <bool NS>
__device__ __forceinline__ void ddpg_gather_tile(const DdpgDev &L, const DdpgTile &T, int r0, int B, long long fill, long long upd) {
    const int row = threadIdx.x >> 5, c = threadIdx.x & 31;
    const bool valid = r0 + row < B;
    const long long idx = valid ? dg_row_index(L, upd, fill, r0 + row) : 0;
    const float *src = L.ring + (size_t)idx * DG_ROW;
    if (NS) { nstep_gather_tile(L, T.X, T.Xn, T.sc, idx, valid); return; }
    T.X[row * AT_KIN + c] = valid ? src[c] : 0.f;
    T.Xn[row * AT_KIN + c] = valid ? src[32 + c] : 0.f;
    if (c < 2) T.sc[row * 4 + c] = valid ? src[DG_R + c] : 0.f;
}
// the target's discount of this thread's row: gamma, or gamma^m of the row's window (ddpg_gather_tile left it in sc; read before dz takes its place)
template <bool NS>
__device__ __forceinline__ float ddpg_discount(const DdpgDev &L, const DdpgTile &T) {
    return NS ? T.sc[(threadIdx.x >> 5) * 4 + 2] : L.gamma;
}
// the target networks on Xn: the output of `net`'s target (pre-tanh for the actor, Q for a critic), in every lane of the row; the caller's barrier comes before H1 / H2 are written again
__device__ __forceinline__ float ddpg_target_out(const DdpgDev &L, const DdpgNet &net, const DdpgTile &T) {
    const int ob0 = dg_o_b0(L.h1p), ob1 = dg_o_b1(L.h1p, L.h2p), ow2 = dg_o_w2(L.h1p, L.h2p), ob2 = dg_o_b2(L.h1p, L.h2p);
    ddpg_layer<false>(T.Xn, AT_KIN, AT_KIN, net.t0, net.wt + ob0, T.H1, T.h1_ld, L.h1p);
    __syncthreads();
    ddpg_layer<false>(T.H1, T.h1_ld, L.h1p, net.t1, net.wt + ob1, T.H2, T.h2_ld, L.h2p);
    __syncthreads();
    return ddpg_out_dot(T.H2, T.h2_ld, L.h2p, net.wt + ow2, net.wt[ob2]);
}
// Q(s, a) of the online critic L.q on X against the target y, and the backward pass down to dZ1; everything the weight gradients need goes to L's workspace
__device__ __forceinline__ void ddpg_critic_online(const DdpgDev &L, const DdpgTile &T, int r0, int B, float y) {
    const int tid = threadIdx.x, row = tid >> 5, part = tid & 31;
    const int ob0 = dg_o_b0(L.h1p), ob1 = dg_o_b1(L.h1p, L.h2p), ow2 = dg_o_w2(L.h1p, L.h2p), ob2 = dg_o_b2(L.h1p, L.h2p);
    ddpg_layer<false>(T.X, AT_KIN, AT_KIN, L.q.p0, L.q.w + ob0, T.H1, T.h1_ld, L.h1p);
    __syncthreads();
    ddpg_layer<false>(T.H1, T.h1_ld, L.h1p, L.q.p1, L.q.w + ob1, T.H2, T.h2_ld, L.h2p);
    __syncthreads();
    const float qv = ddpg_out_dot(T.H2, T.h2_ld, L.h2p, L.q.w + ow2, L.q.w[ob2]);
    const bool valid = r0 + row < B;
    const float diff = qv - y;
    // d mean((Q - y)^2) / dQ; prioritised replay: d mean(w (Q - y)^2) / dQ
    const float dz = valid ? (L.aw ? ((2.0f * L.aw[r0 + row]) * diff) / (float)B : (2.0f * diff) / (float)B) : 0.f;
    if (part == 0) {
        if (L.atd) L.atd[r0 + row] = valid ? diff : 0.f;
        T.sc[row * 4 + 2] = dz;
        L.adz[r0 + row] = dz;
        L.arow[2 * (r0 + row)] = valid ? diff * diff : 0.f;
        L.arow[2 * (r0 + row) + 1] = valid ? qv : 0.f;
    }
    ddpg_store_tile(T.X, AT_KIN, L.aX + (size_t)r0 * AT_KIN, AT_KIN);
    ddpg_store_tile(T.H1, T.h1_ld, L.aH1 + (size_t)r0 * L.h1p, L.h1p);
    ddpg_store_tile(T.H2, T.h2_ld, L.aH2 + (size_t)r0 * L.h2p, L.h2p);
    __syncthreads();
    // dZ2 = dz * w2 where H2 > 0 (in place), dZ1 = dZ2 * W1 where H1 > 0 (in place)
    for (int x = tid; x < AT_TM * L.h2p; x += blockDim.x) {
        const int r = x / L.h2p, n = x % L.h2p;
        float *h = T.H2 + (size_t)r * T.h2_ld + n;
        *h = *h > 0.f ? T.sc[r * 4 + 2] * L.q.w[ow2 + n] : 0.f;
    }
    __syncthreads();
    ddpg_layer<true>(T.H2, T.h2_ld, L.h2p, L.q.p1t, nullptr, T.H1, T.h1_ld, L.h1p);
    ddpg_store_tile(T.H2, T.h2_ld, L.aD2 + (size_t)r0 * L.h2p, L.h2p);
    __syncthreads();
    ddpg_store_tile(T.H1, T.h1_ld, L.aD1 + (size_t)r0 * L.h1p, L.h1p);
}
template <bool NS>
__device__ __forceinline__ void ddpg_critic_fwd_pass(const DdpgDev &L, int B, int gate, unsigned char *dg_smem) {
    if (!ddpg_gate(L, gate)) return;
    const DdpgTile T = ddpg_tile(dg_smem, L.h1p, L.h2p);
    const int tid = threadIdx.x, r0 = blockIdx.x * AT_TM, ns = L.n_obs + 1;
    const int row = tid >> 5, part = tid & 31;
    ddpg_gather_tile<NS>(L, T, r0, B, L.cnt[DG_FILL], L.cnt[DG_UPDATES]);
    __syncthreads();
    // a' = pi_target(s')
    const float z = ddpg_target_out(L, L.pi, T);
    if (part == 0) T.Xn[row * AT_KIN + ns] = ddpg_tanh(z) * L.scale + L.mean;
    __syncthreads();
    // Q_target(s', a')
    const float qn = ddpg_target_out(L, L.q, T);
    const float y = T.sc[row * 4 + 0] + (ddpg_discount<NS>(L, T) * T.sc[row * 4 + 1]) * qn;
    __syncthreads();
    // Q(s, a)
    ddpg_critic_online(L, T, r0, B, y);
}
__device__ __forceinline__ void ddpg_critic_fwd_body(const DdpgDev &L, int B, int gate, unsigned char *dg_smem) {
    if (L.n_step > 1) ddpg_critic_fwd_pass<true>(L, B, gate, dg_smem);
    else ddpg_critic_fwd_pass<false>(L, B, gate, dg_smem);
}
__global__ void __launch_bounds__(AT_THREADS) k_ddpg_critic_fwd(DdpgDev L, int B, int gate) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dg_smem[];
    ddpg_critic_fwd_body(L, B, gate, dg_smem);
}

// ---- actor pass -------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ddpg_actor_fwd_body(const DdpgDev &L, int B, int gate, unsigned char *dg_smem) {
    if (!ddpg_gate(L, gate)) return;
    const DdpgTile T = ddpg_tile(dg_smem, L.h1p, L.h2p);
    const int tid = threadIdx.x, r0 = blockIdx.x * AT_TM, ns = L.n_obs + 1;
    const long long fill = L.cnt[DG_FILL], upd = L.cnt[DG_UPDATES];
    const int row = tid >> 5, part = tid & 31;
    const bool valid = r0 + row < B;
    {   // gather s: X = (s, 0) for the actor, Xn = (s, pi(s)) for the critic
        const long long idx = valid ? dg_row_index(L, upd, fill, r0 + row) : 0;
        const float v = valid && part < ns ? L.ring[(size_t)idx * DG_ROW + part] : 0.f;
        T.X[row * AT_KIN + part] = v;
        T.Xn[row * AT_KIN + part] = v;
    }
    __syncthreads();
    const int ob0 = dg_o_b0(L.h1p), ob1 = dg_o_b1(L.h1p, L.h2p), ow2 = dg_o_w2(L.h1p, L.h2p), ob2 = dg_o_b2(L.h1p, L.h2p);
    // a = pi(s)
    ddpg_layer<false>(T.X, AT_KIN, AT_KIN, L.pi.p0, L.pi.w + ob0, T.H1, T.h1_ld, L.h1p);
    __syncthreads();
    ddpg_layer<false>(T.H1, T.h1_ld, L.h1p, L.pi.p1, L.pi.w + ob1, T.H2, T.h2_ld, L.h2p);
    __syncthreads();
    const float th = ddpg_tanh(ddpg_out_dot(T.H2, T.h2_ld, L.h2p, L.pi.w + ow2, L.pi.w[ob2]));
    if (part == 0) T.Xn[row * AT_KIN + ns] = th * L.scale + L.mean;
    ddpg_store_tile(T.X, AT_KIN, L.aX + (size_t)r0 * AT_KIN, AT_KIN);
    ddpg_store_tile(T.H1, T.h1_ld, L.aH1 + (size_t)r0 * L.h1p, L.h1p);
    ddpg_store_tile(T.H2, T.h2_ld, L.aH2 + (size_t)r0 * L.h2p, L.h2p);
    __syncthreads();
    // Q(s, a) with the critic as it is now, and dQ/da through it
    ddpg_layer<false>(T.Xn, AT_KIN, AT_KIN, L.q.p0, L.q.w + ob0, T.H1, T.h1_ld, L.h1p);
    __syncthreads();
    ddpg_layer<false>(T.H1, T.h1_ld, L.h1p, L.q.p1, L.q.w + ob1, T.H2, T.h2_ld, L.h2p);
    __syncthreads();
    for (int x = tid; x < AT_TM * L.h2p; x += blockDim.x) {
        const int r = x / L.h2p, n = x % L.h2p;
        float *h = T.H2 + (size_t)r * T.h2_ld + n;
        *h = *h > 0.f ? L.q.w[ow2 + n] : 0.f;
    }
    __syncthreads();
    ddpg_layer<true>(T.H2, T.h2_ld, L.h2p, L.q.p1t, nullptr, T.H1, T.h1_ld, L.h1p);
    __syncthreads();
    double dqda_d = 0.0;
    for (int n = part; n < L.h1p; n += 32) dqda_d += (double)T.H1[(size_t)row * T.h1_ld + n] * (double)L.q.w[(size_t)n * AT_KIN + ns];
    dqda_d += __shfl_xor(dqda_d, 1); dqda_d += __shfl_xor(dqda_d, 2); dqda_d += __shfl_xor(dqda_d, 4); dqda_d += __shfl_xor(dqda_d, 8); dqda_d += __shfl_xor(dqda_d, 16);
    const float dqda = (float)dqda_d;
    // loss = -mean(Q): dz = -(1 / B) dQ/da * scale * (1 - tanh^2)
    const float dz = valid ? ((-dqda / (float)B) * L.scale) * (1.0f - th * th) : 0.f;
    if (part == 0) { T.sc[row * 4 + 2] = dz; L.adz[r0 + row] = dz; }
    __syncthreads();
    // the actor's backward pass: its H2, H1 come back from the workspace (this workgroup wrote them above)
    for (int x = tid; x < AT_TM * L.h2p; x += blockDim.x) {
        const int r = x / L.h2p, n = x % L.h2p;
        T.H2[(size_t)r * T.h2_ld + n] = L.aH2[(size_t)(r0 + r) * L.h2p + n] > 0.f ? T.sc[r * 4 + 2] * L.pi.w[ow2 + n] : 0.f;
    }
    for (int x = tid; x < AT_TM * L.h1p; x += blockDim.x) {
        const int r = x / L.h1p, n = x % L.h1p;
        T.H1[(size_t)r * T.h1_ld + n] = L.aH1[(size_t)(r0 + r) * L.h1p + n];
    }
    __syncthreads();
    ddpg_layer<true>(T.H2, T.h2_ld, L.h2p, L.pi.p1t, nullptr, T.H1, T.h1_ld, L.h1p);
    ddpg_store_tile(T.H2, T.h2_ld, L.aD2 + (size_t)r0 * L.h2p, L.h2p);
    __syncthreads();
    ddpg_store_tile(T.H1, T.h1_ld, L.aD1 + (size_t)r0 * L.h1p, L.h1p);
}
__global__ void __launch_bounds__(AT_THREADS) k_ddpg_actor_fwd(DdpgDev L, int B, int gate) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dg_smem[];
    ddpg_actor_fwd_body(L, B, gate, dg_smem);
}

// ---- weight gradients ---------------------------------------------------------------------------------------------------------------------------
// One workgroup per 16 x 16 tile of out[i][j] = sum_b Lm[b][i] * Rm[b][j]; an operand with ld = 0 is a vector broadcast over its 16 columns
// (ones: the bias gradients; dz: the last layer's).  Jobs in blockIdx order: dW1, dW0, db1, db0, dW2, db2.
// k_dqn_wgrad (stmpc_dqn_kernels.hpp) launches the first four jobs only, its matrix output layer in the place of layer 1: the scalar head's jobs stay LAST.
__device__ __forceinline__ void ddpg_wgrad_body(const DdpgDev &L, int which, int Bp, int gate, double (*part_s)[256]) {
    if (!ddpg_gate(L, gate)) return;
    const DdpgNet &net = which ? L.q : L.pi;
    const int t1 = L.h2p >> 4, t0 = L.h1p >> 4;
    int job = blockIdx.x;
    const float *Lm, *Rm; int ldL, ldR, i0 = 0, j0 = 0, out_ld, rows_out; float *out; bool Lone = false, Rone = false;
    if (job < t1 * t0) { i0 = (job / t0) * 16; j0 = (job % t0) * 16; Lm = L.aD2; ldL = L.h2p; Rm = L.aH1; ldR = L.h1p; out = net.g + dg_o_w1(L.h1p); out_ld = L.h1p; rows_out = 16; }
    else if ((job -= t1 * t0) < t0 * 2) { i0 = (job / 2) * 16; j0 = (job % 2) * 16; Lm = L.aD1; ldL = L.h1p; Rm = L.aX; ldR = AT_KIN; out = net.g; out_ld = AT_KIN; rows_out = 16; }
    else if ((job -= t0 * 2) < t1) { j0 = job * 16; Lm = L.adz; ldL = 0; Lone = true; Rm = L.aD2; ldR = L.h2p; out = net.g + dg_o_b1(L.h1p, L.h2p); out_ld = 0; rows_out = 1; }
    else if ((job -= t1) < t0) { j0 = job * 16; Lm = L.adz; ldL = 0; Lone = true; Rm = L.aD1; ldR = L.h1p; out = net.g + dg_o_b0(L.h1p); out_ld = 0; rows_out = 1; }
    else if ((job -= t0) < t1) { j0 = job * 16; Lm = L.adz; ldL = 0; Rm = L.aH2; ldR = L.h2p; out = net.g + dg_o_w2(L.h1p, L.h2p); out_ld = 0; rows_out = 1; }
    else { Lm = L.adz; ldL = 0; Rm = L.adz; ldR = 0; Rone = true; out = net.g + dg_o_b2(L.h1p, L.h2p); out_ld = 0; rows_out = 1; }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 15, kk = lane >> 4;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const at_f4 zero = {0.f, 0.f, 0.f, 0.f};
    auto opa = [&](int ks) { const int b = ks * 4 + kk; return ks >= (Bp >> 2) ? 0.f : (Lone ? 1.0f : (ldL ? Lm[(size_t)b * ldL + i0 + j] : Lm[b])); };
    auto opb = [&](int ks) { const int b = ks * 4 + kk; return ks >= (Bp >> 2) ? 0.f : (Rone ? 1.0f : (ldR ? Rm[(size_t)b * ldR + j0 + j] : Rm[b])); };
    // 4 minibatch rows per MFMA; a wave takes groups of four such steps in turn, sums each group on its own (pairwise) and adds the group sums in order in fp64
    // (ddpg_layer's reasoning)
    for (int ks = wave * 4; ks < (Bp >> 2); ks += DG_WG_WAVES * 4) {
        const at_f4 t0 = __builtin_amdgcn_mfma_f32_16x16x4f32(opa(ks), opb(ks), zero, 0, 0, 0);
        const at_f4 t1 = __builtin_amdgcn_mfma_f32_16x16x4f32(opa(ks + 1), opb(ks + 1), zero, 0, 0, 0);
        const at_f4 t2 = __builtin_amdgcn_mfma_f32_16x16x4f32(opa(ks + 2), opb(ks + 2), zero, 0, 0, 0);
        const at_f4 t3 = __builtin_amdgcn_mfma_f32_16x16x4f32(opa(ks + 3), opb(ks + 3), zero, 0, 0, 0);
        const at_f4 blk = (t0 + t1) + (t2 + t3);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] += (double)blk[r];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) part_s[wave][(kk * 4 + r) * 16 + j] = acc[r];
    __syncthreads();
    const int x = threadIdx.x;
    if (x < 256) {
        double sd = part_s[0][x];
#pragma unroll
        for (int w = 1; w < DG_WG_WAVES; ++w) sd += part_s[w][x];       // wave order: fixed
        const float s = (float)sd;
        const int i = x >> 4, jj = x & 15;
        if (rows_out == 16) out[(size_t)(i0 + i) * out_ld + j0 + jj] = s;
        else if (i == 0 && (!Rone || jj == 0)) out[j0 + jj] = s;
    }
}
__global__ void __launch_bounds__(64 * DG_WG_WAVES) k_ddpg_wgrad(DdpgDev L, int which, int Bp, int gate) {
    __shared__ double part_s[DG_WG_WAVES][256];
    ddpg_wgrad_body(L, which, Bp, gate, part_s);
}

// ---- Adam + Polyak + re-pack ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ size_t dg_packed_index(int n, int k, int kblocks) {
    return ((((size_t)(n >> 4) * kblocks + (k >> 4)) * 64) + (n & 15) + 16 * ((k & 15) >> 2)) * 4 + (k & 3);
}
// one element's Adam step (bias-corrected through step = lr / (1 - beta1^t) and bc2s = sqrt(1 - beta2^t)): moments stored, the new weight returned
__device__ __forceinline__ float ddpg_adam_step(const DdpgDev &L, const DdpgNet &net, int i, float w, float step, float bc2s) {
    const float g = net.g[i];
    const float m = L.beta1 * net.m[i] + L.omb1 * g;
    const float v = L.beta2 * net.v[i] + L.omb2 * (g * g);
    const float denom = sqrtf(v) / bc2s + L.eps;
    net.m[i] = m; net.v[i] = v;
    return w - step * (m / denom);
}
// element i of the padded parameter array (online value w, target value wt) into the packed copies the layers consume
__device__ __forceinline__ void ddpg_repack(const DdpgDev &L, const DdpgNet &net, int i, float w, float wt) {
    const int ow1 = dg_o_w1(L.h1p), ob1 = dg_o_b1(L.h1p, L.h2p), ob0 = dg_o_b0(L.h1p);
    if (i < ob0) {
        const size_t p = dg_packed_index(i / AT_KIN, i % AT_KIN, AT_KIN >> 4);
        net.p0[p] = w; net.t0[p] = wt;
    } else if (i >= ow1 && i < ob1) {
        const int n = (i - ow1) / L.h1p, k = (i - ow1) % L.h1p;
        const size_t p = dg_packed_index(n, k, L.h1p >> 4);
        net.p1[p] = w; net.t1[p] = wt;
        net.p1t[dg_packed_index(k, n, L.h2p >> 4)] = w;
    }
}
// mode 0: Adam step with learning rate lr, Polyak, re-pack; mode 1: re-pack only (after stmpc_ddpg_set_params).  bump: this launch ends an update.
__device__ __forceinline__ void ddpg_adam_body(const DdpgDev &L, int which, float lr, int mode, int bump, int gate) {
    if (mode == 0 && !ddpg_gate(L, gate)) return;
    const DdpgNet &net = which ? L.q : L.pi;
    const int np = dg_nparam(L.h1p, L.h2p);
    const float pw1 = net.bpow[0] * L.beta1, pw2 = net.bpow[1] * L.beta2;
    const long long upd = L.cnt[DG_UPDATES];
    const float step = lr / (1.0f - pw1), bc2s = sqrtf(1.0f - pw2);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < np; i += gridDim.x * blockDim.x) {
        float w = net.w[i], wt = net.wt[i];
        if (mode == 0) {
            w = ddpg_adam_step(L, net, i, w, step, bc2s);
            wt = L.omtau * wt + L.tau * w;
            net.w[i] = w; net.wt[i] = wt;
        }
        ddpg_repack(L, net, i, w, wt);
    }
    __syncthreads();
    if (mode == 0 && threadIdx.x == 0 && dg_last_block(L.tick + DG_T_ADAM + which, gridDim.x)) {
        net.bpow[0] = pw1; net.bpow[1] = pw2;
        if (bump) L.cnt[DG_UPDATES] = upd + 1;
    }
}
__global__ void __launch_bounds__(256) k_ddpg_adam(DdpgDev L, int which, float lr, int mode, int bump, int gate) { ddpg_adam_body(L, which, lr, mode, bump, gate); }

// padded parameter layout -> the tensors one after the other, row-major, unpadded: W0 [h1][n_in] | b0 | W1 [h2][h1] | b1 | W2 [h2] | b2
__global__ void k_ddpg_unpad(DdpgDev L, int n_in, const float *__restrict__ src, float *__restrict__ dst) {
    const int n0 = L.h1 * n_in, n1 = n0 + L.h1, n2 = n1 + L.h2 * L.h1, n3 = n2 + L.h2, n4 = n3 + L.h2, total = n4 + 1;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        int s;
        if (i < n0) s = (i / n_in) * AT_KIN + i % n_in;
        else if (i < n1) s = dg_o_b0(L.h1p) + (i - n0);
        else if (i < n2) s = dg_o_w1(L.h1p) + ((i - n1) / L.h1) * L.h1p + (i - n1) % L.h1;
        else if (i < n3) s = dg_o_b1(L.h1p, L.h2p) + (i - n2);
        else if (i < n4) s = dg_o_w2(L.h1p, L.h2p) + (i - n3);
        else s = dg_o_b2(L.h1p, L.h2p);
        dst[i] = src[s];
    }
}

// last critic loss, mean Q of the last minibatch, fill, updates -> out [4] fp64; one workgroup, 64 strided partial sums in fp64, added by a butterfly: a fixed order
__device__ __forceinline__ void ddpg_stats_body(const DdpgDev &L, int B, double *out) {
    const int lane = threadIdx.x;
    double sl = 0.0, sq = 0.0;
    for (int r = lane; r < B; r += 64) { sl += (double)L.arow[2 * r]; sq += (double)L.arow[2 * r + 1]; }
    for (int o = 1; o < 64; o <<= 1) { sl += __shfl_xor(sl, o); sq += __shfl_xor(sq, o); }
    if (lane == 0) {
        out[0] = sl / (double)B; out[1] = sq / (double)B;
        out[2] = (double)L.cnt[DG_FILL]; out[3] = (double)L.cnt[DG_UPDATES];
    }
}
__global__ void __launch_bounds__(64) k_ddpg_stats(DdpgDev L, int B, double *out) { ddpg_stats_body(L, B, out); }

// ---- acting -------------------------------------------------------------------------------------------------------------------------------------
// a standard normal in float32 from one hash: Box-Muller on its two 24-bit draws, which are returned too
__device__ __forceinline__ float dg_gauss(unsigned long long h, unsigned int &u1, unsigned int &u2) {
    u1 = (unsigned int)(h >> 40); u2 = (unsigned int)((h >> 8) & 0xFFFFFFull);
    const float f1 = (float)(u1 + 1u) * 5.9604644775390625e-8f;      // (0, 1]: multiples of 2^-24, exact in float32
    const float f2 = (float)u2 * 5.9604644775390625e-8f;             // [0, 1)
    return sqrtf(-2.0f * logf(f1)) * cosf(6.2831855f * f2);
}
// action [N] fp64 = clip(pi(obs, time_scale * ticks) + noise_std * gauss); gauss: Box-Muller on two 24-bit draws of splitmix64(seed ^ stream, acting call, env).
// dbg (may be null) uint32 [N][4]: the two draws, the bits of the float32 gaussian, the bits of the float32 greedy action.
__device__ __forceinline__ void ddpg_act_body(const DdpgDev &L, int N, const float *__restrict__ obs, int obs_stride, const int *__restrict__ ticks, int noise,
                                              double *__restrict__ action, unsigned int *__restrict__ dbg, unsigned char *dg_smem) {
    const DdpgTile T = ddpg_tile(dg_smem, L.h1p, L.h2p);
    const int tid = threadIdx.x, e0 = blockIdx.x * AT_TM;
    const long long acts = L.cnt[DG_ACTS];
    const int row = tid >> 5, part = tid & 31, e = e0 + row;
    float v = 0.f;
    if (e < N) {
        if (part < L.n_obs) v = obs[(size_t)e * obs_stride + part];
        else if (part == L.n_obs) v = L.time_scale * (float)ticks[e];
    }
    T.X[row * AT_KIN + part] = v;
    __syncthreads();
    const int ob0 = dg_o_b0(L.h1p), ob1 = dg_o_b1(L.h1p, L.h2p), ow2 = dg_o_w2(L.h1p, L.h2p), ob2 = dg_o_b2(L.h1p, L.h2p);
    actor_layer(T.X, AT_KIN, AT_KIN, L.pi.p0, L.pi.w + ob0, T.H1, T.h1_ld, L.h1p);
    __syncthreads();
    actor_layer(T.H1, T.h1_ld, L.h1p, L.pi.p1, L.pi.w + ob1, T.H2, T.h2_ld, L.h2p);
    __syncthreads();
    const float z = ddpg_out_dot(T.H2, T.h2_ld, L.h2p, L.pi.w + ow2, L.pi.w[ob2]);
    if (part == 0 && e < N) {
        const float greedy = ddpg_tanh(z) * L.scale + L.mean;
        float a = greedy, g = 0.f;
        unsigned int u1 = 0, u2 = 0;
        if (noise) {
            g = dg_gauss(dg_hash(L.seed ^ DG_NOISE_STREAM, (unsigned long long)acts, (unsigned long long)e), u1, u2);
            a = greedy + L.noise_std * g;
        }
        a = a < L.a_low ? L.a_low : (a > L.a_high ? L.a_high : a);
        action[e] = (double)a;
        if (dbg) { dbg[4 * e] = u1; dbg[4 * e + 1] = u2; dbg[4 * e + 2] = __float_as_uint(g); dbg[4 * e + 3] = __float_as_uint(greedy); }
    }
    __syncthreads();
    if (noise && tid == 0 && dg_last_block(L.tick + DG_T_ACT, gridDim.x)) L.cnt[DG_ACTS] = acts + 1;
}
__global__ void __launch_bounds__(AT_THREADS) k_ddpg_act(DdpgDev L, int N, const float *__restrict__ obs, int obs_stride, const int *__restrict__ ticks, int noise,
                                                         double *__restrict__ action, unsigned int *__restrict__ dbg) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dg_smem[];
    ddpg_act_body(L, N, obs, obs_stride, ticks, noise, action, dbg, dg_smem);
}

}  // namespace stmpc

#include "stmpc_per_kernels.hpp"
#include "stmpc_nstep_kernels.hpp"
