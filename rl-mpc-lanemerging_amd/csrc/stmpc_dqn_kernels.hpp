// stmpc_dqn_kernels.hpp -- an on-device DQN learner for the discrete-action vector environments (sumo-jerk-v0, sumo-accel-v0): the reference's
// hand-written trainer (TRAIN_DQN: DQNAgent._train dqn.py:257-359, get_targets dqn.py:673-705, the DQN module dqn.py:566-658), restated.
// The Q-network has the one shape the reference trains: n_obs -> h1 -> ReLU -> A, float32 like the reference's module.
//
// The learner is built on the DDPG learner's parts and changes none of them.  Its struct EMBEDS a DdpgDev (`base`): the replay ring, the counters,
// the tickets, the minibatch workspace and prioritised replay's fields are that struct's, and the Q-network lives in base.q in the DDPG parameter
// layout with h2p := Ap (A padded to a multiple of 16): W0 [h1p][32] | b0 [h1p] | W1 [Ap][h1p] | b1 [Ap] (| an unused tail that stays zero).  That
// makes dg_hash sampling, k_replay_gather, ddpg_gate, ddpg_layer, ddpg_wgrad_body, ddpg_adam_step, ddpg_repack, ddpg_stats_body and the three
// stmpc_per_kernels.hpp kernels usable as they are.
//
// One update is three launches whose shapes depend on (B, h1, A) alone (five with prioritised replay: k_per_sample in front, k_per_update behind
// the weight gradients); every counter stays on the device:
//   k_dqn_fwd     one workgroup per 16 minibatch rows: gathers them; double DQN: a* = first argmax of the ONLINE net on s', Qt(s', a*) of the
//                 target net (plain DQN: max_a Qt(s', a)); g = gamma * that, clipped to [clip_min, clip_max] if asked; y = r + g (r alone on a terminated row);
//                 q = Q(s)[a], diff = q - y; SmoothL1 with beta 1, mean over B: dz = w * clamp(diff, -1, 1) / B.  dZout is one-hot, so
//                 dZ1[row][k] = H1 > 0 ? dz * W1[a][k] : 0 is a row gather.  Pad columns A <= j < Ap take part in neither argmax nor max (a pad Q
//                 of 0 would win wherever all real Q are negative).  The hidden layer is ddpg_layer, the output layer dqn_out_layer: the same MFMA
//                 loops without the ReLU.  X, H1, dZ1, dZout, dz go to the workspace
//   k_dqn_wgrad   ddpg_wgrad_body on the first four of its jobs (dW1 = dZout^T H1, dW0 = dZ1^T X, db1, db0): the grid ends before the scalar
//                 head's jobs.  The summation order is k_ddpg_wgrad's: no float atomics, no cross-workgroup partial sums
//   k_dqn_adam    Adam (ddpg_adam_step) + the hard copy of the target on every target_period-th update, decided from the device's update
//                 counter + the re-packing of both (ddpg_repack)
// Acting (k_dqn_act): Q(s) for N observations, greedy index = first maximum over the real A columns; with exploration one hash per (seed, acting
// call, env): its top 24 bits are u in [0, 1), and where u < eps the action is the hash's next 24 bits modulo A (do_dqn_control, dqn.py:661-670).
#pragma once
#include "stmpc_ddpg_kernels.hpp"

namespace stmpc {

constexpr int DQ_ACTION = 66;       // the replay row's action column (the index as float32: exact, A <= 256); DG_ROW's columns 66, 67 are free
constexpr unsigned long long DQN_STREAM = 0x64716E657870ull;        // the exploration draws' seed is seed ^ this ("dqnexp")

struct DqnDev {
    DdpgDev base;                   // ring, counters, tickets, workspace, tree; base.q: the Q-network; base.h2p = Ap, base.h2 = A; base.pi unused (null)
    int A, Ap, dbl, clip, target_period;
    float clip_min, clip_max;
};

// parameters that take part in Adam: everything in front of the DDPG layout's scalar head
__host__ __device__ inline int dq_nparam(int h1p, int Ap) { return dg_o_w2(h1p, Ap); }

// ---- replay: k_replay_push's row with an int32 action index in column DQ_ACTION and no time feature ---------------------------------------------
// (every kernel's body is a __device__ function of the learner's struct: the lone entry passes its by-value argument, the population entry of
// stmpc_dqn_pop_kernels.hpp the member blockIdx.y selects)
__device__ __forceinline__ void dqn_push_body(const DqnDev &D, int N, const float *__restrict__ obs, const float *__restrict__ next_obs, const float *__restrict__ final_obs,
                                              int obs_stride, const int *__restrict__ action, const double *__restrict__ reward,
                                              const unsigned char *__restrict__ term, const unsigned char *__restrict__ trunc) {
    const DdpgDev &L = D.base;
    const long long cursor = L.cnt[DG_CURSOR], fill = L.cnt[DG_FILL], frames = L.cnt[DG_FRAMES];
    const float done_v = L.n_step > 1 ? 1.f : 0.f;                  // (ddpg_push_body's)
    for (long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x; x < (long long)N * DG_ROW; x += (long long)gridDim.x * blockDim.x) {
        const int e = (int)(x / DG_ROW), c = (int)(x % DG_ROW);
        const bool done = term[e] || trunc[e];
        float v = 0.f;
        if (c < L.n_obs) v = obs[(size_t)e * obs_stride + c];
        else if (c >= 32 && c < 32 + L.n_obs) v = (done && final_obs ? final_obs : next_obs)[(size_t)e * obs_stride + (c - 32)];
        else if (c == DG_R) v = (float)reward[e];
        else if (c == DG_MASK) v = term[e] ? 0.f : 1.f;
        else if (c == DG_DONE) v = done ? done_v : 0.f;
        else if (c == DQ_ACTION) { const int a = action[e]; v = (float)(a < 0 ? 0 : (a >= D.A ? D.A - 1 : a)); }     // (the env latches an index out of range; the ring stays in range)
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
    if (last_s) per_push_tree(L, cursor, N);
}
__global__ void __launch_bounds__(256) k_dqn_push(DqnDev D, int N, const float *__restrict__ obs, const float *__restrict__ next_obs, const float *__restrict__ final_obs,
                                                  int obs_stride, const int *__restrict__ action, const double *__restrict__ reward,
                                                  const unsigned char *__restrict__ term, const unsigned char *__restrict__ trunc) {
    dqn_push_body(D, N, obs, next_obs, final_obs, obs_stride, action, reward, term, trunc);
}

// ---- pieces -------------------------------------------------------------------------------------------------------------------------------------
// the output layer, out[16][np] = in[16][kp] * W^T + bias: ddpg_layer<false>'s operands, lane order and summation order (16-wide k blocks summed on
// their own, the block sums added in k order in fp64, one rounding with the bias) without the ReLU
__device__ __forceinline__ void dqn_out_layer(const float *in, int in_ld, int kp, const float *packed, const float *bias, float *out, int out_ld, int np) {
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
        const double bv = (double)bias[n];
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(size_t)(kk * 4 + r) * out_ld + n] = (float)(acc[r] + bv);
    }
}

// Q[16][Ap] of one of the two networks (target: its packed copies and biases) on in[16][32]; H1 keeps the hidden activations.  Ends with a barrier
__device__ __forceinline__ void dqn_q(const DqnDev &D, const DdpgTile &T, const float *in, bool target) {
    const DdpgDev &L = D.base;
    const DdpgNet &n = L.q;
    const float *w = target ? n.wt : n.w;
    ddpg_layer<false>(in, AT_KIN, AT_KIN, target ? n.t0 : n.p0, w + dg_o_b0(L.h1p), T.H1, T.h1_ld, L.h1p);
    __syncthreads();
    dqn_out_layer(T.H1, T.h1_ld, L.h1p, target ? n.t1 : n.p1, w + dg_o_b1(L.h1p, D.Ap), T.H2, T.h2_ld, D.Ap);
    __syncthreads();
}

// the first maximum of q[0 ... A) as torch.argmax returns it, by the 32 lanes of a row; every lane of the row gets (index, value)
// (ties across strides: a lane keeps the first of its own columns part, part + 32, ... that holds its maximum, the merge the lower index of two equal values)
__device__ __forceinline__ int dqn_argmax(const float *q, int A, float &best) {
    const int part = threadIdx.x & 31;
    float bv = -INFINITY; int bi = A;                               // (bi = A: a lane without a column, which never wins)
    for (int j = part; j < A; j += 32) { const float v = q[j]; if (bi == A || v > bv) { bv = v; bi = j; } }
    for (int o = 1; o < 32; o <<= 1) {
        const float ov = __shfl_xor(bv, o); const int oi = __shfl_xor(bi, o);
        if (oi < A && (bi >= A || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
    }
    best = bv;
    return bi < A ? bi : 0;
}

// ---- forward / backward -------------------------------------------------------------------------------------------------------------------------
// dbg (may be null) float32 [B][4]: a* (plain DQN: the maximum's index), the target net's Q there, y, Q(s, a)
// (NS: the n-step instance, as ddpg_critic_fwd_pass's)
template <bool NS>
__device__ __forceinline__ void dqn_fwd_pass(const DqnDev &D, int B, int gate, float *__restrict__ dbg, unsigned char *dg_smem) {
    const DdpgDev &L = D.base;
    if (!ddpg_gate(L, gate)) return;
    const DdpgTile T = ddpg_tile(dg_smem, L.h1p, D.Ap);
    const int tid = threadIdx.x, r0 = blockIdx.x * AT_TM, row = tid >> 5, part = tid & 31;
    const bool valid = r0 + row < B;
    const long long fill = L.cnt[DG_FILL], upd = L.cnt[DG_UPDATES];
    int act = 0;
    {   // gather: X = s, Xn = s' (columns >= n_obs are zero in the ring), sc = (reward, mask)
        const long long idx = valid ? dg_row_index(L, upd, fill, r0 + row) : 0;
        const float *src = L.ring + (size_t)idx * DG_ROW;
        if (NS) nstep_gather_tile(L, T.X, T.Xn, T.sc, idx, valid);      // s' and the mask of the window's last row, sc = (R, mask, gamma^m)
        else {
            T.X[row * AT_KIN + part] = valid ? src[part] : 0.f;
            T.Xn[row * AT_KIN + part] = valid ? src[32 + part] : 0.f;
            if (part < 2) T.sc[row * 4 + part] = valid ? src[DG_R + part] : 0.f;
        }
        act = valid ? (int)src[DQ_ACTION] : 0;
    }
    __syncthreads();
    int astar = 0;
    float qsel;
    if (D.dbl) {                                                    // a* from the online net on s'
        dqn_q(D, T, T.Xn, false);
        astar = dqn_argmax(T.H2 + (size_t)row * T.h2_ld, D.A, qsel);
        __syncthreads();
    }
    dqn_q(D, T, T.Xn, true);
    if (D.dbl) qsel = T.H2[(size_t)row * T.h2_ld + astar];
    else astar = dqn_argmax(T.H2 + (size_t)row * T.h2_ld, D.A, qsel);
    float g = ddpg_discount<NS>(L, T) * qsel;
    if (D.clip) g = g < D.clip_min ? D.clip_min : (g > D.clip_max ? D.clip_max : g);
    const float y = T.sc[row * 4 + 1] != 0.f ? T.sc[row * 4 + 0] + g : T.sc[row * 4 + 0];      // a terminated row is its reward alone (next_state is None), whatever g is
    __syncthreads();
    // Q(s), q = Q(s)[a]
    dqn_q(D, T, T.X, false);
    const float qv = T.H2[(size_t)row * T.h2_ld + act];
    const float diff = qv - y;
    const float cl = diff < -1.0f ? -1.0f : (diff > 1.0f ? 1.0f : diff);
    // d mean(smooth_l1(Q - y)) / dQ; prioritised replay: the row's term carries its importance weight
    const float dz = valid ? (L.aw ? (L.aw[r0 + row] * cl) / (float)B : cl / (float)B) : 0.f;
    if (part == 0) {
        const float ad = fabsf(diff);
        if (L.atd) L.atd[r0 + row] = valid ? diff : 0.f;
        L.adz[r0 + row] = dz;
        L.arow[2 * (r0 + row)] = valid ? (ad < 1.0f ? 0.5f * diff * diff : ad - 0.5f) : 0.f;
        L.arow[2 * (r0 + row) + 1] = valid ? qv : 0.f;
        if (dbg && valid) { float *o = dbg + 4 * (size_t)(r0 + row); o[0] = (float)astar; o[1] = qsel; o[2] = y; o[3] = qv; }
    }
    ddpg_store_tile(T.X, AT_KIN, L.aX + (size_t)r0 * AT_KIN, AT_KIN);
    ddpg_store_tile(T.H1, T.h1_ld, L.aH1 + (size_t)r0 * L.h1p, L.h1p);
    // dZout [16][Ap]: dz in the action's column; dZ1 = dz * W1[a] where H1 > 0
    for (int j = part; j < D.Ap; j += 32) L.aD2[(size_t)(r0 + row) * D.Ap + j] = j == act ? dz : 0.f;
    const float *w1a = L.q.w + dg_o_w1(L.h1p) + (size_t)act * L.h1p;
    for (int k = part; k < L.h1p; k += 32)
        L.aD1[(size_t)(r0 + row) * L.h1p + k] = T.H1[(size_t)row * T.h1_ld + k] > 0.f ? dz * w1a[k] : 0.f;
}
__device__ __forceinline__ void dqn_fwd_body(const DqnDev &D, int B, int gate, float *__restrict__ dbg, unsigned char *dg_smem) {
    if (D.base.n_step > 1) dqn_fwd_pass<true>(D, B, gate, dbg, dg_smem);
    else dqn_fwd_pass<false>(D, B, gate, dbg, dg_smem);
}
__global__ void __launch_bounds__(AT_THREADS) k_dqn_fwd(DqnDev D, int B, int gate, float *__restrict__ dbg) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dg_smem[];
    dqn_fwd_body(D, B, gate, dbg, dg_smem);
}

// ---- weight gradients: k_ddpg_wgrad's body; the grid covers its jobs dW1, dW0, db1, db0 and stops in front of the scalar head's ------------------
__global__ void __launch_bounds__(64 * DG_WG_WAVES) k_dqn_wgrad(DqnDev D, int Bp, int gate) {
    __shared__ double part_s[DG_WG_WAVES][256];
    ddpg_wgrad_body(D.base, 1, Bp, gate, part_s);
}

// ---- Adam + target sync + re-pack ---------------------------------------------------------------------------------------------------------------
// mode 0: Adam step, the hard copy of the target if this update's number is a multiple of target_period, re-pack; mode 1: re-pack only
__device__ __forceinline__ void dqn_adam_body(const DqnDev &D, float lr, int mode, int gate) {
    const DdpgDev &L = D.base;
    if (mode == 0 && !ddpg_gate(L, gate)) return;
    const DdpgNet &net = L.q;
    const int np = dq_nparam(L.h1p, D.Ap);
    const float pw1 = net.bpow[0] * L.beta1, pw2 = net.bpow[1] * L.beta2;
    const long long upd = L.cnt[DG_UPDATES];
    const bool sync = (upd + 1) % D.target_period == 0;
    const float step = lr / (1.0f - pw1), bc2s = sqrtf(1.0f - pw2);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < np; i += gridDim.x * blockDim.x) {
        float w = net.w[i], wt = net.wt[i];
        if (mode == 0) {
            w = ddpg_adam_step(L, net, i, w, step, bc2s);
            net.w[i] = w;
            if (sync) { wt = w; net.wt[i] = wt; }
        }
        ddpg_repack(L, net, i, w, wt);
    }
    __syncthreads();
    if (mode == 0 && threadIdx.x == 0 && dg_last_block(L.tick + DG_T_ADAM + 1, gridDim.x)) {
        net.bpow[0] = pw1; net.bpow[1] = pw2;
        L.cnt[DG_UPDATES] = upd + 1;
    }
}
__global__ void __launch_bounds__(256) k_dqn_adam(DqnDev D, float lr, int mode, int gate) { dqn_adam_body(D, lr, mode, gate); }

// padded parameter layout -> W0 [h1][n_obs] | b0 [h1] | W1 [A][h1] | b1 [A], row-major, unpadded
__global__ void k_dqn_unpad(DqnDev D, const float *__restrict__ src, float *__restrict__ dst) {
    const DdpgDev &L = D.base;
    const int n0 = L.h1 * L.n_obs, n1 = n0 + L.h1, n2 = n1 + D.A * L.h1, total = n2 + D.A;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        int s;
        if (i < n0) s = (i / L.n_obs) * AT_KIN + i % L.n_obs;
        else if (i < n1) s = dg_o_b0(L.h1p) + (i - n0);
        else if (i < n2) s = dg_o_w1(L.h1p) + ((i - n1) / L.h1) * L.h1p + (i - n1) % L.h1;
        else s = dg_o_b1(L.h1p, D.Ap) + (i - n2);
        dst[i] = src[s];
    }
}

__global__ void __launch_bounds__(64) k_dqn_stats(DqnDev D, int B, double *out) { ddpg_stats_body(D.base, B, out); }

// ---- acting -------------------------------------------------------------------------------------------------------------------------------------
// action [N] int32: the greedy index, or -- explore != 0 and the row's u < eps -- the second draw modulo A.  dbg_q (may be null) float32 [N][A]
__device__ __forceinline__ void dqn_act_body(const DqnDev &D, int N, const float *__restrict__ obs, int obs_stride, float eps, int explore,
                                             int *__restrict__ action, float *__restrict__ dbg_q, unsigned char *dg_smem) {
    const DdpgDev &L = D.base;
    const DdpgTile T = ddpg_tile(dg_smem, L.h1p, D.Ap);
    const int tid = threadIdx.x, e0 = blockIdx.x * AT_TM, row = tid >> 5, part = tid & 31, e = e0 + row;
    const long long acts = L.cnt[DG_ACTS];
    T.X[row * AT_KIN + part] = e < N && part < L.n_obs ? obs[(size_t)e * obs_stride + part] : 0.f;
    __syncthreads();
    dqn_q(D, T, T.X, false);
    float qbest;
    int a = dqn_argmax(T.H2 + (size_t)row * T.h2_ld, D.A, qbest);
    if (e < N) {
        if (dbg_q) for (int j = part; j < D.A; j += 32) dbg_q[(size_t)e * D.A + j] = T.H2[(size_t)row * T.h2_ld + j];
        if (part == 0) {
            if (explore) {
                const unsigned long long h = dg_hash(L.seed ^ DQN_STREAM, (unsigned long long)acts, (unsigned long long)e);
                const float u = (float)(unsigned int)(h >> 40) * 5.9604644775390625e-8f;      // [0, 1): a multiple of 2^-24, exact in float32
                if (u < eps) a = (int)((unsigned int)((h >> 16) & 0xFFFFFFull) % (unsigned int)D.A);
            }
            action[e] = a;
        }
    }
    __syncthreads();
    if (explore && tid == 0 && dg_last_block(L.tick + DG_T_ACT, gridDim.x)) L.cnt[DG_ACTS] = acts + 1;
}
__global__ void __launch_bounds__(AT_THREADS) k_dqn_act(DqnDev D, int N, const float *__restrict__ obs, int obs_stride, float eps, int explore,
                                                        int *__restrict__ action, float *__restrict__ dbg_q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dg_smem[];
    dqn_act_body(D, N, obs, obs_stride, eps, explore, action, dbg_q, dg_smem);
}

}  // namespace stmpc
