// stmpc_per_kernels.hpp -- prioritised replay for the DDPG / TD3 learner's ring: the reference's hand-written trainer samples from a sum tree
// (dqn.py:267-349, SumTree dqn.py:727-794; USE_PRIORITIZED_ER = True, PER_ALPHA 0.5, PER_MIN_PRIORITY 1e-6, PER_MAX_PRIORITY 4.0), restated.
//
// The tree has the reference's layout: L = capacity rounded up to a power of two, 2L - 1 fp64 nodes, root 0, children of i at 2i + 1 and 2i + 2, ring
// position p at leaf p + L - 1, unfilled leaves 0.  An internal node is always RECOMPUTED as left + right (the reference's _update_sum), never adjusted
// by a difference and never built with atomics: its value does not depend on the order of the writes below it, so a tree is reproducible bit for bit.
//   per_push_tree   the tree part of a push, in the last workgroup of k_replay_push: the N new leaves get max_priority ^ alpha, their ancestors are
//                   recomputed level by level (a contiguous range per level, two when the ring wraps), a barrier between levels
//   k_per_sample    one workgroup: B descents (per_sample_index, the function the C host twin calls too) into idx[Bp], and the importance weights
//                   (fill * p / total) ^ -beta over the minibatch's largest, fp64 -> float32, into aw[Bp]; beta = 0 writes 1.0f
//   k_per_update    one workgroup, after the critic pass: leaf[idx_r] = min(|td_r| + min_priority, max_priority) ^ alpha with the float32 td = Q - y the
//                   critic pass left in atd (TD3: the larger of both critics' |td|); of rows with the same index the highest wins (the reference's
//                   loop order; B^2 / 2 comparisons in LDS); then the B paths' ancestors level by level
// A descent is about log2(L) dependent fp64 loads; these kernels are latency chains, not throughput kernels.  Both are gated like the update.
// Each kernel's text is a __device__ body taking the learner's struct by reference (per_sample_body, per_update_body); the __global__ entries here pass
// their by-value argument, the populations' entries (stmpc_per_pop_kernels.hpp) a row of a device table.
// The gathers of the update read idx[] instead of hashing (DdpgDev::idx != null), because the priorities change between the critic and the actor pass.
#pragma once
#include "stmpc_ddpg_kernels.hpp"

namespace stmpc {

constexpr unsigned long long PER_STREAM = 0x70657264726177ull;      // the rolls' seed is seed ^ this ("perdraw")
constexpr int PER_REDRAWS = 3;
constexpr int PER_THREADS = 256;

__host__ __device__ inline double per_pow(double p, double alpha) { return alpha == 0.5 ? sqrt(p) : (alpha == 1.0 ? p : pow(p, alpha)); }
// the weight of a row whose critic error was td
__host__ __device__ inline double per_priority(float td, double min_priority, double max_priority, double alpha) {
    const double e = fabs((double)td) + min_priority;
    return per_pow(e < max_priority ? e : max_priority, alpha);
}

// Ring position of minibatch row `row` of update `upd`: roll = uniform01(hash) * tree[0] (53 bits), descent as the reference's _traverse_tree
// (roll <= left: left; else roll -= left, right).  A leaf at or past `fill` or of weight 0 (reachable through rounding only) is redrawn with the
// attempt number in the hash's upper row bits, PER_REDRAWS times; after that the row falls back to the uniform index of stmpc_ddpg_sample_index.
__host__ __device__ inline long long per_sample_index(const double *tree, long long leaves, long long fill, unsigned long long seed, unsigned long long upd,
                                                      unsigned int row) {
    if (fill < 1) return 0;
    const double total = tree[0];
    for (unsigned long long a = 0; a <= (unsigned long long)PER_REDRAWS; ++a) {
        const unsigned long long h = dg_hash(seed ^ PER_STREAM, upd, (unsigned long long)row | (a << 32));
        double roll = ((double)(h >> 11) * 0x1.0p-53) * total;
        long long i = 0;
        while (i < leaves - 1) {
            const long long left = 2 * i + 1;
            const double wl = tree[left];
            if (roll <= wl) i = left;
            else { roll -= wl; i = left + 1; }
        }
        const long long p = i - (leaves - 1);
        if (p < fill && tree[i] > 0.0) return p;
    }
    return (long long)(dg_hash(seed, upd, (unsigned long long)row) % (unsigned long long)fill);
}

// (declared in stmpc_ddpg_kernels.hpp; every thread of ONE workgroup calls it) ring rows cursor ... cursor + N - 1 (mod capacity) were just written
__device__ __forceinline__ void per_push_tree(const DdpgDev &L, long long cursor, int N) {
    double *tree = L.tree;
    const long long C = L.capacity, nl = L.per_L;
    const double w = per_pow(L.per_max, L.per_alpha);
    // inclusive leaf ranges: up to the ring's end, and the wrapped rest (empty: hi < lo, and stays so under >> 1)
    long long lo[2] = {cursor, 0}, hi[2] = {(cursor + N < C ? cursor + N : C) - 1, cursor + N - C - 1};
    for (int k = 0; k < 2; ++k)
        for (long long p = lo[k] + threadIdx.x; p <= hi[k]; p += blockDim.x) tree[nl - 1 + p] = w;
    for (long long width = nl >> 1; width >= 1; width >>= 1) {       // the level of `width` nodes begins at index width - 1
        __syncthreads();
        for (int k = 0; k < 2; ++k) {
            lo[k] >>= 1; hi[k] >>= 1;
            for (long long q = lo[k] + threadIdx.x; q <= hi[k]; q += blockDim.x) {
                const long long i = width - 1 + q;
                tree[i] = tree[2 * i + 1] + tree[2 * i + 2];
            }
        }
    }
}

// (every thread of ONE workgroup calls it; red: PER_THREADS doubles of LDS.  The returns are workgroup-uniform -- the gate reads the learner's counters,
// beta is a constant of the learner -- and the first of them precedes the first barrier)
__device__ __forceinline__ void per_sample_body(const DdpgDev &L, int B, int Bp, int gate, double *red) {
    if (!ddpg_gate(L, gate)) return;
    const int tid = threadIdx.x;
    const long long fill = L.cnt[DG_FILL], upd = L.cnt[DG_UPDATES], nl = L.per_L;
    const double *tree = L.tree;
    double pmin = INFINITY;                                         // the smallest sampled weight has the largest importance weight
    for (int r = tid; r < Bp; r += PER_THREADS) {
        long long p = 0;
        if (r < B) {
            p = per_sample_index(tree, nl, fill, L.seed, (unsigned long long)upd, (unsigned int)r);
            const double w = tree[nl - 1 + p];
            if (w > 0.0 && w < pmin) pmin = w;
        }
        L.idx[r] = p;
    }
    if (L.per_beta == 0.0) {
        for (int r = tid; r < Bp; r += PER_THREADS) L.aw[r] = r < B ? 1.0f : 0.f;
        return;
    }
    red[tid] = pmin;
    __syncthreads();
    for (int o = PER_THREADS >> 1; o > 0; o >>= 1) {
        if (tid < o && red[tid + o] < red[tid]) red[tid] = red[tid + o];
        __syncthreads();
    }
    const double total = tree[0], scale = (double)fill, wmax = pow(scale * red[0] / total, -L.per_beta);
    for (int r = tid; r < Bp; r += PER_THREADS) {                   // (idx[r] is this thread's own store)
        float w = 0.f;
        if (r < B) {
            const double p = tree[nl - 1 + L.idx[r]];
            w = p > 0.0 ? (float)(pow(scale * p / total, -L.per_beta) / wmax) : 1.0f;
        }
        L.aw[r] = w;
    }
}
__global__ void __launch_bounds__(PER_THREADS) k_per_sample(DdpgDev L, int B, int Bp, int gate) {
    __shared__ double red[PER_THREADS];
    per_sample_body(L, B, Bp, gate, red);
}

// the td of row r that sets its priority: view 0's, or critic 2's where that is larger in magnitude (atd2 null: DDPG)
__device__ __forceinline__ float per_td(const DdpgDev &L, const float *atd2, int r) {
    const float t1 = L.atd[r];
    if (!atd2) return t1;
    const float t2 = atd2[r];
    return fabsf(t2) > fabsf(t1) ? t2 : t1;
}

constexpr int PER_MAX_B = 8192;     // stmpc_ddpg_create's largest batch

// (every thread of ONE workgroup calls it; idx_s: PER_MAX_B ints of LDS; atd2: critic 2's Q - y, null for DDPG.  The return is workgroup-uniform and
// precedes the first barrier)
__device__ __forceinline__ void per_update_body(const DdpgDev &L, const float *atd2, int B, int gate, int *idx_s) {
    if (!ddpg_gate(L, gate)) return;
    const int tid = threadIdx.x;
    double *tree = L.tree;
    const long long nl = L.per_L;
    for (int r = tid; r < B; r += PER_THREADS) idx_s[r] = (int)L.idx[r];
    __syncthreads();
    for (int r = tid; r < B; r += PER_THREADS) {
        const int p = idx_s[r];
        bool wins = true;
        for (int r2 = r + 1; r2 < B; ++r2)
            if (idx_s[r2] == p) { wins = false; break; }
        if (wins) tree[nl - 1 + p] = per_priority(per_td(L, atd2, r), L.per_min, L.per_max, L.per_alpha);
    }
    int shift = 1;
    for (long long width = nl >> 1; width >= 1; width >>= 1, ++shift) {
        __syncthreads();
        for (int r = tid; r < B; r += PER_THREADS) {                // (rows that share an ancestor store the same sum)
            const long long i = width - 1 + (idx_s[r] >> shift);
            tree[i] = tree[2 * i + 1] + tree[2 * i + 2];
        }
    }
}
__global__ void __launch_bounds__(PER_THREADS) k_per_update(DdpgDev L, const float *atd2, int B, int gate) {
    __shared__ int idx_s[PER_MAX_B];
    per_update_body(L, atd2, B, gate, idx_s);
}

// what the last sampling step and critic pass left: idx int64 [B], td float32 [B] (per_td), weight float32 [B]
__global__ void k_per_last(DdpgDev L, const float *atd2, int B, long long *idx, float *td, float *weight) {
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < B; r += gridDim.x * blockDim.x) {
        idx[r] = L.idx[r]; td[r] = per_td(L, atd2, r); weight[r] = L.aw[r];
    }
}

}  // namespace stmpc
