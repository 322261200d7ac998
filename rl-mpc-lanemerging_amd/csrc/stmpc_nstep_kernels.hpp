// stmpc_nstep_kernels.hpp -- multi-step (n-step) returns for the learners' replay, formed at sampling time from the ring itself: the uncorrected
// n-step return of Rainbow (Hessel et al. 2018, section "Multi-step learning") and D4PG (Barth-Maron et al. 2018, eq. 5).
//
// A push writes the N rows of one env step at cursor + e, so the transition that follows ring row i in the same env is row (i + N) % capacity,
// whatever the capacity, as long as every push has N rows (the host refuses another N on a learner with n_step > 1).  With
//   age(i) = (cursor - 1 - i) mod capacity (0: the newest row),  row_k = (i + k N) % capacity,  row_k exists iff age(i) >= k N
// (a row newer than i cannot have been overwritten while i is live), the window of row i has length m = the smallest k + 1, k = 0 .. n - 1, at which
// row_k is done (terminated or truncated: column DG_DONE), k + 1 == n, or row_{k+1} does not exist (the window ran into the ring's newest rows: a
// shorter return, not a refusal).  R = sum_{k<m} gamma^k r(row_k), disc = gamma^m; s' and the mask come from row_{m-1} (a truncated row bootstraps
// from its stored final observation with mask 1, a terminated one has mask 0, as in the one-step target).
//
// Arithmetic, fixed so that learner.nstep_window_host restates it bit for bit: gamma^k is the running fp64 product 1 * g * g ... of g =
// (double)(float)gamma, the terms gamma^k * (double)r_k are added in k order, every operation explicitly unfused (__dmul_rn, __dadd_rn), and R and
// disc are rounded to float32 once.  At m = 1 that is R == r and disc == gamma exactly.
//
// The window is found by the 32 lanes that own a minibatch row in the fused forward kernels (threadIdx.x >> 5 is the row): lane k loads reward
// and done flag of row_k -- all k addresses follow from i, so the loads of a workgroup's 16 rows are issued together and none depends on another --,
// a ballot over the row's lanes gives m, and the sum runs over shuffles in k order.
#pragma once
#include "stmpc_ddpg_kernels.hpp"

namespace stmpc {

// by ALL lanes of a wave, the 32 lanes of a half (threadIdx.x & 32) with the same ring row i; every lane gets the window
__device__ __forceinline__ NstepWin nstep_window(const DdpgDev &L, long long i, long long cursor) {
    const int k = threadIdx.x & 31, base = threadIdx.x & 32, n = L.n_step > 1 ? L.n_step : 1;      // (0 on a learner that was never enabled: one step)
    const long long cap = L.capacity, N = L.rows_push;
    long long age = (cursor - 1 - i) % cap;
    if (age < 0) age += cap;
    const bool live = k < n && age >= k * N;
    float r = 0.f, dn = 0.f;
    if (live) {
        const float *src = L.ring + (size_t)((i + k * N) % cap) * DG_ROW;
        r = src[DG_R]; dn = src[DG_DONE];
    }
    const bool stop = live && (dn != 0.f || k + 1 == n || age < (k + 1) * N);
    const unsigned int bits = (unsigned int)(__ballot(stop) >> base);      // this row's lanes
    const int m = bits ? __ffs(bits) : 1;                           // (k = 0 is always live, and the first k that is not followed stops)
    const double g = (double)L.gamma;
    double gk = 1.0;
    for (int j = 0; j < k && j < n; ++j) gk = __dmul_rn(gk, g);
    const double term = __dmul_rn(gk, (double)r), gk1 = __dmul_rn(gk, g);
    double R = __shfl(term, base);
    for (int j = 1; j < n; ++j) {                                   // k order; n is the wave's, m the row's
        const double t = __shfl(term, base + j);
        if (j < m) R = __dadd_rn(R, t);
    }
    NstepWin w;
    w.R = (float)R; w.disc = (float)__shfl(gk1, base + m - 1); w.last = (i + (long long)(m - 1) * N) % cap; w.m = m;
    return w;
}

// the fused forwards' gather of a learner with n_step > 1 (ddpg_gather_tile, dqn_fwd_body), 32 lanes per minibatch row: X = row idx's [0, 32),
// Xn = [32, 64) of its window's last row, sc = (R, that row's mask, gamma^m).  A body of its own, so that the one-step gather keeps its text
__device__ __forceinline__ void nstep_gather_tile(const DdpgDev &L, float *X, float *Xn, float *sc, long long idx, bool valid) {
    const int row = threadIdx.x >> 5, c = threadIdx.x & 31;
    const NstepWin w = nstep_window(L, idx, L.cnt[DG_CURSOR]);
    const float *src = L.ring + (size_t)idx * DG_ROW, *nx = L.ring + (size_t)w.last * DG_ROW;
    X[row * AT_KIN + c] = valid ? src[c] : 0.f;
    Xn[row * AT_KIN + c] = valid ? nx[32 + c] : 0.f;
    if (c == 0) { sc[row * 4 + 0] = valid ? w.R : 0.f; sc[row * 4 + 1] = valid ? nx[DG_MASK] : 0.f; sc[row * 4 + 2] = w.disc; }
}

// the minibatch of the current update index as the n-step target sees it: out [B][DG_ROW] = row i with [32, 64) (s') and the mask of the window's last
// row and R in the reward's place.  Two minibatch rows per wave
__device__ __forceinline__ void nstep_gather_body(const DdpgDev &L, int B, float *out, long long fill, long long upd) {
    const int lane = threadIdx.x & 63, c0 = lane & 31;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    const long long cursor = L.cnt[DG_CURSOR];
    for (int r0 = 2 * wave; r0 < B; r0 += 2 * nwaves) {
        const int r = r0 + (lane >> 5);
        const bool valid = r < B;
        const long long idx = valid ? dg_row_index(L, upd, fill, r) : 0;
        const NstepWin w = nstep_window(L, idx, cursor);
        if (!valid) continue;
        const float *src = L.ring + (size_t)idx * DG_ROW, *nx = L.ring + (size_t)w.last * DG_ROW;
        for (int c = c0; c < DG_ROW; c += 32)
            out[(size_t)r * DG_ROW + c] = c == DG_R ? w.R : ((c >= 32 && c < 64) || c == DG_MASK ? nx[c] : src[c]);
    }
}

// diagnostics: the windows of n_idx arbitrary ring rows, out [n_idx][4] fp64 = R, disc, the last row's index, m
__global__ void __launch_bounds__(256) k_nstep_window(DdpgDev L, const long long *__restrict__ idx, int n_idx, double *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    const long long cursor = L.cnt[DG_CURSOR];
    for (int r0 = 2 * wave; r0 < n_idx; r0 += 2 * nwaves) {
        const int r = r0 + (lane >> 5);
        const bool valid = r < n_idx;
        const NstepWin w = nstep_window(L, valid ? idx[r] : 0, cursor);
        if (valid && (lane & 31) == 0) {
            double *o = out + 4 * (size_t)r;
            o[0] = (double)w.R; o[1] = (double)w.disc; o[2] = (double)w.last; o[3] = (double)w.m;
        }
    }
}

}  // namespace stmpc
