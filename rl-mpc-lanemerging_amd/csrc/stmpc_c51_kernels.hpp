// stmpc_c51_kernels.hpp -- an on-device categorical (C51) DQN learner for the discrete-action vector environments: the distributional head of the
// reference's third agent (rainbow.py: the `all` library's rainbow preset), after Bellemare, Dabney and Munos 2017, "A Distributional Perspective on
// Reinforcement Learning", Algorithm 1.  The network n_obs -> h1 -> ReLU -> A * K emits, for every action a, K logits in the contiguous columns
// a K ... a K + K - 1; their softmax is a distribution over the fixed support z_k = v_min + k dz, dz = (v_max - v_min) / (K - 1), and Q(s, a) is its mean.
//
// The learner is built on the DQN learner's parts and changes none of them.  Its struct EMBEDS a DqnDev (`dq`, and through it the DdpgDev with the
// ring, counters, tickets, workspace and sum tree); the network lives in dq.base.q in the DDPG parameter layout with h2p := Ap = A * K padded to a
// multiple of 16.  dqn_push_body, ddpg_layer, dqn_out_layer (through dqn_q), ddpg_wgrad_body, dqn_adam_body, ddpg_gate, nstep_gather_tile,
// ddpg_discount, the three k_per_* kernels and ddpg_stats_body are used as they are.
//
// One update is three launches (five with prioritised replay):
//   k_c51_fwd     one workgroup per 16 minibatch rows, 32 lanes per row: gathers them; a* = the first maximum over the REAL actions of the expected
//                 values of the online net (double) or the target net on s' (pad columns belong to no action); p' = softmax of the TARGET net's block
//                 a*; m = the projection of the shifted support R + disc z_j onto the support (c51_project_row); log-softmax of the online net's
//                 block a (the stored action) on s; row loss l = -sum_i m_i log p_i; dZout[a K + i] = (w / B)(p_i - m_i), every other column an exact
//                 zero; dZ1 = dZout W1 where H1 > 0, a sum over the K rows of the action's block in i order.  atd = l (the priority), arow = (l, Q(s, a))
//   k_c51_wgrad   ddpg_wgrad_body on its first four jobs, as k_dqn_wgrad; dZout is dense here, which the body handles for DDPG
//   k_c51_adam    dqn_adam_body
// Arithmetic of the softmax: the float32 logits go to fp64, the maximum is subtracted, exp and log are the accurate fp64 functions, the sums over k
// run lane-strided with a butterfly behind them (a fixed order), and every result is rounded to float32 once.  The projection accumulates in fp64 in
// j order: no float atomics, no scatter adds.  It is the gather form: it stays right where b_j is an integer, where the textbook l / u scatter
// loses the mass.
//
// The dueling head (C51Dev::dueling; Wang et al. 2016, "Dueling Network Architectures for Deep Reinforcement Learning", in the categorical form of
// Hessel et al. 2018, "Rainbow", section "Dueling networks"; a restatement of the published head: parity with the `all` library's own is not pinned,
// the library is absent).  The network is n_obs -> h1 -> ReLU -> (A + 1) * K: the A advantage blocks sit where the action blocks sit, columns a K ...
// a K + K - 1, the value block comes last, columns A K ... A K + K - 1, and Ap = pad16((A + 1) K).  The logits of action a are
//   l[a][k] = V[k] + Adv[a][k] - (1 / A) sum_b Adv[b][k]
// formed by c51_dueling_combine behind every dqn_q, in place over the advantage blocks; from there on the first A blocks of a row are ordinary C51
// logits and everything above holds as it stands.  Backward, with g[k] = (w / B)(p[k] - m[k]) of the stored action a: dZout is dense -- advantage
// block b gets g[k] ((b == a) - 1 / A), the value block g[k], pad columns and the rows at or beyond B exact zeros -- and dZ1 sums over all (A + 1) K
// rows of W1 in row order.  In the acting and evaluation kernels the head is a branch on D.dueling, uniform across the grid; the forward / backward pass
// takes it as a template argument and has a kernel per head (k_c51_fwd, k_c51_fwd_duel), because with both heads in one kernel the plain head's pass
// lost its register budget.  With dueling == 0 every kernel computes what it computed without it.
#pragma once
#include "stmpc_dqn_kernels.hpp"

namespace stmpc {

struct C51Dev {
    DqnDev dq;                      // dq.A: the real actions; dq.Ap = pad16(A * K) = dq.base.h2p; dq.base.h2 = A * K; dq.clip unused (0)
    int K;                          // atoms
    int dueling;                    // 1: the dueling head -- dq.base.h2 = (A + 1) K, dq.Ap = pad16 of it, the value block behind the A advantage blocks
    double v_min, v_max, dz;        // the support, in fp64: dz = (v_max - v_min) / (K - 1) is no float32 number at the shipped K = 51
};

// LDS: DdpgTile's, then m [16][K]
__host__ inline size_t c51_tile_bytes(int h1p, int Ap, int K) { return ddpg_tile_bytes(h1p, Ap) + (size_t)AT_TM * K * sizeof(float); }
__device__ __forceinline__ float *c51_m_tile(const DdpgTile &T) { return T.H2 + (size_t)AT_TM * T.h2_ld; }

// sum of a double over the 32 lanes of a row; every lane gets it (xor butterfly: a fixed order)
__device__ __forceinline__ double c51_row_sum(double s) {
    s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4); s += __shfl_xor(s, 8); s += __shfl_xor(s, 16);
    return s;
}
// the softmax's two statistics of x[0 ... K) by the 32 lanes of a row: mx = the maximum, se = sum_k exp(x_k - mx); every lane gets both
__device__ __forceinline__ void c51_block_stats(const float *x, int K, double &mx, double &se) {
    const int part = threadIdx.x & 31;
    float m = -INFINITY;
    for (int k = part; k < K; k += 32) m = fmaxf(m, x[k]);
    for (int o = 1; o < 32; o <<= 1) m = fmaxf(m, __shfl_xor(m, o));
    mx = (double)m;
    double s = 0.0;
    for (int k = part; k < K; k += 32) s += exp((double)x[k] - mx);
    se = c51_row_sum(s);
}
// the mean of softmax(x[0 ... K)) over the support, in fp64, in every lane of the row
__device__ __forceinline__ double c51_block_mean(const C51Dev &D, const float *x) {
    const int part = threadIdx.x & 31;
    double mx, se;
    c51_block_stats(x, D.K, mx, se);
    double s = 0.0;
    for (int k = part; k < D.K; k += 32) s += (D.v_min + (double)k * D.dz) * exp((double)x[k] - mx);
    return c51_row_sum(s) / se;
}
// expected values of the A real actions from a row of logits q[Ap]: the first maximum's index as torch.argmax returns it (the values compared are
// the float32 ones a caller sees), `best` its value; dbg_q (may be null): the A values of this row.  By the 32 lanes of a row; every lane gets both
__device__ __forceinline__ int c51_greedy(const C51Dev &D, const float *q, float &best, float *dbg_q) {
    int bi = 0;
    float bv = 0.f;
    for (int a = 0; a < D.dq.A; ++a) {
        const float v = (float)c51_block_mean(D, q + (size_t)a * D.K);
        if (a == 0 || v > bv) { bv = v; bi = a; }
        if (dbg_q && (threadIdx.x & 31) == 0) dbg_q[a] = v;
    }
    best = bv;
    return bi;
}

// The dueling head's combine of one row of outputs q[(A + 1) K], in place, by the row's 32 lanes: l[a][k] = (V[k] + Adv[a][k]) - (sum_b Adv[b][k]) / A.
// The float32 outputs go to fp64, the sum runs in b order, the division and the two additions are fp64, and the result is rounded to float32 once and
// stored over Adv[a][k].  A lane owns the columns k = part, part + 32, ... of its row in every block: no lane reads what another writes.  The value
// block stays.  Ends with a barrier (every thread of the workgroup calls it: the branch that leads here is uniform)
__device__ __forceinline__ void c51_dueling_combine(const C51Dev &D, float *q) {
    const int part = threadIdx.x & 31, A = D.dq.A, K = D.K;
    const float *v = q + (size_t)A * K;
    for (int k = part; k < K; k += 32) {
        double s = 0.0;
        for (int b = 0; b < A; ++b) s += (double)q[(size_t)b * K + k];
        const double mean = s / (double)A, vk = (double)v[k];
        for (int a = 0; a < A; ++a) q[(size_t)a * K + k] = (float)((vk + (double)q[(size_t)a * K + k]) - mean);
    }
    __syncthreads();
}

// The categorical projection of one row, by its 32 lanes (all 64 lanes of the wave call it): the atoms z_j move to t_j = clamp(R + disc z_j, v_min,
// v_max) -- R alone where mask == 0: a select, not a product --, b_j = (t_j - v_min) / dz is t_j's position on the support, and atom i receives
//   m_i = sum_j p_j max(0, 1 - |b_j - i|),  j = 0 ... K - 1 in this order, in fp64, rounded to float32 once.
// A lane owns the atoms i = part, part + 32, ...; the b_j and p_j of 32 atoms at a time are formed one per lane and handed round by shuffles.
// p: the row's K probabilities (LDS or global), m: its K outputs (null: nothing is stored); the two must not overlap
__device__ __forceinline__ void c51_project_row(const C51Dev &D, const float *p, float R, float mask, float disc, float *m) {
    const int part = threadIdx.x & 31, base = threadIdx.x & 32, K = D.K;
    const int Kr = (K + 31) & ~31;                                  // (every lane runs every iteration: the shuffles read all 32)
    for (int i = part; i < Kr; i += 32) {
        double acc = 0.0;
        for (int j0 = 0; j0 < K; j0 += 32) {
            const int j = j0 + part;
            double bj = 0.0, pj = 0.0;
            if (j < K) {
                const double zj = D.v_min + (double)j * D.dz;
                double t = mask != 0.f ? (double)R + (double)disc * zj : (double)R;
                t = t < D.v_min ? D.v_min : (t > D.v_max ? D.v_max : t);
                bj = (t - D.v_min) / D.dz;
                pj = (double)p[j];
            }
            const int nj = K - j0 < 32 ? K - j0 : 32;
            for (int jj = 0; jj < nj; ++jj) {
                const double b = __shfl(bj, base + jj), pv = __shfl(pj, base + jj);
                const double w = 1.0 - fabs(b - (double)i);
                if (w > 0.0) acc += pv * w;
            }
        }
        if (i < K && m) m[i] = (float)acc;
    }
}

// ---- forward / backward -------------------------------------------------------------------------------------------------------------------------
// dbg4 (may be null) float32 [B][4]: a*, the target net's expected value there, l, Q(s, a); dist (may be null) float32 [B][2][K]: m and softmax p(s, a)
// (DUEL: the dueling head, a template argument as NS is -- the plain head's kernel then holds the code it held without the dueling head, at its registers)
template <bool NS, bool DUEL>
__device__ __forceinline__ void c51_fwd_pass(const C51Dev &D, int B, int gate, float *__restrict__ dbg4, float *__restrict__ dist, unsigned char *dg_smem) {
    const DdpgDev &L = D.dq.base;
    if (!ddpg_gate(L, gate)) return;
    const int Ap = D.dq.Ap, K = D.K;
    const DdpgTile T = ddpg_tile(dg_smem, L.h1p, Ap);
    float *M = c51_m_tile(T);
    const int tid = threadIdx.x, r0 = blockIdx.x * AT_TM, row = tid >> 5, part = tid & 31;
    const bool valid = r0 + row < B;
    const long long fill = L.cnt[DG_FILL], upd = L.cnt[DG_UPDATES];
    int act = 0;
    {   // gather (k_dqn_fwd's): X = s, Xn = s', sc = (reward, mask) or, n-step, (R, mask, gamma^m)
        const long long idx = valid ? dg_row_index(L, upd, fill, r0 + row) : 0;
        const float *src = L.ring + (size_t)idx * DG_ROW;
        if (NS) nstep_gather_tile(L, T.X, T.Xn, T.sc, idx, valid);
        else {
            T.X[row * AT_KIN + part] = valid ? src[part] : 0.f;
            T.Xn[row * AT_KIN + part] = valid ? src[32 + part] : 0.f;
            if (part < 2) T.sc[row * 4 + part] = valid ? src[DG_R + part] : 0.f;
        }
        act = valid ? (int)src[DQ_ACTION] : 0;
    }
    __syncthreads();
    float *h2 = T.H2 + (size_t)row * T.h2_ld, *mrow = M + (size_t)row * K;
    int astar = 0;
    float qsel;
    if (D.dq.dbl) {                                                 // a* from the online net's expected values on s'
        dqn_q(D.dq, T, T.Xn, false);
        if (DUEL) c51_dueling_combine(D, h2);
        astar = c51_greedy(D, h2, qsel, nullptr);
        __syncthreads();
    }
    dqn_q(D.dq, T, T.Xn, true);
    if (DUEL) c51_dueling_combine(D, h2);
    if (!D.dq.dbl) astar = c51_greedy(D, h2, qsel, nullptr);
    {   // p' = softmax of the target net's block a*, in place over its logits (each lane its own columns), and its mean
        float *blk = h2 + (size_t)astar * K;
        double mx, se;
        c51_block_stats(blk, K, mx, se);
        double s = 0.0;
        for (int k = part; k < K; k += 32) {
            const double pk = exp((double)blk[k] - mx) / se;
            s += (D.v_min + (double)k * D.dz) * pk;
            blk[k] = (float)pk;
        }
        qsel = (float)c51_row_sum(s);
        __syncthreads();
        c51_project_row(D, blk, T.sc[row * 4 + 0], T.sc[row * 4 + 1], ddpg_discount<NS>(L, T), mrow);
    }
    __syncthreads();
    // logits of the online net on s; log-softmax of the stored action's block
    dqn_q(D.dq, T, T.X, false);
    constexpr bool duel = DUEL;
    if (duel) c51_dueling_combine(D, h2);
    const float *blk = h2 + (size_t)act * K;
    double mx, se;
    c51_block_stats(blk, K, mx, se);
    const double lse = log(se);
    const double wB = valid ? (L.aw ? (double)L.aw[r0 + row] : 1.0) / (double)B : 0.0;
    double sl = 0.0, sq = 0.0;
    float *dout = L.aD2 + (size_t)(r0 + row) * Ap;
    const int A = D.dq.A;
    if (duel) { for (int j = (A + 1) * K + part; j < Ap; j += 32) dout[j] = 0.f; }                  // (the pad columns; the rest is dense, below)
    else for (int j = part; j < Ap; j += 32) if (j < act * K || j >= (act + 1) * K) dout[j] = 0.f;
    for (int k = part; k < K; k += 32) {
        const double xs = (double)blk[k] - mx, pk = exp(xs) / se, mk = (double)mrow[k];
        sl += mk * (xs - lse);
        sq += (D.v_min + (double)k * D.dz) * pk;
        const float dzk = valid ? (float)(wB * (pk - mk)) : 0.f;
        if (dist && valid) { float *o = dist + (size_t)(r0 + row) * 2 * K; o[k] = mrow[k]; o[K + k] = (float)pk; }
        if (duel) {                                                 // dense: over this lane's own column of every block of h2, whose logits are read no more
            const double g = valid ? wB * (pk - mk) : 0.0, invA = 1.0 / (double)A;
            for (int b = 0; b < A; ++b) {
                const float db = valid ? (float)(g * ((b == act ? 1.0 : 0.0) - invA)) : 0.f;
                dout[b * K + k] = db;
                h2[b * K + k] = db;
            }
            dout[A * K + k] = dzk;
            h2[A * K + k] = dzk;
        } else {
            dout[act * K + k] = dzk;
            mrow[k] = dzk;                                          // (this lane's own atom: m is read no more)
        }
    }
    const float loss = (float)(-c51_row_sum(sl)), qv = (float)c51_row_sum(sq);
    if (part == 0) {
        if (L.atd) L.atd[r0 + row] = valid ? loss : 0.f;
        L.adz[r0 + row] = (float)wB;
        L.arow[2 * (r0 + row)] = valid ? loss : 0.f;
        L.arow[2 * (r0 + row) + 1] = valid ? qv : 0.f;
        if (dbg4 && valid) { float *o = dbg4 + 4 * (size_t)(r0 + row); o[0] = (float)astar; o[1] = qsel; o[2] = loss; o[3] = qv; }
    }
    ddpg_store_tile(T.X, AT_KIN, L.aX + (size_t)r0 * AT_KIN, AT_KIN);
    ddpg_store_tile(T.H1, T.h1_ld, L.aH1 + (size_t)r0 * L.h1p, L.h1p);
    __syncthreads();
    // dZ1[row][k] = sum_i dZout[a K + i] W1[a K + i][k] where H1 > 0: the K rows of the action's block, in i order, in fp64 (the products are exact there);
    // the dueling head's dZout is dense: all (A + 1) K rows, in row order, read from the row's own h2
    if (duel) {
        const float *w1 = L.q.w + dg_o_w1(L.h1p);
        const int nr = (A + 1) * K;
        for (int k = part; k < L.h1p; k += 32) {
            double s = 0.0;
            for (int i = 0; i < nr; ++i) s += (double)h2[i] * (double)w1[(size_t)i * L.h1p + k];
            L.aD1[(size_t)(r0 + row) * L.h1p + k] = T.H1[(size_t)row * T.h1_ld + k] > 0.f ? (float)s : 0.f;
        }
        return;
    }
    const float *w1a = L.q.w + dg_o_w1(L.h1p) + (size_t)act * K * L.h1p;
    for (int k = part; k < L.h1p; k += 32) {
        double s = 0.0;
        for (int i = 0; i < K; ++i) s += (double)mrow[i] * (double)w1a[(size_t)i * L.h1p + k];
        L.aD1[(size_t)(r0 + row) * L.h1p + k] = T.H1[(size_t)row * T.h1_ld + k] > 0.f ? (float)s : 0.f;
    }
}
template <bool DUEL>
__device__ __forceinline__ void c51_fwd_body(const C51Dev &D, int B, int gate, float *__restrict__ dbg4, float *__restrict__ dist, unsigned char *dg_smem) {
    if (D.dq.base.n_step > 1) c51_fwd_pass<true, DUEL>(D, B, gate, dbg4, dist, dg_smem);
    else c51_fwd_pass<false, DUEL>(D, B, gate, dbg4, dist, dg_smem);
}
__global__ void __launch_bounds__(AT_THREADS) k_c51_fwd(C51Dev D, int B, int gate, float *__restrict__ dbg4, float *__restrict__ dist) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dg_smem[];
    c51_fwd_body<false>(D, B, gate, dbg4, dist, dg_smem);
}
// the dueling head's: the host launches it for a learner whose D.dueling is set (one head per learner and per population: the choice is uniform)
__global__ void __launch_bounds__(AT_THREADS) k_c51_fwd_duel(C51Dev D, int B, int gate, float *__restrict__ dbg4, float *__restrict__ dist) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dg_smem[];
    c51_fwd_body<true>(D, B, gate, dbg4, dist, dg_smem);
}

__global__ void __launch_bounds__(64 * DG_WG_WAVES) k_c51_wgrad(C51Dev D, int Bp, int gate) {
    __shared__ double part_s[DG_WG_WAVES][256];
    ddpg_wgrad_body(D.dq.base, 1, Bp, gate, part_s);
}

__global__ void __launch_bounds__(256) k_c51_adam(C51Dev D, float lr, int mode, int gate) { dqn_adam_body(D.dq, lr, mode, gate); }

// padded parameter layout -> W0 [h1][n_obs] | b0 [h1] | W1 [W][h1] | b1 [W], row-major, unpadded (k_dqn_unpad with W = dq.base.h2 output rows: A K,
// or (A + 1) K of a dueling head)
__global__ void k_c51_unpad(C51Dev D, const float *__restrict__ src, float *__restrict__ dst) {
    const DdpgDev &L = D.dq.base;
    const int AK = L.h2;
    const int n0 = L.h1 * L.n_obs, n1 = n0 + L.h1, n2 = n1 + AK * L.h1, total = n2 + AK;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        int s;
        if (i < n0) s = (i / L.n_obs) * AT_KIN + i % L.n_obs;
        else if (i < n1) s = dg_o_b0(L.h1p) + (i - n0);
        else if (i < n2) s = dg_o_w1(L.h1p) + ((i - n1) / L.h1) * L.h1p + (i - n1) % L.h1;
        else s = dg_o_b1(L.h1p, D.dq.Ap) + (i - n2);
        dst[i] = src[s];
    }
}

__global__ void __launch_bounds__(64) k_c51_stats(C51Dev D, int B, double *out) { ddpg_stats_body(D.dq.base, B, out); }

// debug: m [n][K] = the projection of p [n][K] under (R, mask, disc) [n] each: c51_project_row on rows that come from the caller
__global__ void __launch_bounds__(AT_THREADS) k_c51_project(C51Dev D, int n, const float *__restrict__ p, const float *__restrict__ R, const float *__restrict__ mask,
                                                            const float *__restrict__ disc, float *__restrict__ m) {
    const int r = blockIdx.x * AT_TM + (threadIdx.x >> 5);
    const bool valid = r < n;
    const size_t o = valid ? (size_t)r * D.K : 0;                    // (a row past the end projects row 0 and stores nothing: every lane runs the shuffles)
    const int rr = valid ? r : 0;
    c51_project_row(D, p + o, R[rr], mask[rr], disc[rr], valid ? m + o : nullptr);
}

// ---- acting -------------------------------------------------------------------------------------------------------------------------------------
// k_dqn_act with the expected values in Q's place: the greedy index is their first maximum; the epsilon draw has k_dqn_act's stream constant and
// counter rule.  dbg_q (may be null) float32 [N][A]: the expected values.  (A __device__ body like the others: k_c51_act_pop of
// stmpc_c51_pop_kernels.hpp runs it on the member blockIdx.y selects)
__device__ __forceinline__ void c51_act_body(const C51Dev &D, int N, const float *__restrict__ obs, int obs_stride, float eps, int explore,
                                             int *__restrict__ action, float *__restrict__ dbg_q, unsigned char *dg_smem) {
    const DdpgDev &L = D.dq.base;
    const DdpgTile T = ddpg_tile(dg_smem, L.h1p, D.dq.Ap);
    const int tid = threadIdx.x, e0 = blockIdx.x * AT_TM, row = tid >> 5, part = tid & 31, e = e0 + row;
    const long long acts = L.cnt[DG_ACTS];
    T.X[row * AT_KIN + part] = e < N && part < L.n_obs ? obs[(size_t)e * obs_stride + part] : 0.f;
    __syncthreads();
    dqn_q(D.dq, T, T.X, false);
    if (D.dueling) c51_dueling_combine(D, T.H2 + (size_t)row * T.h2_ld);
    float qbest;
    int a = c51_greedy(D, T.H2 + (size_t)row * T.h2_ld, qbest, dbg_q && e < N ? dbg_q + (size_t)e * D.dq.A : nullptr);
    if (e < N && part == 0) {
        if (explore) {
            const unsigned long long h = dg_hash(L.seed ^ DQN_STREAM, (unsigned long long)acts, (unsigned long long)e);
            const float u = (float)(unsigned int)(h >> 40) * 5.9604644775390625e-8f;      // [0, 1): a multiple of 2^-24, exact in float32
            if (u < eps) a = (int)((unsigned int)((h >> 16) & 0xFFFFFFull) % (unsigned int)D.dq.A);
        }
        action[e] = a;
    }
    __syncthreads();
    if (explore && tid == 0 && dg_last_block(L.tick + DG_T_ACT, gridDim.x)) L.cnt[DG_ACTS] = acts + 1;
}
__global__ void __launch_bounds__(AT_THREADS) k_c51_act(C51Dev D, int N, const float *__restrict__ obs, int obs_stride, float eps, int explore,
                                                        int *__restrict__ action, float *__restrict__ dbg_q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dg_smem[];
    c51_act_body(D, N, obs, obs_stride, eps, explore, action, dbg_q, dg_smem);
}

}  // namespace stmpc
